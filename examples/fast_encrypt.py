#!/usr/bin/env python3
"""Fixed-base encryption: a vector encrypted with a FastRandomizer, W x + b applied with fresh outputs
(linear_map(..., randomizer=...)), then threshold-decrypted by three parties.

The randomiser is h_s^a for a base h_s fixed per key and a short secret exponent a — NOT the reference's r^N; read the
docstring of protocols.distributed_keygen_amd.randomizer before using it.  The key is synthetic.
   python examples/fast_encrypt.py [--key-length 2048] [--dim 64] [--device-rng]
--device-rng draws the exponents on the GPU (protocols.distributed_keygen_amd.device_rng: what that generator is).
"""
import argparse
import random
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--device-rng", action="store_true", help="draw the secret exponents on the device (ChaCha20 kernel) instead of os.urandom")
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, FastRandomizer, generate_base, homomorphic, synthetic

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    rng = random.Random(1)
    d = args.dim
    x = [rng.randrange(-1000, 1000) for _ in range(d)]
    W = [[rng.randrange(-(1 << 63), 1 << 63) for _ in range(d)] for _ in range(d)]
    b = [rng.randrange(-1000, 1000) for _ in range(d)]
    t0 = time.perf_counter()
    # once per key: the base and (on first use) its table
    fr = FastRandomizer(n, generate_base(n, engine=eng), engine=eng, device_rng=True if args.device_rng else None)
    fr.randomizers(1)
    t1 = time.perf_counter()
    cts = fr.encrypt(x)
    t2 = time.perf_counter()
    y = homomorphic.linear_map(cts, W, n=n, bias=b, engine=eng, randomizer=fr)      # fresh before they leave the party
    t3 = time.perf_counter()
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = y if e >= 0 else eng.modinv_batch(y, n2)
        partials.append(eng.powmod_nsquare_batch(bases, abs(e), n))
    out, ok = eng.combine_batch([[partials[i][k] for i in range(3)] for k in range(d)], n, key.theta_inv)
    t4 = time.perf_counter()
    want = [(sum(w * v for w, v in zip(row, x)) + bj) % n for row, bj in zip(W, b)]
    assert all(ok) and out == want, "W x + b did not survive the round trip"
    print(f"key_length {args.key_length}, {d} x {d} map, exponents drawn on the {'device' if args.device_rng else 'host'}: base and table {1e3 * (t1 - t0):.1f} ms (once per key), encrypt "
          f"{1e3 * (t2 - t1):.1f} ms, W x + b with fresh outputs {1e3 * (t3 - t2):.1f} ms, threshold decryption "
          f"{1e3 * (t4 - t3):.1f} ms — all {d} outputs equal (W x + b) mod N")


if __name__ == "__main__":
    main()
