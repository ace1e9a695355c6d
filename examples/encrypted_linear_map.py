#!/usr/bin/env python3
"""An encrypted linear layer: W x + b applied to an encrypted vector, then threshold-decrypted by three parties.

The key is synthetic (protocols.distributed_keygen_amd.synthetic); encryption, the linear map (homomorphic.linear_map:
the multi-exponentiation kernel modulo N^2), re-randomisation, partial decryption and recombination all run on the GPU.
   python examples/encrypted_linear_map.py [--key-length 2048] [--dim 64]
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
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, homomorphic, synthetic

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    rng = random.Random(1)
    d = args.dim
    x = [rng.randrange(-1000, 1000) for _ in range(d)]
    W = [[rng.randrange(-(1 << 63), 1 << 63) for _ in range(d)] for _ in range(d)]
    b = [rng.randrange(-1000, 1000) for _ in range(d)]
    t0 = time.perf_counter()
    cts = eng.encrypt_batch([v % n for v in x], [rng.randrange(1, n) for _ in x], n)
    t1 = time.perf_counter()
    y = homomorphic.linear_map(cts, W, n=n, bias=b, engine=eng)
    y = eng.randomize_batch(y, [rng.randrange(1, n) for _ in y], n)        # fresh ciphertexts before they leave the party
    t2 = time.perf_counter()
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = y if e >= 0 else eng.modinv_batch(y, n2)
        partials.append(eng.powmod_nsquare_batch(bases, abs(e), n))
    out, ok = eng.combine_batch([[partials[i][k] for i in range(3)] for k in range(d)], n, key.theta_inv)
    t3 = time.perf_counter()
    want = [(sum(w * v for w, v in zip(row, x)) + bj) % n for row, bj in zip(W, b)]
    assert all(ok) and out == want, "W x + b did not survive the round trip"
    print(f"key_length {args.key_length}, {d} x {d} map: encrypt {1e3 * (t1 - t0):.1f} ms, W x + b {1e3 * (t2 - t1):.1f} ms, "
          f"threshold decryption {1e3 * (t3 - t2):.1f} ms — all {d} outputs equal (W x + b) mod N")


if __name__ == "__main__":
    main()
