#!/usr/bin/env python3
"""Packed threshold decryption: many small sums per decryption.

Signed values are encrypted, summed in groups on the ciphertexts (homomorphic.sum_groups), packed 64 sums of 32 bits
per ciphertext at key_length 2048 (packing.pack: the packing kernel modulo N^2), threshold-decrypted by three parties and
unpacked (packing.unpack); the sums are checked against the plain ones.  The key is synthetic
(protocols.distributed_keygen_amd.synthetic); every modular step runs on the GPU.
   python examples/packed_threshold_decrypt.py [--key-length 2048] [--groups 1000] [--group-size 16]
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
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--group-size", type=int, default=16)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, homomorphic, packing, synthetic

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    rng = random.Random(1)
    g, s = args.groups, args.group_size
    x = [rng.randrange(-(1 << 20), 1 << 20) for _ in range(g * s)]       # sums of 16 stay well inside 32-bit slots
    t0 = time.perf_counter()
    cts = eng.encrypt_batch([v % n for v in x], [rng.randrange(1, n) for _ in x], n)
    sums = homomorphic.sum_groups([cts[j * s : (j + 1) * s] for j in range(g)], n=n, engine=eng)
    t1 = time.perf_counter()
    packed = packing.pack(sums, 32, n=n, engine=eng)
    packed = eng.randomize_batch(packed, [rng.randrange(1, n) for _ in packed], n)   # fresh before they leave the party
    t2 = time.perf_counter()
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = packed if e >= 0 else eng.modinv_batch(packed, n2)
        partials.append(eng.powmod_nsquare_batch(bases, abs(e), n))
    out, ok = eng.combine_batch([list(p) for p in zip(*partials)], n, key.theta_inv)
    got = packing.unpack(out, 32, g, n, signed=True)
    t3 = time.perf_counter()
    want = [sum(x[j * s : (j + 1) * s]) for j in range(g)]
    assert all(ok) and got == want, "the packed sums did not survive the round trip"
    print(f"key_length {args.key_length}: {g} sums of {s} signed values, {packing.slots_per_ciphertext(n, 32)} per ciphertext "
          f"-> {len(packed)} decryptions instead of {g}: encrypt + sums {1e3 * (t1 - t0):.1f} ms, pack {1e3 * (t2 - t1):.1f} ms, "
          f"threshold decryption + unpack {1e3 * (t3 - t2):.1f} ms — all {g} sums correct")


if __name__ == "__main__":
    main()
