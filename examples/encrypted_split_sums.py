#!/usr/bin/env python3
"""Encrypted split sums: the left and right gradient sums of every split threshold of a gradient-boosted tree, from
encrypted gradients, without decrypting a histogram.

The label holder encrypts one gradient g_i per sample.  The feature holder knows every sample's bin under every feature
and computes the F x B bin sums H[f][b] with one homomorphic.histogram; then, still on ciphertexts,
    G_L[f][s] = sum_{b <= s} H[f][b]     (homomorphic.cumsum of every feature's bins)
    G_R[f][s] = sum_{b >= s} H[f][b]     (the same with reverse=True: no subtraction, so no inverse of any ciphertext)
— one modular product per bin and direction.  The 2 F B sums are packed 32 bits each (packing.pack), threshold-decrypted
by three parties, unpacked and compared with numpy's cumulative sums.  The key is synthetic
(protocols.distributed_keygen_amd.synthetic); every modular step runs on the GPU.
   python examples/encrypted_split_sums.py [--key-length 2048] [--samples 5000] [--features 10] [--bins 32]
"""
import argparse
import random
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

VALUE_BITS = 12           # g_i as a fixed-point value in [-2^11, 2^11): a sum over 2^19 samples stays inside a 32-bit slot


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--features", type=int, default=10)
    ap.add_argument("--bins", type=int, default=32)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, homomorphic, packing, synthetic

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    S, F, B = args.samples, args.features, args.bins
    assert S <= 1 << 19, "more samples need wider slots"
    rng = np.random.default_rng(1)
    py = random.Random(1)
    half = 1 << (VALUE_BITS - 1)
    g = rng.integers(-half, half, size=S)
    bins = rng.integers(-1, B, size=(F, S))                   # -1: the sample has no value for this feature
    # ---- label holder
    cts = eng.encrypt_batch([int(v) % n for v in g], [py.randrange(1, n) for _ in g], n)
    # ---- feature holder: bin sums, then the running sums from both ends, all on ciphertexts
    t0 = time.perf_counter()
    hist = homomorphic.histogram(cts, bins, B, n=n, engine=eng)
    t1 = time.perf_counter()
    left = homomorphic.cumsum(hist, n, engine=eng)
    right = homomorphic.cumsum(hist, n, reverse=True, engine=eng)
    t2 = time.perf_counter()
    sums = [c for rows in (left, right) for row in rows for c in row]
    packed = packing.pack(sums, 32, n=n, engine=eng)
    packed = eng.randomize_batch(packed, [py.randrange(1, n) for _ in packed], n)      # fresh before they leave the party
    # ---- three parties decrypt
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = packed if e >= 0 else eng.modinv_batch(packed, n2)
        partials.append(eng.powmod_nsquare_batch(bases, abs(e), n))
    out, ok = eng.combine_batch([list(p) for p in zip(*partials)], n, key.theta_inv)
    got = np.array(packing.unpack(out, 32, 2 * F * B, n, signed=True), dtype=np.int64).reshape(2, F, B)
    h = np.array([[g[bins[f] == b].sum() for b in range(B)] for f in range(F)])
    want_left = np.cumsum(h, axis=1)
    want_right = np.cumsum(h[:, ::-1], axis=1)[:, ::-1]
    assert all(ok) and (got[0] == want_left).all() and (got[1] == want_right).all(), "the encrypted split sums differ from numpy's"
    print(f"key_length {args.key_length}: {S} samples x {F} features in {B} bins: histogram {1e3 * (t1 - t0):.1f} ms, "
          f"G_L and G_R of all {F * B} thresholds {1e3 * (t2 - t1):.1f} ms (first calls: the key's plan included), "
          f"{len(packed)} packed threshold decryptions instead of {2 * F * B} — all {2 * F * B} sums equal numpy's")


if __name__ == "__main__":
    main()
