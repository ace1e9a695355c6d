#!/usr/bin/env python3
"""Encrypted gradient histograms: the per-feature, per-bin sums of encrypted (g_i, h_i) that a gradient-boosted tree is
grown from when the party that holds the features must not see the gradients (SecureBoost).

The label holder packs (g_i, h_i) as two signed slots of ONE plaintext per sample (slots.encode: slot 0 = g_i, slot 1 = h_i;
the slot width comes from slots.slot_bits_for with the sample count as the bound of a sum), encrypts the n plaintexts and
sends them.  The feature holder knows the bin of every sample under every feature — public to it — and computes all
F x B bin sums with one homomorphic.histogram: one modular product per (sample, feature), both slots at once, nothing
decrypted.  Three parties threshold-decrypt the F x B results and slots.decode splits them into the sums of g and of h.
Compared with numpy.  The key is synthetic (protocols.distributed_keygen_amd.synthetic); every modular step runs on the GPU.
   python examples/encrypted_gradient_histogram.py [--key-length 2048] [--samples 20000] [--features 10] [--bins 32]
"""
import argparse
import random
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

VALUE_BITS = 16           # g_i and h_i as fixed-point values in [-2^15, 2^15)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--features", type=int, default=10)
    ap.add_argument("--bins", type=int, default=32)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, homomorphic, packing, slots, synthetic
    from protocols.distributed_keygen_amd.shared_key import GpuPaillierSharedKey, PlainCiphertext, ShareView

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    n = key.n
    S, F, B = args.samples, args.features, args.bins
    rng = np.random.default_rng(1)
    half = 1 << (VALUE_BITS - 1)
    g = rng.integers(-half, half, size=S)
    h = rng.integers(-half, half, size=S)
    bins = rng.integers(-1, B, size=(F, S))                   # -1: the sample has no value for this feature
    # ---- label holder: two slots per plaintext, wide enough for a sum over all samples
    b = slots.slot_bits_for(VALUE_BITS, 0, S)
    k = packing.slots_per_ciphertext(n, b)
    vals = np.zeros((S, k), dtype=np.int64)
    vals[:, 0], vals[:, 1] = g, h
    plaintexts = slots.encode(vals.reshape(-1), n, b, engine=eng)
    py = random.Random(1)
    cts = eng.encrypt_batch(plaintexts, [py.randrange(1, n) for _ in plaintexts], n)
    # ---- feature holder: every bin sum of every feature, on ciphertexts
    t0 = time.perf_counter()
    hist = homomorphic.histogram(cts, bins, B, n=n, engine=eng)
    t1 = time.perf_counter()
    # ---- three parties decrypt the F x B sums
    keys = {i: GpuPaillierSharedKey(n, key.t, i, ShareView({i: key.shares[i]}, key.degree, key.n_fac), key.theta, engine=eng)
            for i in (1, 2, 3)}
    flat = [PlainCiphertext(c, n) for row in hist for c in row]
    parts = {i: sk.partial_decrypt_batch(flat) for i, sk in keys.items()}
    sums = keys[1].decrypt_batch([{i: parts[i][e] for i in keys} for e in range(len(flat))])
    dec = np.array(slots.decode(sums, n, b, F * B * k, engine=eng), dtype=np.int64).reshape(F, B, k)
    want_g = np.array([[g[bins[f] == j].sum() for j in range(B)] for f in range(F)])
    want_h = np.array([[h[bins[f] == j].sum() for j in range(B)] for f in range(F)])
    assert (dec[:, :, 0] == want_g).all() and (dec[:, :, 1] == want_h).all(), "the encrypted bin sums differ from numpy's"
    print(f"key_length {args.key_length}: {S} samples x {F} features in {B} bins, (g, h) in two slots of {b} bits: "
          f"{int((bins >= 0).sum())} encrypted additions in {1e3 * (t1 - t0):.1f} ms (first call: the key's plan included), {F * B} threshold decryptions — "
          f"all {2 * F * B} sums equal numpy's")


if __name__ == "__main__":
    main()
