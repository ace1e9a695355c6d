#!/usr/bin/env python3
"""The label holder's round trip with an ordinary private key: encrypt_slots -> homomorphic.histogram -> decrypt_t -> decode.

The label holder of a gradient-boosted tree knows the primes p and q of its own key.  It packs (g_i, h_i) as two signed
slots of ONE plaintext per sample and encrypts them with the reference's randomiser r^N through the CRT route
(PaillierPrivateKey.encrypt_slots: the plaintext rows never leave the device; one draw per ciphertext, two half-size
modexps, csrc/mx_crt_enc.hpp) — no FastRandomizer, no table, no extra assumption.  The feature holder computes all
F x B bin sums on the ciphertexts (homomorphic.histogram), and the label holder decrypts them by the CRT route
(decrypt_t) straight into slots.decode_t on the device.  Compared with numpy.  The key is synthetic (its primes are known
by construction); every modular step runs on the GPU.
   python examples/private_key_encrypt.py [--key-length 2048] [--samples 20000] [--features 10] [--bins 32]
"""
import argparse
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
    from protocols.distributed_keygen_amd import Engine, PaillierPrivateKey, homomorphic, limbs, packing, slots, synthetic

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    private_key = PaillierPrivateKey(key.p, key.q, engine=eng)
    n, n2 = private_key.n, private_key.n_square
    S, F, B = args.samples, args.features, args.bins
    rng = np.random.default_rng(1)
    half = 1 << (VALUE_BITS - 1)
    g = rng.integers(-half, half, size=S)
    h = rng.integers(-half, half, size=S)
    bins = rng.integers(-1, B, size=(F, S))                   # -1: the sample has no value for this feature
    # ---- label holder: two slots per plaintext, wide enough for a sum over all samples; fresh randomness of its own
    b = slots.slot_bits_for(VALUE_BITS, 0, S)
    k = packing.slots_per_ciphertext(n, b)
    vals = np.zeros((S, k), dtype=np.int64)
    vals[:, 0], vals[:, 1] = g, h
    t0 = time.perf_counter()
    cts = private_key.encrypt_slots(vals.reshape(-1), b)
    t1 = time.perf_counter()
    # ---- feature holder: every bin sum of every feature, on ciphertexts
    hist = homomorphic.histogram(cts, bins, B, n=n, engine=eng)
    # ---- label holder again: CRT decryption, the plaintext rows decoded on the device
    flat = [c for row in hist for c in row]
    rows_t, status_t = private_key.decrypt_t(eng.to_device(limbs.pack_reduced(flat, limbs.limbs_for(n2), n2)))
    assert not bool(status_t.any()), "a ciphertext shares a factor with N"
    dec = slots.decode_t(rows_t, n, b, F * B * k, engine=eng).cpu().numpy().reshape(F, B, k)
    want_g = np.array([[g[bins[f] == j].sum() for j in range(B)] for f in range(F)])
    want_h = np.array([[h[bins[f] == j].sum() for j in range(B)] for f in range(F)])
    assert (dec[:, :, 0] == want_g).all() and (dec[:, :, 1] == want_h).all(), "the encrypted bin sums differ from numpy's"
    print(f"key_length {args.key_length}: {S} samples of (g, h) in two slots of {b} bits encrypted with the private key in "
          f"{1e3 * (t1 - t0):.1f} ms (first call: the key's plans included), {F} features x {B} bins summed on ciphertexts, "
          f"{F * B} private-key decryptions — all {2 * F * B} sums equal numpy's")


if __name__ == "__main__":
    main()
