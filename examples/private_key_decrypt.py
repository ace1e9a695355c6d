#!/usr/bin/env python3
"""Encrypted scoring decrypted with an ordinary private key: slots.encrypt -> homomorphic.matmul -> private decrypt -> decode.

The scoring side packs B samples of I small signed features across the slots of one plaintext per feature and scores them
with a public W and bias (as examples/slot_packed_scoring.py does).  The decrypting party here holds a plain Paillier key
— it knows the primes p and q of N — so the J x R result ciphertexts are decrypted by the CRT route
(PaillierPrivateKey.decrypt_t: two half-size modexps per ciphertext, csrc/mx_crt.hpp) and the plaintext rows go straight
into slots.decode_t on the device.  Compared with numpy.  The key is synthetic (its primes are known by construction);
every modular step runs on the GPU.
   python examples/private_key_decrypt.py [--key-length 2048] [--batch 4096] [--features 64] [--scores 4]
"""
import argparse
import random
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

VALUE_BITS, WEIGHT_BITS, BIAS_BITS = 8, 8, 10


def private_scores(eng, private_key, fr, x, W, bias):
    """x [B, I] int64 features, W [R, I], bias [R] -> (scores [B, R] as an int64 tensor on the device, slot width,
    ciphertexts decrypted).  Everything between the features and the scores is ciphertexts."""
    import torch

    from protocols.distributed_keygen_amd import homomorphic, limbs, packing, slots

    n, n2 = private_key.n, private_key.n_square
    B, I = x.shape
    R = W.shape[0]
    b = slots.slot_bits_for(VALUE_BITS, WEIGHT_BITS, I, BIAS_BITS)
    k = packing.slots_per_ciphertext(n, b)
    J = -(-B // k)
    cols = [slots.encrypt(np.ascontiguousarray(x[:, f]), fr, b) for f in range(I)]          # I x J ciphertexts
    packed_bias = [slots.encode([int(v)] * k, n, b, engine=eng)[0] for v in bias]             # beta_r in every slot
    out = homomorphic.matmul([[cols[f][j] for f in range(I)] for j in range(J)], W.tolist(), n=n, bias=packed_bias,
                             engine=eng, randomizer=fr)                                       # J x R ciphertexts
    flat = [out[j][r] for r in range(R) for j in range(J)]                                    # the plaintexts of score r in order
    cts_t = eng.to_device(limbs.pack_reduced(flat, limbs.limbs_for(n2), n2))
    rows_t, status_t = private_key.decrypt_t(cts_t, engine=eng)                               # rows in combine_t's format
    assert not bool(status_t.any()), "a ciphertext shares a factor with N"
    scores = torch.stack([slots.decode_t(rows_t[r * J : (r + 1) * J], n, b, B, engine=eng) for r in range(R)], dim=1)
    return scores, b, R * J


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--scores", type=int, default=4)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, PaillierPrivateKey, synthetic
    from protocols.distributed_keygen_amd.randomizer import FastRandomizer, generate_base

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    private_key = PaillierPrivateKey(key.p, key.q, engine=eng)
    rng = np.random.default_rng(1)
    B, I, R = args.batch, args.features, args.scores
    x = rng.integers(-(1 << (VALUE_BITS - 1)), 1 << (VALUE_BITS - 1), size=(B, I))
    W = rng.integers(-(1 << WEIGHT_BITS) + 1, 1 << WEIGHT_BITS, size=(R, I))
    bias = rng.integers(-(1 << BIAS_BITS) + 1, 1 << BIAS_BITS, size=R)
    fr = FastRandomizer(key.n, generate_base(key.n, rng=random.Random(1), engine=eng), engine=eng, device_rng=True)
    t0 = time.perf_counter()
    scores, b, n_dec = private_scores(eng, private_key, fr, x, W, bias)
    got = scores.cpu().numpy()
    t1 = time.perf_counter()
    assert (got == x @ W.T + bias).all(), "the encrypted scores differ from W x + bias"
    print(f"key_length {args.key_length}: {B} samples x {I} features -> {R} scores each in slots of {b} bits, "
          f"{n_dec} private-key decryptions instead of {B * R}, {1e3 * (t1 - t0):.1f} ms — all {B * R} scores equal numpy's")


if __name__ == "__main__":
    main()
