#!/usr/bin/env python3
"""Slot-packed encrypted scoring: the samples of a batch packed ACROSS the slots of one plaintext per feature.

B samples of I small signed features are packed feature by feature (slots.encrypt: slot s of the ciphertexts of feature f
holds sample s, k samples per ciphertext), scored with one public W and a bias on ceil(B / k) "samples" of I ciphertexts
(homomorphic.matmul: every weight multiplies all k slots at once; the bias is encoded once per slot), threshold-decrypted by
three parties and decoded on the device (Engine.combine_t -> slots.decode_t).  The slot width comes from slots.slot_bits_for:
the widest score W x + bias can produce, not the width of the inputs.  Compared with numpy.  The key is synthetic
(protocols.distributed_keygen_amd.synthetic); every modular step runs on the GPU.
   python examples/slot_packed_scoring.py [--key-length 2048] [--batch 4096] [--features 64] [--scores 4]
"""
import argparse
import random
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

VALUE_BITS, WEIGHT_BITS, BIAS_BITS = 8, 8, 10


def packed_scores(eng, key, fr, x, W, bias):
    """x [B, I] int64 features, W [R, I], bias [R] -> (scores [B, R] as an int64 tensor on the device, slot width,
    ciphertexts encrypted, ciphertexts decrypted).  Everything between the features and the scores is ciphertexts."""
    import torch

    from protocols.distributed_keygen_amd import homomorphic, limbs, packing, slots

    n, n2 = key.n, key.n_square
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
    l2 = limbs.limbs_for(n2)
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = flat if e >= 0 else eng.modinv_batch(flat, n2)
        partials.append(eng.powmod_nsquare_t(eng.to_device(limbs.pack_reduced(bases, l2, n2)), n, abs(e)))
    rows_t = eng.combine_t(torch.stack(partials), n, key.theta_inv, packed=True)
    assert not bool(rows_t[:, -1].any()), "a recombination was not divisible by N"
    scores = torch.stack([slots.decode_t(rows_t[r * J : (r + 1) * J], n, b, B, engine=eng) for r in range(R)], dim=1)
    return scores, b, I * J, R * J


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--scores", type=int, default=4)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, synthetic
    from protocols.distributed_keygen_amd.randomizer import FastRandomizer, generate_base

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    rng = np.random.default_rng(1)
    B, I, R = args.batch, args.features, args.scores
    x = rng.integers(-(1 << (VALUE_BITS - 1)), 1 << (VALUE_BITS - 1), size=(B, I))
    W = rng.integers(-(1 << WEIGHT_BITS) + 1, 1 << WEIGHT_BITS, size=(R, I))
    bias = rng.integers(-(1 << BIAS_BITS) + 1, 1 << BIAS_BITS, size=R)
    fr = FastRandomizer(key.n, generate_base(key.n, rng=random.Random(1), engine=eng), engine=eng, device_rng=True)
    t0 = time.perf_counter()
    scores, b, n_enc, n_dec = packed_scores(eng, key, fr, x, W, bias)
    got = scores.cpu().numpy()
    t1 = time.perf_counter()
    assert (got == x @ W.T + bias).all(), "the encrypted scores differ from W x + bias"
    print(f"key_length {args.key_length}: {B} samples x {I} features -> {R} scores each in slots of {b} bits: "
          f"{n_enc} encryptions instead of {B * I}, {n_dec} threshold decryptions instead of {B * R}, "
          f"{1e3 * (t1 - t0):.1f} ms — all {B * R} scores equal numpy's")


if __name__ == "__main__":
    main()
