#!/usr/bin/env python3
"""Encrypted batch scoring: one public weight matrix applied to a batch of encrypted feature vectors.

B feature vectors of small signed integers are encrypted with a fixed-base FastRandomizer, scored on the ciphertexts
(homomorphic.matmul: W x_b + bias for every sample in one call — the weights are public plaintexts, W is planned and
uploaded once, and the results are re-randomised on the device), packed 32 bits per score (packing.pack),
threshold-decrypted by three parties and compared with numpy.  The key is synthetic
(protocols.distributed_keygen_amd.synthetic); every modular step runs on the GPU.
   python examples/encrypted_batch_scoring.py [--key-length 2048] [--batch 256] [--features 64] [--scores 4]
"""
import argparse
import random
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--scores", type=int, default=4)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, homomorphic, packing, synthetic
    from protocols.distributed_keygen_amd.randomizer import FastRandomizer, generate_base

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    rng = np.random.default_rng(1)
    B, I, R = args.batch, args.features, args.scores
    x = rng.integers(-128, 128, size=(B, I))                   # 8-bit features, 8-bit weights: scores fit 32-bit slots
    W = rng.integers(-128, 128, size=(R, I))
    bias = rng.integers(-1000, 1000, size=R)
    fr = FastRandomizer(n, generate_base(n, rng=random.Random(1), engine=eng), engine=eng)
    t0 = time.perf_counter()
    flat = fr.encrypt([int(v) for v in x.reshape(-1)])
    cts = [flat[b * I : (b + 1) * I] for b in range(B)]
    t1 = time.perf_counter()
    scores = homomorphic.matmul(cts, W.tolist(), n=n, bias=[int(v) for v in bias], engine=eng, randomizer=fr)
    t2 = time.perf_counter()
    packed = packing.pack([c for row in scores for c in row], 32, n=n, engine=eng, randomizer=fr)
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = packed if e >= 0 else eng.modinv_batch(packed, n2)
        partials.append(eng.powmod_nsquare_batch(bases, abs(e), n))
    out, ok = eng.combine_batch([list(p) for p in zip(*partials)], n, key.theta_inv)
    got = np.array(packing.unpack(out, 32, B * R, n, signed=True)).reshape(B, R)
    t3 = time.perf_counter()
    want = x @ W.T + bias
    assert all(ok) and (got == want).all(), "the encrypted scores differ from W x + bias"
    print(f"key_length {args.key_length}: {B} samples x {I} features -> {R} scores each: encrypt {1e3 * (t1 - t0):.1f} ms, "
          f"encrypted W x + bias {1e3 * (t2 - t1):.1f} ms, pack + threshold decryption of {len(packed)} ciphertexts "
          f"{1e3 * (t3 - t2):.1f} ms — all {B * R} scores equal numpy's")


if __name__ == "__main__":
    main()
