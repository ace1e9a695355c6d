#!/usr/bin/env python3
"""Encrypted convolution: a public kernel slid over an encrypted image.

A small image of signed 8-bit pixels is encrypted with a fixed-base FastRandomizer, convolved on the ciphertexts
(homomorphic.conv2d: O public kernels with a bias each, zero padding — the kernels are public plaintexts, every pixel gets
one table however many windows cover it, and the results are re-randomised on the device), packed 32 bits per output
(packing.pack), threshold-decrypted by three parties and compared with the plaintext convolution.  The key is synthetic
(protocols.distributed_keygen_amd.synthetic); every modular step runs on the GPU.
   python examples/encrypted_convolution.py [--key-length 2048] [--size 12] [--channels 1] [--kernels 4] [--ksize 3]
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
    ap.add_argument("--size", type=int, default=12)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=4)
    ap.add_argument("--ksize", type=int, default=3)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, homomorphic, packing, synthetic
    from protocols.distributed_keygen_amd.randomizer import FastRandomizer, generate_base

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    rng = np.random.default_rng(1)
    C, S, O, K = args.channels, args.size, args.kernels, args.ksize
    pad = K // 2
    x = rng.integers(-128, 128, size=(1, C, S, S))             # 8-bit pixels, 8-bit taps: outputs fit 32-bit slots
    w = rng.integers(-128, 128, size=(O, C, K, K))
    bias = rng.integers(-1000, 1000, size=O)
    fr = FastRandomizer(n, generate_base(n, rng=random.Random(1), engine=eng), engine=eng)
    t0 = time.perf_counter()
    flat = iter(fr.encrypt([int(v) for v in x.reshape(-1)]))
    cts = [[[[next(flat) for _ in range(S)] for _ in range(S)] for _ in range(C)]]
    t1 = time.perf_counter()
    y = homomorphic.conv2d(cts, w.tolist(), n=n, bias=[int(v) for v in bias], padding=pad, engine=eng, randomizer=fr)
    t2 = time.perf_counter()
    outs = [c for plane in y[0] for row in plane for c in row]
    packed = packing.pack(outs, 32, n=n, engine=eng, randomizer=fr)
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = packed if e >= 0 else eng.modinv_batch(packed, n2)
        partials.append(eng.powmod_nsquare_batch(bases, abs(e), n))
    out, ok = eng.combine_batch([list(p) for p in zip(*partials)], n, key.theta_inv)
    got = np.array(packing.unpack(out, 32, len(outs), n, signed=True)).reshape(O, len(y[0][0]), len(y[0][0][0]))
    t3 = time.perf_counter()
    xp = np.pad(x[0], ((0, 0), (pad, pad), (pad, pad)))
    oh, ow = got.shape[1:]
    want = np.array([[[int((xp[:, r : r + K, c : c + K] * w[o]).sum()) + int(bias[o]) for c in range(ow)] for r in range(oh)] for o in range(O)])
    assert all(ok) and (got == want).all(), "the encrypted convolution differs from the plaintext one"
    print(f"key_length {args.key_length}: {C} x {S} x {S} pixels under {O} kernels of {K} x {K}: encrypt {1e3 * (t1 - t0):.1f} ms, "
          f"encrypted convolution {1e3 * (t2 - t1):.1f} ms, pack + threshold decryption of {len(packed)} ciphertexts "
          f"{1e3 * (t3 - t2):.1f} ms — all {got.size} outputs equal the plaintext convolution")


if __name__ == "__main__":
    main()
