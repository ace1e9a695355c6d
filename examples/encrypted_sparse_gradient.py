#!/usr/bin/env python3
"""Encrypted gradient of a vertical linear or logistic regression over sparse features: X^T Enc(d).

The label holder encrypts the residuals d_i (fixed-point, signed) and sends them.  The feature holder has a sparse
feature matrix X — one-hot blocks of categorical features and a few sparse numeric columns in signed fixed point —
which is public to it, and computes the gradient X^T d of every column on the ciphertexts with ONE
homomorphic.sparse_matmul: X^T is handed over as a torch sparse COO tensor (a CSR triple of arrays works the same), and
nothing is planned term by term.  The results are packed, many sums per ciphertext (packing.pack), threshold-decrypted by
three parties and unpacked, and compared with numpy's X^T d.  The key is synthetic
(protocols.distributed_keygen_amd.synthetic); every modular step runs on the GPU.
   python examples/encrypted_sparse_gradient.py [--key-length 2048] [--samples 20000] [--categorical 8] [--categories 16] [--numeric 4]
"""
import argparse
import random
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

RESIDUAL_BITS = 16        # d_i as a fixed-point value in [-2^15, 2^15)
WEIGHT_BITS = 8           # numeric features as fixed-point values in (-2^8, 2^8)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--categorical", type=int, default=8)
    ap.add_argument("--categories", type=int, default=16)
    ap.add_argument("--numeric", type=int, default=4)
    ap.add_argument("--density", type=float, default=0.1, help="share of the samples with a value in a numeric column")
    args = ap.parse_args()
    import torch

    from protocols.distributed_keygen_amd import Engine, homomorphic, packing, slots, synthetic

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    S, F, C, Q = args.samples, args.categorical, args.categories, args.numeric
    rng = np.random.default_rng(1)
    py = random.Random(1)
    half = 1 << (RESIDUAL_BITS - 1)
    d = rng.integers(-half, half, size=S)
    # ---- feature holder's X^T as (column, sample, value) triples: F one-hot blocks of C columns, then Q numeric columns
    cat = rng.integers(0, C, size=(F, S))
    cols = [(np.arange(F)[:, None] * C + cat).reshape(-1)]
    samples = [np.tile(np.arange(S), F)]
    values = [np.ones(F * S, dtype=np.int64)]
    for q in range(Q):
        picked = np.flatnonzero(rng.random(S) < args.density)
        cols.append(np.full(picked.size, F * C + q))
        samples.append(picked)
        values.append(rng.integers(-(1 << WEIGHT_BITS) + 1, 1 << WEIGHT_BITS, size=picked.size))
    cols, samples, values = np.concatenate(cols), np.concatenate(samples), np.concatenate(values)
    n_cols = F * C + Q
    xt = torch.sparse_coo_tensor(torch.from_numpy(np.stack([cols, samples])), torch.from_numpy(values), size=(n_cols, S))
    # ---- label holder: the encrypted residuals
    cts = eng.encrypt_batch([int(v) % n for v in d], [py.randrange(1, n) for _ in range(S)], n)
    # ---- feature holder: the gradient of every column, on ciphertexts; packed before it leaves
    t0 = time.perf_counter()
    grad = homomorphic.sparse_matmul(cts, xt, n=n, engine=eng)
    t1 = time.perf_counter()
    b = slots.slot_bits_for(RESIDUAL_BITS, WEIGHT_BITS, S)
    packed = packing.pack(grad, b, n=n, engine=eng)
    packed = eng.randomize_batch(packed, [py.randrange(1, n) for _ in packed], n)    # fresh before they leave the party
    # ---- three parties decrypt the packed gradient
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = packed if e >= 0 else eng.modinv_batch(packed, n2)
        partials.append(eng.powmod_nsquare_batch(bases, abs(e), n))
    out, ok = eng.combine_batch([list(p) for p in zip(*partials)], n, key.theta_inv)
    got = packing.unpack(out, b, n_cols, n, signed=True)
    want = np.zeros(n_cols, dtype=np.int64)
    np.add.at(want, cols, values * d[samples])
    assert all(ok) and got == want.tolist(), "the encrypted gradient differs from numpy's"
    print(f"key_length {args.key_length}: X^T d for {S} encrypted residuals and {n_cols} sparse columns ({cols.size} non-zeros, "
          f"weights of up to {WEIGHT_BITS} bits) in {1e3 * (t1 - t0):.1f} ms (first call: the key's plan included), "
          f"{len(packed)} packed threshold decryptions of {packing.slots_per_ciphertext(n, b)} slots of {b} bits instead of {n_cols} — "
          f"all {n_cols} sums equal numpy's")


if __name__ == "__main__":
    main()
