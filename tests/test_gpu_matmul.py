"""Encrypted matrix products over a batch of ciphertext vectors on the GPU (csrc/mx_matmul_n2.hpp,
Engine.matmul_nsquare_t, homomorphic.matmul), bit-exact against pow and against the single-vector linear map."""

from __future__ import annotations

import ctypes
import math
import random

import pytest

import hostpow

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def odd_modulus(bits: int, rng: random.Random) -> int:
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def key_n(key_length: int) -> int:
    from protocols.distributed_keygen_amd import synthetic

    return synthetic.make_key(key_length, 3, 1).n


def units(rng, n, count):
    """Residues modulo n^2 that are coprime to n (a negative weight inverts them)."""
    out = []
    while len(out) < count:
        v = rng.randrange(1, n * n)
        if math.gcd(v, n) == 1:
            out.append(v)
    return out


def want_matmul(samples, weights, n, bias=None):
    """[[(1 + (bias_j mod n) n) prod_i x_i^W_ji mod n^2]] through hostpow (inverses for the negative weights)."""
    n2 = n * n
    jobs, shape = [], []
    for smp in samples:
        for row in weights:
            items = [(i, w) for i, w in (row.items() if isinstance(row, dict) else enumerate(row)) if w]
            shape.append(len(items))
            jobs += [(smp[i] % n2 if w > 0 else pow(smp[i], -1, n2), abs(w), n2) for i, w in items]
    powers = hostpow.powmod_many(jobs)
    out, at, k = [], 0, 0
    for smp in samples:
        ys = []
        for j in range(len(weights)):
            acc = (1 + (bias[j] % n) * n) % n2 if bias is not None else 1
            for v in powers[at : at + shape[k]]:
                acc = acc * v % n2
            at += shape[k]
            k += 1
            ys.append(acc)
        out.append(ys)
    return out


@pytest.mark.parametrize("key_length", [128, 2048, "odd"])
def test_matches_pow_and_the_single_vector_map(eng, key_length):
    rng = random.Random(f"matmul {key_length}")
    n = key_n(key_length) if key_length != "odd" else odd_modulus(1531, rng)
    samples = [units(rng, n, 7) for _ in range(5)]                  # B = 5: no multiple of 64 / K
    dense = [[rng.randrange(-(1 << 63), 1 << 63) for _ in range(7)],
             [0, 1, -1, (1 << 64) - 1, -(1 << 64), rng.randrange(n * n), -rng.randrange(n * n)],
             [rng.randrange(-1000, 1000) for _ in range(7)]]
    sparse = [{0: 3, 6: -(1 << 100)}, {}, {5: rng.getrandbits(64), 2: -1, 3: 0}]
    bias = [rng.randrange(n), -5, n + 7]
    for weights in (dense, sparse):
        got = eng.ciphertext_matmul_batch(samples, weights, n, bias=bias)
        assert got == want_matmul(samples, weights, n, bias)
        assert got == [eng.ciphertext_linear_map_batch(smp, weights, n, bias=bias) for smp in samples]
    assert eng.ciphertext_matmul_batch(samples, dense, n) == want_matmul(samples, dense, n)


def test_every_instance_has_a_parity_case(eng):
    from protocols.distributed_keygen_amd import limbs

    lib = eng.lib
    cnt = lib.mx_matmul_nsquare_instances(None, None, 0)
    lanes, lpls = (ctypes.c_int * cnt)(), (ctypes.c_int * cnt)()
    assert lib.mx_matmul_nsquare_instances(lanes, lpls, cnt) == cnt
    want = {(lanes[i], lpls[i]) for i in range(cnt)}
    rng = random.Random(17)
    seen = set()
    for bits in (130, 200, 400, 900, 2000, 3000, 4000, 6000, 8000):
        n = odd_modulus(bits, rng)
        n2 = n * n
        k, l, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        tile, ch = ctypes.c_int64(), ctypes.c_int64()
        assert lib.mx_matmul_nsquare_shape(bits, 4, 5, 4, 70, 3, 256 << 20, 0, 0, k, l, w, tile, ch) == 0
        seen.add((k.value, l.value))
        samples = [[rng.randrange(n2) for _ in range(3)] + [n2 + 3] for _ in range(3)]          # B = 3, I = 4
        W = [[rng.getrandbits(70) for _ in range(4)] for _ in range(5)]                         # R = 5
        W[1] = [0, 1, 2, 3]
        want_y = [v for ys in want_matmul(samples, W, n) for v in ys]
        x_t = eng.to_device(limbs.pack_reduced([c for smp in samples for c in smp], limbs.limbs_for(n2), n2))
        for window in (0, 1, 8):
            got = limbs.unpack(eng.to_host(eng.matmul_nsquare_t(x_t, 3, W, n, window=window)))
            assert got == want_y, (bits, window)
    assert seen == want


@pytest.mark.parametrize("window", [1, 4])
@pytest.mark.parametrize("batch", [40, 70])
def test_rows_of_zero_and_sparse_digits_match_pow(eng, window, batch):
    """Values only (that zero digits are skipped is a matter of time: tools/matmul_probe.py): an all-zero row, a row of powers of two (most digits zero) and a dense random row.  key_length 128
    runs groups of one lane, 64 samples per wavefront: 40 samples leave every wavefront ragged (3 x 40 outputs would put
    two weight rows into one wavefront if the rows were not padded), 70 give a full and a ragged wavefront per row."""
    from protocols.distributed_keygen_amd import limbs

    rng = random.Random(f"vote {window} {batch}")
    n = key_n(128)
    n2 = n * n
    assert eng.matmul_nsquare_shape(n, 9, 3, 9, 16, batch, 256 << 20)[1] == batch       # one tile
    samples = [units(rng, n, 9) for _ in range(batch)]
    W = [[0] * 9,
         [1 << rng.randrange(16) for _ in range(8)] + [-(1 << 15)],
         [rng.randrange(-(1 << 15), 1 << 15) for _ in range(9)]]
    want = [v for ys in want_matmul(samples, W, n, [0, 3, 0]) for v in ys]
    x_t = eng.to_device(limbs.pack_reduced([c for smp in samples for c in smp], limbs.limbs_for(n2), n2))
    got = limbs.unpack(eng.to_host(eng.matmul_nsquare_t(x_t, batch, W, n, bias=[0, 3, 0], window=window)))
    assert got == want


def test_tiles_and_split_k_on_the_device(eng):
    from protocols.distributed_keygen_amd import limbs

    rng = random.Random(23)
    n = key_n(128)
    n2 = n * n
    batch, cols = 37, 130
    samples = [units(rng, n, cols) for _ in range(batch)]
    W = [[rng.randrange(-(1 << 15), 1 << 15) or 1 for _ in range(cols)]]
    # a budget that holds 10 samples of the table columns, at the window the library picks when everything fits
    free = eng._matmul_plan(n, cols, batch, W, [5], table_budget=1 << 40)
    assert free.tile_batch == batch and free.n_cols == cols
    lanes = ctypes.c_int()
    assert eng.lib.mx_matmul_nsquare_shape(n.bit_length(), 1, 1, 1, 1, 1, 0, 0, 0, lanes, ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()) == 0
    budget = 10 * free.n_cols * ((2 * lanes.value * 9 * 4) << free.window) + 1000
    plan = eng._matmul_plan(n, cols, batch, W, [5], table_budget=budget)
    assert plan.tile_batch == 10 and plan.combine and len(plan.part_rows) >= 2          # ragged last tile of 7; split-K by itself
    x_t = eng.to_device(limbs.pack_reduced([c for smp in samples for c in smp], limbs.limbs_for(n2), n2))
    got = limbs.unpack(eng.to_host(eng.matmul_nsquare_t(x_t, batch, W, n, bias=[5], table_budget=budget)))
    assert got == [v for ys in want_matmul(samples, W, n, [5]) for v in ys]


def test_refusals_and_empty_shapes(eng):
    n = key_n(128)
    with pytest.raises(ValueError):
        eng.ciphertext_matmul_batch([[3, 5], [7, n]], [[1, -1]], n)          # a negative weight on a non-invertible input
    with pytest.raises(ValueError):
        eng.ciphertext_matmul_batch([[3, 5], [7]], [[1, 1]], n)
    with pytest.raises(ValueError):
        eng.ciphertext_matmul_batch([[3, 5]], [[1, 1, 1]], n)
    with pytest.raises(ValueError):
        eng.ciphertext_matmul_batch([[3, 5]], [[1, 1]], n, bias=[1, 2])
    assert eng.ciphertext_matmul_batch([], [[1, 1]], n) == []                # B = 0
    assert eng.ciphertext_matmul_batch([[3, 5], [7, 9]], [], n) == [[], []]   # R = 0
    assert eng.ciphertext_matmul_batch([[], []], [[], {}], n, bias=[4, 0]) == [[1 + 4 * n, 1]] * 2      # I = 0
    assert eng.ciphertext_matmul_batch([[0, 7]], [[0, 2], [1, 1]], n) == [[49, 0]]      # a zero weight on a zero input gives 1


@pytest.fixture(scope="module")
def round_trip_case():
    from protocols.distributed_keygen_amd import synthetic

    rng = random.Random(29)
    key = synthetic.make_key(1024, 3, 1)
    m = [[rng.randrange(key.n) for _ in range(16)] for _ in range(4)]
    cts = [[synthetic.encrypt(key, v, rng) for v in row] for row in m]
    W = [[rng.randrange(-(1 << 63), 1 << 63) for _ in range(16)] for _ in range(8)]
    b = [rng.randrange(key.n) for _ in range(8)]
    want = [[(sum(w * v for w, v in zip(row, ms)) + bj) % key.n for row, bj in zip(W, b)] for ms in m]
    return key, cts, W, b, want


def threshold_decrypt(eng, key, y):
    n, n2 = key.n, key.n_square
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = y if e >= 0 else eng.modinv_batch(y, n2)
        partials.append(eng.powmod_nsquare_batch(bases, abs(e), n))
    out, ok = eng.combine_batch([[partials[i][k] for i in range(3)] for k in range(len(y))], n, key.theta_inv)
    assert all(ok)
    return out


def test_encrypted_matmul_round_trip(eng, round_trip_case):
    from protocols.distributed_keygen_amd import homomorphic

    key, cts, W, b, want = round_trip_case
    rng = random.Random(31)
    y = homomorphic.matmul(cts, W, n=key.n, bias=b, engine=eng)
    flat = [v for ys in y for v in ys]
    flat = eng.randomize_batch(flat, [rng.randrange(1, key.n) for _ in flat], key.n)
    assert threshold_decrypt(eng, key, flat) == [v for row in want for v in row]


def test_randomizer_changes_the_ciphertexts_and_not_the_plaintexts(eng, round_trip_case):
    from protocols.distributed_keygen_amd import homomorphic
    from protocols.distributed_keygen_amd.randomizer import FastRandomizer, generate_base

    key, cts, W, b, want = round_trip_case
    plain = homomorphic.matmul(cts, W, n=key.n, bias=b, engine=eng)
    fr = FastRandomizer(key.n, generate_base(key.n, rng=random.Random(37), engine=eng), engine=eng)
    fresh = homomorphic.matmul(cts, W, n=key.n, bias=b, engine=eng, randomizer=fr)
    assert [len(ys) for ys in fresh] == [8] * 4
    assert all(f != p for fs, ps in zip(fresh, plain) for f, p in zip(fs, ps))
    assert threshold_decrypt(eng, key, [v for ys in fresh for v in ys]) == [v for row in want for v in row]


@pytest.mark.parametrize("case,tile,window", [("key128", 70, 1), ("key128", 70, 4), ("odd8000", 3, 4)])
def test_matrix_product_and_convolution_entry_points_agree_on_the_one_kernel(eng, case, tile, window):
    """One product through mx_matmul_nsquare_run (stride = tile, no origin array) and through mx_conv_nsquare_run
    (index * tile, origin = 0 .. tile - 1, stride 1, one position per image): the same launch of the shared-weight
    kernel said twice, so both results are bit-identical to each other and to pow.  Three table columns and a tile of
    two or more samples make a dropped or misplaced stride visible; every row names the one shared table through a
    negative index.  key_length 128 runs groups of one lane (a full and a ragged wavefront per row at 70 samples), the
    8000-bit modulus groups of 32 (two per wavefront: one surplus group per row at 3 samples)."""
    import numpy as np
    import torch

    from protocols.distributed_keygen_amd import limbs
    from protocols.distributed_keygen_amd import multiexp_plan as mp
    from protocols.distributed_keygen_amd.engine import _ConvBackend

    rng = random.Random(f"one kernel {case} {tile} {window}")
    n = key_n(128) if case == "key128" else odd_modulus(8000, rng)
    n2 = n * n
    cols, rows = 3, 3
    lanes = ctypes.c_int()
    assert eng.lib.mx_matmul_nsquare_shape(n.bit_length(), cols, rows, cols + 1, 16, tile, 1 << 40, 0, 0, lanes, ctypes.c_int(),
                                           ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()) == 0
    assert lanes.value == (1 if case == "key128" else 32)
    x = [[rng.randrange(1, n2) for _ in range(tile)] for _ in range(cols)]          # x[column][sample]
    shared = rng.randrange(1, n2)
    orders = [[0, 1, 2, -1], [-1, 2, 0, 1], [1, -1, 2, 0]]                          # ~(-1) = shared table 0
    W = [[rng.randrange(1, 1 << 16) for _ in range(cols + 1)] for _ in range(rows)]
    W[1][2] = 0                                                                     # a zero weight among the terms
    index = np.array(orders, dtype=np.int32)
    weights = np.array(W, dtype=np.uint32).reshape(rows, cols + 1, 1)
    as_matmul = mp.Launch(rows=list(range(rows)), index=index, weights=weights, weight_bits=16)
    as_conv = mp.Launch(rows=list(range(rows)), index=np.where(index >= 0, index * tile, index).astype(np.int32),
                        weights=weights, weight_bits=16)
    jobs = [((x[i][b] if i >= 0 else shared), W[j][t], n2) for b in range(tile) for j in range(rows) for t, i in enumerate(orders[j])]
    powers = hostpow.powmod_many(jobs)
    want = [math.prod(powers[k : k + cols + 1]) % n2 for k in range(0, len(powers), cols + 1)]          # [sample][row]
    limbs2 = limbs.limbs_for(n2)
    be = _ConvBackend(eng, n, limbs2, n.bit_length())
    tables_t = eng.to_device(limbs.pack_reduced([v for col in x for v in col] + [shared], limbs2, n2))
    got_matmul = be.run_matmul(tables_t, cols, 1, tile, as_matmul, window)
    got_conv = be.run_conv(tables_t, cols * tile, 1, as_conv, window, np.arange(tile, dtype=np.int64), 1)
    assert got_matmul.shape == got_conv.shape == (tile * rows, limbs2)
    assert torch.equal(got_matmul, got_conv)
    assert limbs.unpack(eng.to_host(got_matmul)) == want
    assert limbs.unpack(eng.to_host(got_conv)) == want
