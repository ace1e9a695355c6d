"""Encrypted sparse matrix products on the GPU (csrc/mx_spmm_n2.hpp, Engine.spmm_nsquare_t, homomorphic.sparse_matmul),
bit-exact against CPython's ``pow`` products and against ciphertext_linear_map_batch on the same rows given as dicts."""

from __future__ import annotations

import ctypes
import random

import numpy as np
import pytest

import spmm_cases as cases

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


CROW, COL, VAL, BIAS = cases.parity_matrix()
_cases = {}


def parity_case(key_length):
    """(n, inputs, expected without a bias, expected with it) of the shared parity matrix: computed once per modulus."""
    if key_length not in _cases:
        n = key_n(key_length) if key_length != "odd" else odd_modulus(1531, random.Random("spmm odd"))
        cts = cases.parity_inputs(n)
        _cases[key_length] = (n, cts, cases.expected(cts, CROW, COL, VAL, n), cases.expected(cts, CROW, COL, VAL, n, BIAS))
    return _cases[key_length]


def rows_of(eng, cts, n):
    from protocols.distributed_keygen_amd import limbs

    return eng.to_device(limbs.pack_reduced(cts, limbs.limbs_for(n * n), n * n))


def ints_of(eng, rows_t):
    from protocols.distributed_keygen_amd import limbs

    return limbs.unpack(eng.to_host(rows_t))


@pytest.mark.parametrize("key_length", [128, 2048, "odd"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_matches_pow_products_and_linear_map(eng, key_length, with_bias):
    n, cts, want, want_bias = parity_case(key_length)
    bias = BIAS if with_bias else None
    got = eng.ciphertext_spmm_batch(cts, CROW, COL, VAL, n, bias=bias)
    assert got == (want_bias if with_bias else want)
    assert want[0] == 1 and cts[2] >= n * n and BIAS[3] >= n and min(BIAS) < 0      # what the case is there for
    assert got == eng.ciphertext_linear_map_batch(cts, cases.dict_rows(CROW, COL, VAL), n, bias=bias)


@pytest.mark.parametrize("key_length", [128, 2048, "odd"])
def test_window_chunk_and_budget_overrides_change_nothing(eng, key_length):
    n, cts, want, want_bias = parity_case(key_length)
    x_t = rows_of(eng, cts, n)
    for window in range(1, 9):
        assert ints_of(eng, eng.spmm_nsquare_t(x_t, CROW, COL, VAL, n, bias=BIAS, window=window)) == want_bias, window
    for chunk in (1, 2, 0, 1000):
        assert ints_of(eng, eng.spmm_nsquare_t(x_t, CROW, COL, VAL, n, chunk=chunk)) == want, chunk
    # a budget below one table: every table is a stage of its own
    assert ints_of(eng, eng.spmm_nsquare_t(x_t, CROW, COL, VAL, n, bias=BIAS, table_budget_bytes=1)) == want_bias
    row_bytes = eng.spmm_nsquare_shape(n, 60, 9, 80, 63, 3)[2]
    assert ints_of(eng, eng.spmm_nsquare_t(x_t, CROW, COL, VAL, n, window=3, chunk=3, table_budget_bytes=30 * row_bytes)) == want


def test_index_tensors_on_either_side_and_sparse_tensors(eng):
    import torch

    from protocols.distributed_keygen_amd import homomorphic

    n, cts, want, want_bias = parity_case(2048)
    x_t = rows_of(eng, cts, n)
    host = [torch.tensor(v) for v in (CROW, COL, VAL)]
    dev = [t.to(eng.device) for t in host]
    out_t = eng.spmm_nsquare_t(x_t, *dev, n, bias=BIAS)
    assert out_t.is_cuda and out_t.dtype == torch.int32 and tuple(out_t.shape) == (cases.N_ROWS, x_t.shape[1])
    assert ints_of(eng, out_t) == want_bias
    assert ints_of(eng, eng.spmm_nsquare_t(x_t, *host, n, bias=BIAS)) == want_bias
    assert ints_of(eng, eng.spmm_nsquare_t(x_t, dev[0].to(torch.int32), np.array(COL, dtype=np.int32), VAL, n)) == want
    # torch's own sparse tensors: the CSR tensor keeps the duplicate and the stored zeros, the COO tensor goes through
    # torch's to_sparse_csr
    csr = torch.sparse_csr_tensor(host[0], host[1], host[2], size=(cases.N_ROWS, cases.N_IN))
    assert homomorphic.sparse_matmul(cts, csr, n=n, bias=BIAS, engine=eng) == want_bias
    row = torch.repeat_interleave(torch.arange(cases.N_ROWS), host[0][1:] - host[0][:-1])
    coo = torch.sparse_coo_tensor(torch.stack([row, host[1]]), host[2], size=(cases.N_ROWS, cases.N_IN))
    assert homomorphic.sparse_matmul(cts, coo, n=n, engine=eng) == want
    assert homomorphic.sparse_matmul(cts, (CROW, COL, VAL), n=n, engine=eng) == want


def test_a_multiple_of_n_is_legal_under_positive_weights_only(eng):
    n = key_n(128)
    cts = [5 * n, 7, 11, 0]
    crow, col = [0, 2, 4], [0, 1, 2, 3]
    val = [3, -2, 5, 1]
    assert eng.ciphertext_spmm_batch(cts, crow, col, val, n) == cases.expected(cts, crow, col, val, n)
    with pytest.raises(ValueError):
        eng.ciphertext_spmm_batch(cts, crow, col, [-3, -2, 5, 1], n)
    with pytest.raises(ValueError):
        eng.ciphertext_spmm_batch(cts, crow, col, [3, -2, 5, -1], n)


def test_weights_all_one_are_the_histogram(eng):
    n = key_n(128)
    rng = random.Random(23)
    cts = [rng.randrange(n * n) for _ in range(50)] + [0, 9 * n]
    bins = [rng.randrange(-1, 6) for _ in cts]
    members = [[i for i, b in enumerate(bins) if b == k] for k in range(6)]
    crow = [0]
    for m in members:
        crow.append(crow[-1] + len(m))
    col = [i for m in members for i in m]
    assert eng.spmm_nsquare_shape(n, len(cts), 6, len(col), 1)[:2] == (1, 1)
    assert eng.ciphertext_spmm_batch(cts, crow, col, [1] * len(col), n) == eng.ciphertext_histogram_batch(cts, [bins], 6, n)[0]


def test_every_instance_has_a_parity_case(eng):
    lib = eng.lib
    cnt = lib.mx_spmm_nsquare_instances(None, None, 0)
    lanes, lpls = (ctypes.c_int * cnt)(), (ctypes.c_int * cnt)()
    assert lib.mx_spmm_nsquare_instances(lanes, lpls, cnt) == cnt
    want = {(lanes[i], lpls[i]) for i in range(cnt)}
    rng = random.Random(19)
    seen = set()
    crow, col, val = [0, 3, 3, 5, 9], [0, 4, 8, 2, 2, 1, 3, 5, 7], [77, -1234, 5, 1, -9, 31000, -31000, 0, 2]
    for bits in (130, 200, 400, 900, 2000, 3000, 4000, 6000, 8000):
        n = odd_modulus(bits, rng)
        k, l = eng.histogram_nsquare_shape(n, 9, 6, 18)[:2]
        seen.add((k, l))
        cts = [cases.unit(rng, n) for _ in range(8)] + [n * n + 3]
        x_t = rows_of(eng, cts, n)
        for window, bias in ((0, None), (3, [5, -1, 2 * n + 1, 0])):
            got = ints_of(eng, eng.spmm_nsquare_t(x_t, crow, col, val, n, bias=bias, window=window))
            assert got == cases.expected(cts, crow, col, val, n, bias), (bits, window)
    assert seen == want


def test_two_calls_on_two_streams(eng):
    import torch

    n, cts, want, want_bias = parity_case(2048)
    x_t = rows_of(eng, cts, n)
    dev = [torch.tensor(v, device=eng.device) for v in (CROW, COL, VAL)]
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    a_t = eng.spmm_nsquare_t(x_t, *dev, n, chunk=2)                               # several levels in flight on this stream ...
    with torch.cuda.stream(side):
        b_t = eng.spmm_nsquare_t(x_t, *dev, n, bias=BIAS, window=2, chunk=2)     # ... while the side stream runs its own
    cur.wait_stream(side)
    assert ints_of(eng, a_t) == want
    assert ints_of(eng, b_t) == want_bias


def test_refusals_and_empty_shapes(eng):
    import torch

    n = key_n(128)
    cts = [3, 5, 7]
    x_t = rows_of(eng, cts, n)
    good = ([0, 2, 3], [0, 2, 1], [4, -5, 6])
    for crow, col, val in (([0, 2, 1, 3], [0, 2, 1], [4, -5, 6]), ([1, 2, 3], [0, 2, 1], [4, -5, 6]), ([0, 2, 2], [0, 2, 1], [4, -5, 6]),
                           ([0, 2, 3], [0, 3, 1], [4, -5, 6]), ([0, 2, 3], [0, 2, 1], [4, -(1 << 63), 6]),
                           ([0, 2, 3], [0, 2, 1], [4.0, -5.0, 6.0])):
        with pytest.raises(ValueError):
            eng.ciphertext_spmm_batch(cts, crow, col, val, n)
        with pytest.raises(ValueError):
            eng.spmm_nsquare_t(x_t, crow, col, val, n)
    with pytest.raises(ValueError):
        eng.spmm_nsquare_t(x_t, torch.tensor([0, 2, 3], device=eng.device), torch.tensor([0, 5, 1], device=eng.device),
                           torch.tensor([4, -5, 6], device=eng.device), n)
    for kw in (dict(bias=[1, 2, 3]), dict(window=9), dict(window=-1), dict(chunk=1 << 20)):
        with pytest.raises(ValueError):
            eng.spmm_nsquare_t(x_t, *good, n, **kw)
    with pytest.raises(ValueError):
        eng.ciphertext_spmm_batch(cts, *good, n + 1)                               # an even modulus
    n2 = n * n
    assert eng.ciphertext_spmm_batch(cts, *good, n) == [pow(3, 4, n2) * pow(7, -5, n2) % n2, pow(5, 6, n2)]
    assert eng.ciphertext_spmm_batch(cts, [0], [], [], n) == []                    # no rows
    assert eng.ciphertext_spmm_batch(cts, [0, 0, 0], [], [], n, bias=[2, -1]) == [1 + 2 * n, 1 + (n - 1) * n]
    assert eng.ciphertext_spmm_batch([], [0, 0], [], [], n) == [1]                 # no inputs
    assert eng.ciphertext_spmm_batch(cts, [0, 1, 2], [0, 1], [0, 0], n) == [1, 1]  # stored zeros only


class _Given:
    """A FastRandomizer whose next draw is a given list of exponents."""

    def __init__(self, fr, exps):
        self.fr, self.exps = fr, list(exps)

    def spec(self, n, count):
        return self.fr.spec(n, count, exponents=self.exps)


def test_randomizer_multiplies_every_row_by_its_power(eng):
    from protocols.distributed_keygen_amd import homomorphic, randomizer

    n, cts, want, want_bias = parity_case(2048)
    n2 = n * n
    rng = random.Random(47)
    h_s = randomizer.generate_base(n, rng=rng, engine=eng)
    fr = randomizer.FastRandomizer(n, h_s, engine=eng)
    exps = [rng.getrandbits(fr.exp_bits) for _ in range(cases.N_ROWS)]
    fresh = homomorphic.sparse_matmul(cts, (CROW, COL, VAL), n=n, bias=BIAS, engine=eng, randomizer=_Given(fr, exps))
    assert fresh == [v * pow(h_s, a, n2) % n2 for v, a in zip(want_bias, exps)]
    drawn = homomorphic.sparse_matmul(cts, (CROW, COL, VAL), n=n, bias=BIAS, engine=eng, randomizer=fr)
    assert all(u != v for u, v in zip(drawn, want_bias))


def test_encrypted_sparse_product_round_trip(eng):
    """60 small signed values under a 512-bit key and a sparse signed 12 x 60 matrix with 8-bit weights: encrypt,
    sparse_matmul with a bias, threshold decryption by three parties, against numpy's A m + b; once more with two values
    per plaintext in signed slots."""
    from protocols.distributed_keygen_amd import homomorphic, packing, slots, synthetic
    from protocols.distributed_keygen_amd.shared_key import GpuPaillierSharedKey, PlainCiphertext, ShareView

    key = synthetic.make_key(512, 3, 1)
    n = key.n
    rng = random.Random(53)
    nprng = np.random.default_rng(53)
    count, rows, per_row = 60, 12, 7
    g = nprng.integers(-1000, 1000, size=count)
    h = nprng.integers(-1000, 1000, size=count)
    col = np.concatenate([nprng.choice(count, size=per_row, replace=False) for _ in range(rows)])
    val = nprng.integers(-255, 256, size=rows * per_row)
    crow = np.arange(rows + 1) * per_row
    bias = nprng.integers(-500, 500, size=rows)
    dense = np.zeros((rows, count), dtype=np.int64)
    np.add.at(dense, (np.repeat(np.arange(rows), per_row), col), val)
    keys = {i: GpuPaillierSharedKey(n, key.t, i, ShareView({i: key.shares[i]}, key.degree, key.n_fac), key.theta, engine=eng)
            for i in (1, 2, 3)}

    def decrypt(values):
        parts = {i: k.partial_decrypt_batch([PlainCiphertext(c, n) for c in values]) for i, k in keys.items()}
        return keys[1].decrypt_batch([{i: parts[i][e] for i in keys} for e in range(len(values))])

    cts = eng.encrypt_batch([int(v) % n for v in g], [rng.randrange(1, n) for _ in g], n)
    out = homomorphic.sparse_matmul(cts, (crow, col, val), n=n, bias=[int(b) for b in bias], engine=eng)
    plain = decrypt(out)
    assert [m - n if m > n // 2 else m for m in plain] == (dense @ g + bias).tolist()
    # (g_i, h_i) in slots 0 and 1 of plaintext i; per_row terms of 11-bit values under 8-bit weights cannot leave the slot
    # (no bias here: a bias would be added to slot 0 alone)
    b = slots.slot_bits_for(11, 8, per_row)
    k = packing.slots_per_ciphertext(n, b)
    vals = np.zeros((count, k), dtype=np.int64)
    vals[:, 0], vals[:, 1] = g, h
    packed = slots.encode(vals.reshape(-1), n, b, engine=eng)
    assert len(packed) == count
    cts2 = eng.encrypt_batch(packed, [rng.randrange(1, n) for _ in packed], n)
    out2 = homomorphic.sparse_matmul(cts2, (crow, col, val), n=n, engine=eng)
    dec = np.array(slots.decode(decrypt(out2), n, b, rows * k, engine=eng), dtype=np.int64).reshape(rows, k)
    assert dec[:, 0].tolist() == (dense @ g).tolist() and dec[:, 1].tolist() == (dense @ h).tolist() and not dec[:, 2:].any()
