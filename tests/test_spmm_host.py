"""Encrypted sparse matrix products, host side (no GPU): spmm_plan.py against CPython's ``pow`` over the Python-int
backend of tests/spmm_engine.py, the refusals of the public entry points, the window rule and the entry points of the C
ABI, which validate before they touch the runtime, and the metadata of the two new kernels in the built library."""

from __future__ import annotations

import ctypes
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import spmm_cases as cases
from spmm_engine import SpmmEngine, library_shape
from protocols.distributed_keygen_amd import homomorphic as H
from protocols.distributed_keygen_amd import spmm_plan as sp

N = 1000003 * 999983
N2 = N * N
CROW, COL, VAL, BIAS = cases.parity_matrix()
CTS = cases.parity_inputs(N)
WANT = cases.expected(CTS, CROW, COL, VAL, N)
WANT_BIAS = cases.expected(CTS, CROW, COL, VAL, N, BIAS)


def library_chunk(bits):
    """The library's own chunk rule (mx_histogram_nsquare_shape needs no GPU) as the double's chunk function."""
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()

    def chunk_fn(n_rows, n_segments, total_terms):
        k, l, c = (ctypes.c_int() for _ in range(3))
        assert lib.mx_histogram_nsquare_shape(bits, n_rows, n_segments, total_terms, 0, 0, k, l, c, ctypes.c_int64()) == 0
        return c.value
    return chunk_fn


def test_plan_against_the_double_on_the_parity_case():
    eng = SpmmEngine()
    assert eng.ciphertext_spmm_batch(CTS, CROW, COL, VAL, N) == WANT
    be = eng.backend
    (asked, (w, positions)), = be.shapes
    plus, minus = be.pools[0]
    # the tables: the columns under a positive weight, then those under a negative one; the rule's I counts every input
    assert plus == sorted({c for c, v in zip(COL, VAL) if v > 0}) and minus == sorted({c for c, v in zip(COL, VAL) if v < 0})
    assert asked == (cases.N_IN + len(minus), cases.N_ROWS, sum(v != 0 for v in VAL), 63, 0)
    assert positions == -(-63 // w) and be.horners == [(cases.N_ROWS, positions, w, False)]
    assert be.table_calls == [(0, len(plus) + len(minus), w)]                  # every input converted once
    # exactly one product per non-zero digit at the first level, and one row per (row, position) segment at the last
    digits = sum(1 for v in VAL for p in range(positions) if (abs(v) >> (p * w)) & ((1 << w) - 1))
    assert be.runs[0][4] == digits and be.runs[-1][1] == cases.N_ROWS * positions
    assert all(r[3] for r in be.runs)                                          # pair form throughout: Horner stores
    eng = SpmmEngine()
    assert eng.ciphertext_spmm_batch(CTS, CROW, COL, VAL, N, bias=BIAS) == WANT_BIAS
    assert eng.backend.horners[0][3] and eng.backend.converts == [(0, cases.N_ROWS)]      # the bias rows: one conversion
    # numpy and torch forms of the triple
    for conv in (np.array, torch.tensor):
        assert SpmmEngine().ciphertext_spmm_batch(CTS, conv(CROW), conv(COL), conv(VAL), N, bias=BIAS) == WANT_BIAS
    assert H.sparse_matmul(CTS, (CROW, COL, VAL), n=N, bias=BIAS, engine=SpmmEngine()) == WANT_BIAS


def test_digit_terms_are_what_the_kernels_read():
    crow, col, val = torch.tensor([0, 2, 2, 4]), torch.tensor([3, 1, 1, 3]), torch.tensor([5, -6, 0, 16])
    key, table, digit, plus, minus = sp.digit_terms(crow, col, val, 4, 2, 3)
    assert plus.tolist() == [3] and minus.tolist() == [1]
    # 5 = (1, 1, 0), 6 = (2, 1, 0), 16 = (0, 0, 1) in base 4, low digit first; the stored 0 has no digit
    assert key.tolist() == [0, 1, 0, 1, 8] and table.tolist() == [0, 0, 1, 1, 0] and digit.tolist() == [1, 1, 2, 1, 1]
    counts, src = sp.stage_terms(key, table * 3 + digit - 1, 9)
    assert counts.tolist() == [2, 2, 0, 0, 0, 0, 0, 0, 1] and src.tolist() == [0, 4, 0, 3, 0]


@pytest.mark.parametrize("window", range(1, 9))
def test_forced_windows(window):
    eng = SpmmEngine()
    assert eng.ciphertext_spmm_batch(CTS, CROW, COL, VAL, N, bias=BIAS, window=window) == WANT_BIAS
    assert eng.backend.horners == [(cases.N_ROWS, -(-63 // window), window, True)]


@pytest.mark.parametrize("chunk", [1, 2, 0, 1000])
def test_forced_chunks(chunk):
    eng = SpmmEngine()
    assert eng.ciphertext_spmm_batch(CTS, CROW, COL, VAL, N, chunk=chunk) == WANT
    runs = eng.backend.runs
    if chunk:
        assert runs[0][2] == chunk and all(r[2] == max(2, chunk) for r in runs[1:])
    assert (len(runs) > 1) == (chunk in (1, 2, 0))                             # (the double's own chunk is 4)


def test_a_small_budget_forces_stages():
    for window, budget in ((2, 1000), (4, 1), (0, 5000)):
        eng = SpmmEngine()
        got = eng.ciphertext_spmm_batch(CTS, CROW, COL, VAL, N, bias=BIAS, window=window, table_budget_bytes=budget)
        assert got == WANT_BIAS
        be = eng.backend
        plus, minus = be.pools[0]
        assert len(be.pools) == 1 and len(be.table_calls) >= 2
        # the stages cut the tables without a gap or an overlap: every input is converted once
        assert [c[0] for c in be.table_calls] == [0] + [c[1] for c in be.table_calls[:-1]]
        assert be.table_calls[-1][1] == len(plus) + len(minus)
        w = be.table_calls[0][2]
        per = ((1 << w) - 1) * 72
        for lo, hi, _ in be.table_calls[:-1]:
            assert (hi - lo) * per <= max(budget, per)
    assert sp.staging(2 * 10 ** 5, 4 * 10 ** 6, 4, 576, sp.TABLE_BUDGET_BYTES) == (256 << 20) // (15 * 576 + 4 * 20)


def test_the_index_arrays_stay_within_twice_the_terms():
    rng = np.random.default_rng(5)
    n_in, rows, per_col = 3000, 50, 4
    col = np.repeat(np.arange(n_in), per_col)
    row = rng.integers(0, rows, size=col.size)
    val = rng.integers(-(1 << 15), 1 << 15, size=col.size)
    order = np.argsort(row, kind="stable")
    col, val = col[order], val[order]
    crow = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=rows))])
    draw = random.Random(5)
    cts = [cases.unit(draw, N) for _ in range(n_in)]
    eng = SpmmEngine(chunk_fn=library_chunk(2048))
    got = eng.spmm_nsquare_t(cts, crow, col, val, N)
    assert got == cases.expected(cts, crow.tolist(), col.tolist(), val.tolist(), N)
    be = eng.backend
    w, positions = be.shapes[0][1]
    segs = rows * positions
    terms = int(sum(1 for v in val.tolist() for p in range(positions) if (abs(v) >> (p * w)) & ((1 << w) - 1)))
    assert be.runs[0][4] == terms
    for n_rows, pieces, c, _, live in be.runs:
        assert pieces * c <= 2 * live + segs, (pieces, c, live)


def test_window_rule_needs_no_gpu():
    def model(i, r, nnz, b):
        cost = lambda w: i * ((1 << w) - 2) + nnz * -(-b // w) + r * (-(-b // w) - 1) * (w + 1)
        return min(range(1, 7), key=lambda w: (cost(w), w))

    assert library_shape(2048, 10 ** 5, 1024, 10 ** 6, 1) == (0, 1, 1)         # weights in {-1, 0, 1}
    assert library_shape(2048, 7, 3, 100, 0) == (0, 1, 1)                      # no weight at all
    seen = set()
    for i, r, nnz, b in ((10 ** 5, 1024, 10 ** 6, 16), (2 * 10 ** 5, 1024, 10 ** 6, 16), (40, 9, 80, 63), (1, 1, 1, 63),
                         (10 ** 7, 10, 10 ** 7, 8), (100, 10 ** 6, 10 ** 7, 32), (10, 10, 10 ** 9, 63), (1000, 1, 1000, 2),
                         (3, 2, 12, 6), (50, 50, 200, 12)):
        w = model(i, r, nnz, b)
        assert library_shape(2048, i, r, nnz, b) == (0, w, -(-b // w)), (i, r, nnz, b)
        seen.add(w)
    assert len(seen) >= 4
    for window in range(1, 9):
        assert library_shape(2048, 40, 9, 80, 63, window) == (0, window, -(-63 // window))
    for bits in (130, 1531, 2048, 4000, 8000):
        assert library_shape(bits, 40, 9, 80, 16)[0] == 0


def test_abi_refusals_need_no_gpu():
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    assert lib.mx_version() == 404
    k, l, w, d = (ctypes.c_int() for _ in range(4))
    rb = ctypes.c_int64()
    assert lib.mx_spmm_nsquare_shape(2048, 40, 9, 80, 16, 9, 0, k, l, w, d, rb) == 0
    assert (k.value, l.value, rb.value) == (8, 9, 576)
    for bad in ((2048, -1, 9, 80, 16, 0, 0), (2048, 40, -9, 80, 16, 0, 0), (2048, 40, 9, -1, 16, 0, 0), (2048, 40, 9, 80, -1, 0, 0),
                (2048, 40, 9, 80, 64, 0, 0), (2048, 40, 9, 80, 16, 18, 0), (2048, 40, 9, 80, 16, 0, -1), (2048, 40, 9, 80, 16, 0, 9)):
        assert lib.mx_spmm_nsquare_shape(*bad, k, l, w, d, rb) == -1, bad
    assert lib.mx_spmm_nsquare_shape(2048, 40, 9, 80, 16, 0, 0, None, l, w, d, rb) == -1
    assert lib.mx_spmm_nsquare_shape(2048, 40, 9, 80, 16, 0, 0, k, l, w, d, None) == -1
    assert lib.mx_spmm_nsquare_shape(20000, 40, 9, 80, 16, 0, 0, k, l, w, d, rb) == -2           # no narrow instance
    # the table of n inputs is a row set of n (2^w - 1) rows
    assert lib.mx_spmm_nsquare_workspace_bytes(2048, 10, 4, 0) == lib.mx_histogram_nsquare_workspace_bytes(2048, 150, 0) >= 151 * 576
    assert lib.mx_spmm_nsquare_workspace_bytes(2048, 10, 1, 9) == lib.mx_histogram_nsquare_workspace_bytes(2048, 10, 0)
    for bad in ((2048, -1, 4, 0), (2048, 10, 0, 0), (2048, 10, 9, 0), (2048, 10, 4, 18), (2048, 1 << 28, 8, 0), (2048, 1 << 31, 1, 0)):
        assert lib.mx_spmm_nsquare_workspace_bytes(*bad) == -1, bad
    assert lib.mx_spmm_nsquare_workspace_bytes(20000, 10, 4, 0) == -2
    lanes, lpl = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    count = lib.mx_spmm_nsquare_instances(lanes, lpl, 8)
    assert [(lanes[i], lpl[i]) for i in range(count)] == [(kk, 9) for kk in (1, 2, 4, 8, 16, 32)]
    assert lib.mx_spmm_nsquare_instances(None, None, 4) == -1

    # launches: a descriptor that names memory which is never read, because every call below is refused first
    buf = (ctypes.c_uint32 * 64)()
    ptr = ctypes.addressof(buf)
    plan = _lib.NsquarePlan(d_plan=ptr, plan_bytes=256, limbs_n=64, n_bits=2048, geometries=1)
    no_block = _lib.NsquarePlan(d_plan=None, limbs_n=64, n_bits=2048, geometries=1)
    no_narrow = _lib.NsquarePlan(d_plan=ptr, limbs_n=64, n_bits=2048, geometries=0)
    too_wide = _lib.NsquarePlan(d_plan=ptr, limbs_n=625, n_bits=20000, geometries=1)

    ok = dict(plan=plan, inputs=ptr, n=5, limbs2=128, window=4, rows=ptr, rows_bytes=1 << 40, lpl=0)

    def tables(**kw):
        a = dict(ok, **kw)
        return lib.mx_spmm_nsquare_tables(a["plan"], a["inputs"], a["n"], a["limbs2"], a["window"], a["rows"], a["rows_bytes"],
                                          a["lpl"], None)

    for kw in (dict(plan=None), dict(plan=no_block), dict(inputs=None), dict(rows=None), dict(n=0), dict(n=-3), dict(n=1 << 31),
               dict(n=1 << 28), dict(limbs2=0), dict(limbs2=127), dict(lpl=18), dict(window=0), dict(window=9)):
        assert tables(**kw) == -1, kw
    assert tables(plan=no_narrow) == -2 and tables(plan=too_wide, limbs2=1250) == -2
    assert tables(rows_bytes=76 * 576 - 1) == -4 and tables(rows_bytes=0) == -4     # 5 * 15 rows and the one row

    ok = dict(plan=plan, rows=ptr, n_rows=5, positions=4, window=4, bias=None, out=ptr, limbs2=128, out_bytes=1 << 40, lpl=0)

    def horner(**kw):
        a = dict(ok, **kw)
        return lib.mx_spmm_nsquare_horner(a["plan"], a["rows"], a["n_rows"], a["positions"], a["window"], a["bias"], a["out"],
                                          a["limbs2"], a["out_bytes"], a["lpl"], None)

    for kw in (dict(plan=None), dict(plan=no_block), dict(rows=None), dict(out=None), dict(n_rows=0), dict(n_rows=-1),
               dict(n_rows=1 << 31), dict(n_rows=1 << 29), dict(positions=0), dict(positions=65), dict(window=0), dict(window=9),
               dict(limbs2=0), dict(limbs2=127), dict(lpl=18)):
        assert horner(**kw) == -1, kw
    assert horner(plan=no_narrow) == -2 and horner(plan=too_wide, limbs2=1250) == -2
    assert horner(out_bytes=5 * 128 * 4 - 1) == -4


class Ct:
    def __init__(self, v):
        self.v, self.reads = v, 0

        class _S:
            class public_key:
                n = N
        self.scheme = _S

    def get_value(self):
        self.reads += 1
        return self.v


def test_refusals_come_before_any_launch():
    cts = [3, 5, 7]
    good = ([0, 2, 3], [0, 2, 1], [4, -5, 6])
    bad = [
        ([0, 2, 1, 3], [0, 2, 1], [4, -5, 6]),                  # crow decreases
        ([1, 2, 3], [0, 2, 1], [4, -5, 6]),                     # crow[0] != 0
        ([0, 2, 2], [0, 2, 1], [4, -5, 6]),                     # crow[-1] != nnz
        ([0, 2, 4], [0, 2, 1], [4, -5, 6]),
        ([0, 2, 3], [0, 3, 1], [4, -5, 6]),                     # a column >= len(cts)
        ([0, 2, 3], [0, -1, 1], [4, -5, 6]),                    # a negative column
        ([0, 2, 3], [0, 2, 1], [4, -(1 << 63), 6]),             # -2^63
        ([0, 2, 3], [0, 2, 1], [4, 1 << 63, 6]),                # beyond 2^63 - 1
        ([0, 2, 3], [0, 2, 1], [4.0, -5.0, 6.0]),               # not integers
        ([0, 2, 3], [0, 2, 1], np.array([4, -5, 6], dtype=np.float32)),
        ([0, 2, 3], torch.tensor([0.0, 2.0, 1.0]), [4, -5, 6]),
        (torch.tensor([False, True]), [0], [1]),
        ([0, 2, 3], [0, 2, 1], [4, -5]),                        # col and val of different lengths
        ([[0, 2, 3]], [0, 2, 1], [4, -5, 6]),                   # not flat
        ([], [], []),                                           # no crow at all
    ]
    for crow, col, val in bad:
        eng = SpmmEngine()
        with pytest.raises(ValueError):
            eng.ciphertext_spmm_batch(cts, crow, col, val, N)
        assert eng.backend is None
        eng = SpmmEngine()
        with pytest.raises(ValueError):
            H.sparse_matmul(cts, (crow, col, val), n=N, engine=eng)
        assert eng.calls == [] and eng.backend is None
    for bias in ([1], [1, 2, 3], []):                           # a bias of another length
        eng = SpmmEngine()
        with pytest.raises(ValueError):
            eng.ciphertext_spmm_batch(cts, *good, N, bias=bias)
        assert eng.backend is None
        with pytest.raises(ValueError):
            H.sparse_matmul(cts, good, n=N, bias=bias, engine=eng)
        assert eng.calls == []
    # shape and dtype: before a ciphertext is read
    c = Ct(11)
    for matrix, bias in ((([0, 2, 3], [0, 2, 1], [4.0, -5.0, 6.0]), None), (([0, 2, 3], [0, 2, 1], [4, -5]), None), (good, [1]),
                         (torch.eye(3), None), (torch.eye(3).to_sparse_csr(), None), (torch.eye(4, dtype=torch.int64).to_sparse_csr(), None),
                         (torch.eye(3, dtype=torch.int64), None), ("abc", None), ((1, 2), None)):
        with pytest.raises(ValueError):
            H.sparse_matmul([c, c, c], matrix, bias=bias, engine=SpmmEngine())
        assert c.reads == 0
    for bad_n in (2, 1, 10):
        with pytest.raises(ValueError):
            H.sparse_matmul(cts, good, n=bad_n, engine=SpmmEngine())
    with pytest.raises(ValueError):
        H.sparse_matmul(cts, good, engine=SpmmEngine())                            # plain ints need n
    with pytest.raises(ValueError):
        SpmmEngine().ciphertext_spmm_batch(cts, *good, N, window=9)


def test_a_multiple_of_n_is_legal_under_positive_weights_only():
    cts = [5 * N, 7, 11]
    crow, col, val = [0, 2, 3], [0, 1, 2], [3, -2, 5]
    assert SpmmEngine().ciphertext_spmm_batch(cts, crow, col, val, N) == cases.expected(cts, crow, col, val, N)
    eng = SpmmEngine()
    with pytest.raises(ValueError):
        eng.ciphertext_spmm_batch(cts, crow, col, [-3, -2, 5], N)
    assert eng.backend.table_calls == [] and eng.backend.runs == []


def test_empty_shapes_sparse_tensors_and_the_randomiser():
    rng = random.Random(9)
    a, b = Ct(cases.unit(rng, N)), Ct(cases.unit(rng, N))
    eng = SpmmEngine()

    class Rz:
        def spec(self, n, count):
            return ("spec", n, count)

    dense = torch.tensor([[2, 0, -3], [0, 0, 0], [1, 1, 1], [0, 7, 0]])
    want = [pow(a.v, 2, N2) * pow(a.v, -3, N2) % N2, 1, a.v * b.v * a.v % N2, pow(b.v, 7, N2)]
    for matrix in (dense.to_sparse_csr(), dense.to_sparse(), dense.to(torch.int32).to_sparse_csr()):
        assert H.sparse_matmul([a, b, a], matrix, engine=eng, randomizer=Rz()) == want
        assert eng.calls[-1][1] == ("spec", N, 4)                                  # one exponent per row
    assert (a.reads, b.reads) == (3, 3)                                            # once per object and call
    H.sparse_matmul([a, b], ([0, 1], [1], [1]), engine=eng)
    assert eng.calls[-1][1] is None
    # no rows, no terms, no inputs
    assert SpmmEngine().ciphertext_spmm_batch([3, 5], [0], [], [], N) == []
    e0 = SpmmEngine()
    assert e0.ciphertext_spmm_batch([3, 5], [0, 0, 0], [], [], N, bias=[2, -1]) == [1 + 2 * N, 1 + (N - 1) * N]
    assert e0.ciphertext_spmm_batch([], [0, 0], [], [], N) == [1]
    assert e0.ciphertext_spmm_batch([3, 5], [0, 1, 2], [0, 1], [0, 0], N) == [1, 1]          # stored zeros only
    assert e0.backend.table_calls == [] and e0.backend.runs == [] and e0.backend.horners == []


def test_no_spmm_kernel_has_a_private_segment():
    """private_segment_fixed_size 0 and no spilled register for every instance of the two new kernels in the BUILT
    library, read the way tests/test_instances.py reads it for the modexp kernels."""
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root / "tools"))
    import scratch_report

    from protocols.distributed_keygen_amd import _lib

    rows = scratch_report.kernels_of_library(_lib.LIB_PATH)
    names = scratch_report.demangle([r[0] for r in rows])
    spmm = [r for r in rows if "spmm_n2" in names[r[0]]]
    for kk in (1, 2, 4, 8, 16, 32):
        for kernel in ("spmm_n2_table_kernel", "spmm_n2_horner_kernel"):
            assert any(f"mx::{kernel}<{kk}, 9, 29>" in names[r[0]] for r in spmm), (kernel, kk)
    assert len(spmm) == 12
    assert not [(names[r[0]], r[1], r[2]) for r in spmm if r[1] or r[2]]
