"""Encrypted histograms, host side (no GPU): hist_plan.py against plain ``%`` products over the Python-int backend of
tests/hist_engine.py, the refusals of the public entry points, and the shape / workspace / run entry points of the C ABI,
which validate before they touch the runtime."""

from __future__ import annotations

import ctypes
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from hist_engine import HistBackend, HistEngine
from protocols.distributed_keygen_amd import hist_plan as hp
from protocols.distributed_keygen_amd import homomorphic as H

N = 1000003 * 999983
N2 = N * N


def oracle(cts, bins, n_bins, n=N):
    n2 = n * n
    out = []
    for row in bins:
        hist = [1] * n_bins
        for c, b in zip(cts, row):
            if b >= 0:
                hist[b] = hist[b] * c % n2
        out.append(hist)
    return out


def segment_case(chunk, rng):
    """One feature whose bins have 0, 1, C - 1, C, C + 1 samples (in a shuffled order), and one with every sample in one bin."""
    lens = [0, 1, max(0, chunk - 1), chunk, chunk + 1]
    row = [b for b, k in enumerate(lens) for _ in range(k)]
    rng.shuffle(row)
    n = len(row)
    return [rng.randrange(N2) for _ in range(n)], [row, [2] * n], len(lens)


@pytest.mark.parametrize("chunk", [1, 2, 3, 64])
def test_segments_around_the_chunk_against_plain_products(chunk):
    rng = random.Random(chunk)
    cts, bins, n_bins = segment_case(chunk, rng)
    eng = HistEngine()
    got = eng.ciphertext_histogram_batch(cts, bins, n_bins, N, chunk=chunk)
    assert got == oracle(cts, bins, n_bins)
    runs = eng.backend.runs
    assert runs[0][2] == chunk and all(r[2] == max(2, chunk) for r in runs[1:])        # a level has to shrink
    assert [r[3] for r in runs] == [True] * (len(runs) - 1) + [False]                   # only the last level leaves pair form
    # exactly one product per term at the first level, and padding of at most C - 1 per segment and level
    assert runs[0][4] == 2 * len(cts)
    for n_rows, pieces, c, _, terms in runs:
        assert pieces * c - terms <= 2 * n_bins * max(1, c - 1) + 2 * n_bins            # (an empty segment is one whole piece of ones)
    assert eng.backend.converts == [(0, len(cts))]


def test_several_combine_levels_chunk_2_over_a_bin_of_77():
    rng = random.Random(7)
    cts = [rng.randrange(N2) for _ in range(77)]
    eng = HistEngine()
    assert eng.ciphertext_histogram_batch(cts, [[0] * 77], 2, N, chunk=2) == oracle(cts, [[0] * 77], 2)
    # 77 -> 39 -> 20 -> 10 -> 5 -> 3 -> 2 -> 1 pieces of bin 0; the empty bin 1 is one piece of ones, carried from level to level
    assert [(r[1], r[4]) for r in eng.backend.runs] == [(40, 77), (21, 40), (11, 21), (6, 11), (4, 6), (3, 4), (2, 3)]
    assert [r[0] for r in eng.backend.runs] == [77, 40, 21, 11, 6, 4, 3]                # a level's pieces are the next level's rows


def test_the_librarys_chunk_is_asked_for_every_level():
    seen = []

    def chunk_fn(n_rows, n_segments, total_terms):
        seen.append((n_rows, n_segments, total_terms))
        return 5

    rng = random.Random(3)
    cts = [rng.randrange(N2) for _ in range(60)]
    bins = [[rng.randrange(-1, 3) for _ in cts] for _ in range(2)]
    eng = HistEngine(chunk_fn=chunk_fn)
    assert eng.ciphertext_histogram_batch(cts, bins, 3, N) == oracle(cts, bins, 3)
    terms = sum(b >= 0 for row in bins for b in row)
    assert seen[0] == (60, 6, terms) and len(seen) == len(eng.backend.runs) >= 2
    assert all(s[1] == 6 for s in seen) and seen[1][0] == seen[1][2] == eng.backend.runs[0][1]


def library_chunk(bits):
    """The library's own chunk rule (mx_histogram_nsquare_shape needs no GPU) as the double's chunk function."""
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()

    def chunk_fn(n_rows, n_segments, total_terms):
        k, l, c = (ctypes.c_int() for _ in range(3))
        assert lib.mx_histogram_nsquare_shape(bits, n_rows, n_segments, total_terms, 0, 0, k, l, c, ctypes.c_int64()) == 0
        return c.value
    return chunk_fn


@pytest.mark.parametrize("n,feats,n_bins", [(400, 2, 300), (3000, 3, 40), (50000, 4, 7)])
def test_padding_under_the_librarys_own_chunk_rule(n, feats, n_bins):
    """Many short segments, middling ones and a few long ones, planned with the chunk the library picks: at every level
    at most C - 1 padding terms per segment with terms and one whole piece of C per segment without, and C never above
    the mean segment length rounded up — so the index array stays within twice the terms plus one word per segment."""
    rng = np.random.default_rng(n)
    bins = rng.integers(-1, n_bins, size=(feats, n))
    bins[0, bins[0] == 1] = -1                                                        # an empty segment
    cts = [int(v) for v in rng.integers(2, 1 << 62, size=n)]
    eng = HistEngine(chunk_fn=library_chunk(2048))
    got = eng.histogram_nsquare_t(cts, bins, n_bins, N)
    lens = np.array([[int((bins[f] == b).sum()) for b in range(n_bins)] for f in range(feats)]).reshape(-1)
    acc = np.ones(feats * n_bins, dtype=object)
    for f in range(feats):
        for i in np.flatnonzero(bins[f] >= 0):
            acc[f * n_bins + bins[f, i]] = acc[f * n_bins + bins[f, i]] * cts[i] % N2
    assert got == list(acc)
    segs = feats * n_bins
    for level, (n_rows, pieces, c, _, terms) in enumerate(eng.backend.runs):
        assert c <= max(2 if level else 1, -(-terms // segs)), (level, c, terms)
        assert pieces == int(np.maximum(1, -(-lens // c)).sum())
        empty = int((lens == 0).sum())
        assert pieces * c - terms <= (segs - empty) * (c - 1) + empty * c
        assert pieces * c <= 2 * terms + segs
        lens = np.maximum(1, -(-lens // c))                                           # the pieces are the next level's terms
    assert eng.backend.runs[0][4] == int((bins >= 0).sum())                           # exactly one product per kept term


def test_sample_stages_and_feature_slices_under_a_tiny_budget():
    rng = random.Random(11)
    n, n_bins = 77, 4
    cts = [rng.randrange(N2) for _ in range(n)]
    # (rows of 72 bytes.)  2880 bytes: 31 samples with the index words of 5 features beside them; with 20 features the
    # index array no longer fits half the budget beside 20 rows — 18 features per slice, 20 samples per stage; 16 bytes
    # hold no row at all: one sample per stage, two features per slice
    for feats, budget, stages, slices in ((5, 2880, 3, 1), (20, 2880, 4, 2), (5, 16, 77, 3)):
        bins = [[rng.randrange(-1, n_bins) for _ in range(n)] for _ in range(feats)]
        want = oracle(cts, bins, n_bins)
        s_stage, f_slice = hp.staging(n, feats, 72, budget)
        assert (-(-n // s_stage), -(-feats // f_slice)) == (stages, slices), (budget, s_stage, f_slice)
        if 72 + 4 <= budget:
            assert s_stage * (72 + 4 * f_slice) <= budget                               # rows and index arrays fit
        eng = HistEngine()
        assert eng.ciphertext_histogram_batch(cts, bins, n_bins, N, table_budget_bytes=budget) == want, budget
        assert eng.backend.converts == [(lo, min(n, lo + s_stage)) for lo in range(0, n, s_stage)]      # once per sample, whatever the slices
        final = [r for r in eng.backend.runs if not r[3]]
        assert len(final) == slices and sum(r[1] for r in final) == feats * n_bins
    # the default budget: one stage, one slice at any plausible size
    assert hp.staging(10 ** 5, 10, 576, hp.TABLE_BUDGET_BYTES) == (10 ** 5, 10)
    s_stage, f_slice = hp.staging(10 ** 6, 10, 576, hp.TABLE_BUDGET_BYTES)
    assert f_slice == 10 and s_stage == (256 << 20) // 616 and -(-10 ** 6 // s_stage) == 3


def test_skipped_samples_and_the_empty_shapes():
    rng = random.Random(13)
    cts = [rng.randrange(N2) for _ in range(9)] + [0, 1, N2 - 1, 5 * N, N2 + 7]
    n = len(cts)
    bins = [[-1] * n, [rng.choice((-1, 0, 3)) for _ in range(n)], list(range(4)) + [-1] * (n - 4)]
    eng = HistEngine()
    got = eng.ciphertext_histogram_batch(cts, bins, 4, N)
    assert got == oracle(cts, bins, 4) and got[0] == [1, 1, 1, 1]
    for form in (np.array(bins), np.array(bins, dtype=np.int8), torch.tensor(bins), torch.tensor(bins, dtype=torch.int32)):
        assert HistEngine().ciphertext_histogram_batch(cts, form, 4, N) == got
    assert HistEngine().ciphertext_histogram_batch(cts, [], 4, N) == []                                # F = 0
    assert HistEngine().ciphertext_histogram_batch(cts, np.zeros((0, n), dtype=np.int64), 4, N) == []
    e0 = HistEngine()
    assert e0.ciphertext_histogram_batch([], [[], []], 3, N) == [[1, 1, 1], [1, 1, 1]]                 # n = 0: all ones
    assert e0.backend.converts == [] and e0.backend.runs == []
    assert H.histogram([], [[], []], 3, n=N, engine=HistEngine()) == [[1, 1, 1], [1, 1, 1]]


def test_refusals_come_before_any_launch():
    cts = [3, 5, 7]
    for bins, n_bins in (([[0, 1, 2]], 2), ([[0, -2, 1]], 3),                      # a bin >= n_bins, a bin < -1
                         ([0, 1, 2], 3), ([[[0, 1, 2]]], 3),                       # not two-dimensional
                         ([[0, 1]], 3), ([[0, 1, 2, 0]], 3), ([[0, 1, 2], [0, 1]], 3),     # another row length, ragged rows
                         ([[0, 1, 2]], 0), ([[0, 1, 2]], -1),                      # n_bins < 1
                         ([[0.0, 1.0, 2.0]], 3), (np.zeros((1, 3), dtype=np.float32), 3), (torch.zeros((1, 3)), 3),
                         (torch.zeros((1, 3), dtype=torch.bool), 3)):              # not an integer dtype
        eng = HistEngine()
        with pytest.raises(ValueError):
            eng.ciphertext_histogram_batch(cts, bins, n_bins, N)
        assert eng.backend is None
        eng = HistEngine()
        with pytest.raises(ValueError):
            H.histogram(cts, bins, n_bins, n=N, engine=eng)
        assert eng.calls == []
    for bad_n in (2, 1, 10):
        with pytest.raises(ValueError):
            H.histogram(cts, [[0, 1, 2]], 3, n=bad_n, engine=HistEngine())
    with pytest.raises(ValueError):
        H.histogram(cts, [[0, 1, 2]], 3, engine=HistEngine())                      # plain ints need n


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


def test_get_value_is_called_once_per_object_and_the_randomiser_covers_every_bin():
    rng = random.Random(5)
    a, b, c = (Ct(rng.randrange(1, N2)) for _ in range(3))
    eng = HistEngine()

    class Rz:
        def spec(self, n, count):
            return ("spec", n, count)

    bins = [[0, 1, 0, 1, 2], [4, 4, -1, 4, 4]]
    got = H.histogram([a, b, a, c, 11], bins, 5, engine=eng, randomizer=Rz())
    assert (a.reads, b.reads, c.reads) == (1, 1, 1)
    assert got == oracle([a.v, b.v, a.v, c.v, 11], bins, 5)
    assert eng.calls[-1][1] == ("spec", N, 10)                                     # F * n_bins results
    H.histogram([a, b], [[0, 0]], 1, engine=eng)
    assert eng.calls[-1][1] is None


def test_piece_index_is_what_the_kernel_reads():
    counts = torch.tensor([0, 1, 5, 3])
    src = torch.arange(9) + 100
    index, pieces = hp.piece_index(counts, src, 3, 999)
    assert pieces.tolist() == [1, 1, 2, 1] and index.dtype == torch.int32
    assert index.tolist() == [[999, 999, 999], [100, 999, 999], [101, 102, 103], [104, 105, 999], [106, 107, 108]]
    counts, src = hp.stage_terms(torch.tensor([[1, -1, 0, 1], [0, 0, -1, -1]]), 2)
    assert counts.tolist() == [1, 2, 2, 0] and src.tolist() == [2, 0, 3, 0, 1]     # samples ascending inside a segment


def test_abi_shape_and_workspace_need_no_gpu():
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    assert lib.mx_version() == 404
    k, l, c = (ctypes.c_int() for _ in range(3))
    rb = ctypes.c_int64()
    for bits in (130, 200, 400, 900, 1531, 2048, 3000, 4000, 6000, 8000):
        assert lib.mx_histogram_nsquare_shape(bits, 1000, 320, 10 ** 6, 0, 0, k, l, c, rb) == 0, bits
        assert l.value == 9 and k.value in (1, 2, 4, 8, 16, 32)
        assert k.value * l.value * 29 >= bits + 4                                  # a digit modulo N per half: the pair covers N^2
        assert rb.value == 2 * k.value * l.value * 4 and rb.value * 8 >= 2 * bits
        assert 1 <= c.value <= 4096
        assert lib.mx_histogram_nsquare_workspace_bytes(bits, 1000, 0) >= 1001 * rb.value
        assert lib.mx_histogram_nsquare_workspace_bytes(bits, 0, 9) >= rb.value    # the one row alone
    assert lib.mx_histogram_nsquare_shape(2048, 10 ** 5, 320, 10 ** 6, 0, 0, k, l, c, rb) == 0
    assert (k.value, rb.value) == (8, 576) and 16 <= c.value <= 64                 # 10^6 terms: pieces that fill the device
    assert lib.mx_histogram_nsquare_shape(2048, 100, 50, 100, 0, 0, k, l, c, rb) == 0 and c.value == 2      # short segments: their mean
    assert lib.mx_histogram_nsquare_shape(2048, 100, 2, 100, 0, 0, k, l, c, rb) == 0 and c.value == 16
    # many short segments and many terms: the fill-the-device term alone would be 163 — never above the mean segment, 4
    assert lib.mx_histogram_nsquare_shape(2048, 4 * 10 ** 5, 10 ** 6, 4 * 10 ** 6, 0, 0, k, l, c, rb) == 0 and c.value == 4
    assert lib.mx_histogram_nsquare_shape(2048, 10 ** 5, 10 ** 5, 10 ** 6, 0, 0, k, l, c, rb) == 0 and c.value == 10
    assert lib.mx_histogram_nsquare_shape(2048, 10 ** 6, 10 ** 7, 10 ** 6, 0, 0, k, l, c, rb) == 0 and c.value == 1      # mostly empty
    assert lib.mx_histogram_nsquare_shape(128, 10 ** 7, 4, 4 * 10 ** 8, 0, 0, k, l, c, rb) == 0 and c.value == 2035       # few long ones: fill the device
    assert lib.mx_histogram_nsquare_shape(2048, 10 ** 9, 4, 4 * 10 ** 9, 0, 0, k, l, c, rb) == 0 and c.value == 4096
    assert lib.mx_histogram_nsquare_shape(2048, 0, 0, 0, 0, 0, k, l, c, rb) == 0 and c.value >= 1
    assert lib.mx_histogram_nsquare_shape(2048, 100, 2, 100, 9, 1000, k, l, c, rb) == 0 and c.value == 1000  # an explicit chunk
    for bad in ((2048, -1, 2, 100, 0, 0), (2048, 1, -2, 100, 0, 0), (2048, 1, 2, -1, 0, 0), (2048, 1, 2, 100, 18, 0),
                (2048, 1, 2, 100, 0, -1), (2048, 1, 2, 100, 0, 65537)):
        assert lib.mx_histogram_nsquare_shape(*bad, k, l, c, rb) == -1, bad
    assert lib.mx_histogram_nsquare_shape(2048, 1, 2, 100, 0, 0, None, l, c, rb) == -1
    assert lib.mx_histogram_nsquare_shape(2048, 1, 2, 100, 0, 0, k, l, c, None) == -1
    assert lib.mx_histogram_nsquare_shape(20000, 1, 2, 100, 0, 0, k, l, c, rb) == -2        # no narrow instance
    assert lib.mx_histogram_nsquare_workspace_bytes(2048, -1, 0) == -1
    assert lib.mx_histogram_nsquare_workspace_bytes(2048, 1 << 31, 0) == -1
    assert lib.mx_histogram_nsquare_workspace_bytes(2048, 5, 18) == -1
    assert lib.mx_histogram_nsquare_workspace_bytes(20000, 5, 0) == -2
    lanes, lpl = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    count = lib.mx_histogram_nsquare_instances(lanes, lpl, 8)
    assert [(lanes[i], lpl[i]) for i in range(count)] == [(kk, 9) for kk in (1, 2, 4, 8, 16, 32)]
    assert lib.mx_histogram_nsquare_instances(None, None, 4) == -1


def test_abi_refuses_bad_launches_before_anything_is_enqueued():
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    # a descriptor that names memory which is never read, because every call below is refused first
    buf = (ctypes.c_uint32 * 64)()
    ptr = ctypes.addressof(buf)
    plan = _lib.NsquarePlan(d_plan=ptr, plan_bytes=256, limbs_n=64, n_bits=2048, geometries=1)
    no_block = _lib.NsquarePlan(d_plan=None, limbs_n=64, n_bits=2048, geometries=1)
    no_narrow = _lib.NsquarePlan(d_plan=ptr, limbs_n=64, n_bits=2048, geometries=0)
    too_wide = _lib.NsquarePlan(d_plan=ptr, limbs_n=625, n_bits=20000, geometries=1)

    ok = dict(plan=plan, inputs=ptr, n=5, limbs2=128, rows=ptr, rows_bytes=1 << 40, lpl=0)

    def convert(**kw):
        a = dict(ok, **kw)
        return lib.mx_histogram_nsquare_convert(a["plan"], a["inputs"], a["n"], a["limbs2"], a["rows"], a["rows_bytes"], a["lpl"], None)

    for kw in (dict(plan=None), dict(plan=no_block), dict(inputs=None), dict(rows=None), dict(n=0), dict(n=-3), dict(n=1 << 31),
               dict(limbs2=0), dict(limbs2=127), dict(lpl=18)):
        assert convert(**kw) == -1, kw
    assert convert(plan=no_narrow) == -2 and convert(plan=too_wide, limbs2=1250) == -2
    assert convert(rows_bytes=6 * 576 - 1) == -4 and convert(rows_bytes=0) == -4

    ok = dict(plan=plan, rows=ptr, n_rows=5, index=ptr, pieces=3, chunk=4, out=ptr, pair=0, limbs2=128, out_bytes=1 << 40, lpl=0)

    def run(**kw):
        a = dict(ok, **kw)
        return lib.mx_histogram_nsquare_run(a["plan"], a["rows"], a["n_rows"], a["index"], a["pieces"], a["chunk"], a["out"], a["pair"],
                                            a["limbs2"], a["out_bytes"], a["lpl"], None)

    for kw in (dict(plan=None), dict(plan=no_block), dict(rows=None), dict(index=None), dict(out=None), dict(n_rows=-1),
               dict(n_rows=1 << 31), dict(pieces=0), dict(pieces=-1), dict(chunk=0), dict(chunk=-1), dict(chunk=65537),
               dict(limbs2=0), dict(limbs2=127), dict(lpl=18)):
        assert run(**kw) == -1, kw
    assert run(plan=no_narrow) == -2 and run(plan=too_wide, limbs2=1250) == -2
    assert run(pieces=1 << 40) == -2                                               # beyond one grid
    assert run(out_bytes=3 * 128 * 4 - 1) == -4                                    # canonical rows
    assert run(pair=1, out_bytes=4 * 576 - 1) == -4                                # pair-form rows and the one row


def test_no_histogram_kernel_has_a_private_segment():
    """private_segment_fixed_size 0 and no spilled register for every histogram instance of the BUILT library, read the
    way tests/test_instances.py reads it for the modexp kernels."""
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root / "tools"))
    import scratch_report

    from protocols.distributed_keygen_amd import _lib

    rows = scratch_report.kernels_of_library(_lib.LIB_PATH)
    names = scratch_report.demangle([r[0] for r in rows])
    hist = [r for r in rows if "hist_n2" in names[r[0]]]
    for kk in (1, 2, 4, 8, 16, 32):
        for kernel in ("hist_n2_convert_kernel", "hist_n2_kernel"):
            assert any(f"mx::{kernel}<{kk}, 9, 29>" in names[r[0]] for r in hist), (kernel, kk)
    assert len(hist) == 12
    assert not [(names[r[0]], r[1], r[2]) for r in hist if r[1] or r[2]]
