"""Encrypted prefix sums, host side (no GPU): scan_plan.py against plain ``%`` prefix products over the Python-int backend
of tests/scan_engine.py, the refusals of the public entry points, the run / store entry points of the C ABI, which
validate before they touch the runtime, and the scan kernels of the built library."""

from __future__ import annotations

import ctypes
import itertools
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from scan_engine import ScanEngine
from protocols.distributed_keygen_amd import homomorphic as H
from protocols.distributed_keygen_amd import scan_plan as sp

N = 1000003 * 999983
N2 = N * N
LENGTHS = [0, 1, 4, 5, 0, 9, 1]              # with the double's chunk of 4: pieces at, below and above the chunk; empty segments
FORMS = list(itertools.product((False, True), (False, True)))


def oracle(cts, lengths, exclusive=False, reverse=False, n=N):
    """A Python loop of acc = acc * c % n^2 per segment."""
    n2 = n * n
    out, lo = [], 0
    for k in lengths:
        seg = [c % n2 for c in cts[lo : lo + k]]
        lo += k
        if reverse:
            seg.reverse()
        res, acc = [], 1
        for c in seg:
            if exclusive:
                res.append(acc)
            acc = acc * c % n2
            if not exclusive:
                res.append(acc)
        if reverse:
            res.reverse()
        out += res
    return out


def case(seed=1, lengths=LENGTHS):
    rng = random.Random(seed)
    return [rng.randrange(1, N2) for _ in range(sum(lengths))]


def check_launches(be, count, staged=False):
    """What the recorded launches must show for any call: every input converted once, and the scans that are stored
    (the first level of every stage) store every output row exactly once."""
    assert sorted(be.input_converts) == sorted(set(be.input_converts))
    assert sum(hi - lo for lo, hi in be.input_converts) == count
    covered = sorted(i for lo, hi in be.input_converts for i in range(lo, hi))
    assert covered == list(range(count))
    assert sum(be.stores) == count and len(be.stores) == len(be.input_converts)
    if not staged:
        assert be.input_converts == [(0, count)] and be.picks == 0
    for n_rows, _, _, _, _, stored in be.scans:
        assert sorted(stored) == list(range(n_rows))                                   # every row of a level stored, once


@pytest.mark.parametrize("exclusive,reverse", FORMS)
def test_segments_around_the_chunk_against_plain_prefix_products(exclusive, reverse):
    cts = case()
    eng = ScanEngine()
    got = eng.ciphertext_cumsum_batch(cts, LENGTHS, N, exclusive=exclusive, reverse=reverse)
    assert got == oracle(cts, LENGTHS, exclusive, reverse)
    be = eng.backend
    check_launches(be, len(cts))
    # chunk 4: segments of 1, 4, 5, 9, 1 rows are 1, 1, 2, 3, 1 pieces; one level of carries (3 pieces fit one piece)
    assert [(r[0], r[1], r[2], r[3]) for r in be.runs] == [(20, 8, 4, True)]
    assert [(s[0], s[1], s[2], s[3], s[4]) for s in be.scans] == [(8, 5, 4, False, True), (20, 8, 4, True, exclusive)]
    assert sorted(be.scans[1][5]) == list(range(20))                                   # every output row, once
    if exclusive:
        firsts = [0, 1, 5, 10, 19] if not reverse else [0, 4, 9, 18, 19]
        assert all(got[i] == 1 for i in firsts)


@pytest.mark.parametrize("chunk", [1, 2, 3, 1000])
@pytest.mark.parametrize("exclusive,reverse", FORMS)
def test_chunk_overrides_change_nothing(chunk, exclusive, reverse):
    cts = case(chunk)
    eng = ScanEngine()
    got = eng.ciphertext_cumsum_batch(cts, LENGTHS, N, exclusive=exclusive, reverse=reverse, chunk=chunk)
    assert got == oracle(cts, LENGTHS, exclusive, reverse)
    be = eng.backend
    check_launches(be, len(cts))
    assert be.scans[-1][2] == chunk and all(s[2] == max(2, chunk) for s in be.scans[:-1])   # a level has to shrink
    assert all(s[4] for s in be.scans[:-1])                                            # carries are exclusive scans
    assert len(be.scans) == len(be.runs) + 1                                           # totals only where carries exist
    if chunk == 2:
        assert len(be.scans) >= 4                                                      # 9 rows: 5, 3, 2, 1 pieces
    if chunk == 1000:
        assert be.runs == [] and len(be.scans) == 1 and not be.scans[0][3]             # one launch, no totals, no carries


def test_segments_that_fit_one_piece_are_one_scan_launch():
    lengths = [32] * 7 + [0, 5]
    cts = case(5, lengths)
    eng = ScanEngine(chunk_fn=lambda n_rows, n_segments, total: 32)
    assert eng.ciphertext_cumsum_batch(cts, lengths, N) == oracle(cts, lengths)
    be = eng.backend
    assert be.runs == [] and len(be.scans) == 1 and be.scans[0][:4] == (len(cts), 8, 32, False)
    assert be.input_converts == [(0, len(cts))] and be.stores == [len(cts)]


def test_one_series_and_the_librarys_chunk_is_asked_for_every_level():
    seen = []

    def chunk_fn(n_rows, n_segments, total):
        seen.append((n_rows, n_segments, total))
        return 5

    cts = case(9, [131])
    eng = ScanEngine(chunk_fn=chunk_fn)
    for exclusive, reverse in FORMS:
        del seen[:]
        assert eng.ciphertext_cumsum_batch(cts, None, N, exclusive=exclusive, reverse=reverse) == oracle(cts, [131], exclusive, reverse)
        assert seen == [(131, 1, 131), (27, 1, 27), (6, 1, 6), (2, 1, 2)]              # 131 -> 27 -> 6 -> 2 -> 1 pieces
        check_launches(eng.backend, 131)


@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("rows_per_stage", [1, 2, 3, 7])
@pytest.mark.parametrize("exclusive,reverse", FORMS)
def test_stage_boundaries_inside_segments(rows_per_stage, chunk, exclusive, reverse):
    cts = case(rows_per_stage)
    eng = ScanEngine()
    budget = rows_per_stage * (72 + 4)                                                  # the double's row_bytes and one index word
    got = eng.ciphertext_cumsum_batch(cts, LENGTHS, N, exclusive=exclusive, reverse=reverse, chunk=chunk, table_budget_bytes=budget)
    assert got == oracle(cts, LENGTHS, exclusive, reverse)
    be = eng.backend
    check_launches(be, len(cts), staged=True)
    stages = -(-len(cts) // rows_per_stage)
    assert len(be.input_converts) == stages and max(hi - lo for lo, hi in be.input_converts) == rows_per_stage
    assert be.picks == stages * (2 if exclusive else 1)                                # the running total: one row, one product if exclusive
    assert any(s[3] for s in be.scans)                                                 # a crossing segment started from a carry


def test_zero_and_non_invertible_inputs_need_no_inverse():
    lengths = [6, 5]
    cts = [7, N, 0, 11, 13, 17, 3 * N, 5, N2 - 1, 1, N2 + 4]
    for exclusive, reverse in FORMS:
        eng = ScanEngine()
        got = eng.ciphertext_cumsum_batch(cts, lengths, N, exclusive=exclusive, reverse=reverse, chunk=2)
        assert got == oracle(cts, lengths, exclusive, reverse)
    assert ScanEngine().ciphertext_cumsum_batch(cts, lengths, N)[:6] == [7, 7 * N % N2, 0, 0, 0, 0]


def test_index_arrays_are_int32_within_the_row_set():
    seen = []

    eng = ScanEngine()
    cts = case(3)
    import scan_engine

    orig = scan_engine.ScanBackend.scan

    def scan(self, rows, n_rows, index, carry, exclusive):
        seen.append((n_rows, index.clone(), None if carry is None else (carry[1], carry[2].clone())))
        return orig(self, rows, n_rows, index, carry, exclusive)

    scan_engine.ScanBackend.scan = scan
    try:
        assert eng.ciphertext_cumsum_batch(cts, LENGTHS, N, reverse=True) == oracle(cts, LENGTHS, reverse=True)
    finally:
        scan_engine.ScanBackend.scan = orig
    assert len(seen) == 2
    for n_rows, index, carry in seen:
        assert index.dtype == torch.int32 and int(index.min()) >= 0 and int(index.max()) <= n_rows
        if carry is not None:
            assert carry[1].dtype == torch.int32 and int(carry[1].min()) >= 0 and int(carry[1].max()) <= carry[0]
    # the level of the rows: segments reversed in place, pieces of 4, padded with the one row (20)
    assert seen[1][1].tolist() == [[0, 20, 20, 20], [4, 3, 2, 1], [9, 8, 7, 6], [5, 20, 20, 20],
                                   [18, 17, 16, 15], [14, 13, 12, 11], [10, 20, 20, 20], [19, 20, 20, 20]]
    assert seen[1][2][1].tolist() == list(range(8))                                    # piece p starts from carry row p


def test_refusals_come_before_any_backend_call():
    cts = case()
    for bad, lengths in (("negative", [21, -1]), ("sum", [3, 4]), ("sum", []), ("dtype", [1.0] * 20),
                         ("dtype", torch.ones(20)), ("dims", [[10], [10]]), ("dims", torch.ones((2, 2), dtype=torch.int64))):
        eng = ScanEngine()
        with pytest.raises(ValueError):
            eng.ciphertext_cumsum_batch(cts, lengths, N)
        assert eng.backend is None and eng.calls == [], bad
    for n in (4, 0, -7):                                                               # a modulus the pair kernel refuses
        eng = ScanEngine()
        with pytest.raises(ValueError):
            eng.ciphertext_cumsum_batch(cts, None, n)
        assert eng.backend is None
    with pytest.raises(ValueError):
        ScanEngine().ciphertext_cumsum_batch(cts, None, N, chunk=65537)
    assert sp.as_lengths(np.array([2, 3], dtype=np.uint8), 5).tolist() == [2, 3]
    assert sp.as_lengths(torch.tensor([5], dtype=torch.int32), 5).dtype == torch.int64


def test_no_ciphertexts_and_empty_segments():
    eng = ScanEngine()
    assert eng.ciphertext_cumsum_batch([], [], N) == [] and eng.ciphertext_cumsum_batch([], [0, 0], N) == []
    assert eng.ciphertext_cumsum_batch([], None, N) == []
    assert eng.backend.input_converts == [] and eng.backend.scans == []
    assert H.cumsum([], N, engine=eng) == [] and H.cumsum([[], []], N, engine=eng) == [[], []]


class Ct:
    """The reference's ciphertext object, as far as homomorphic._values reads it."""

    class _Scheme:
        class public_key:
            n = N

    scheme = _Scheme

    def __init__(self, v):
        self.v, self.reads = v, 0

    def get_value(self):
        self.reads += 1
        return self.v


class Randomizer:
    def __init__(self):
        self.asked = []

    def spec(self, n, count):
        self.asked.append((n, count))
        return ("spec", n, count)


def test_public_interface_flat_and_nested():
    cts = case(11)
    eng = ScanEngine()
    assert H.cumsum(cts, N, engine=eng) == oracle(cts, [len(cts)])
    assert eng.calls[-1][1:] == ([len(cts)], False, False, None)
    nested, lo = [], 0
    for k in LENGTHS:
        nested.append(cts[lo : lo + k])
        lo += k
    for exclusive, reverse in FORMS:
        got = H.cumsum(nested, N, exclusive=exclusive, reverse=reverse, engine=eng)
        assert [len(g) for g in got] == LENGTHS
        assert [v for g in got for v in g] == oracle(cts, LENGTHS, exclusive, reverse)
        assert eng.calls[-1][1:] == (LENGTHS, exclusive, reverse, None)
    assert H.cumsum([tuple(cts[:3]), cts[3:5]], N, engine=eng) == [oracle(cts[:3], [3]), oracle(cts[3:5], [2])]
    with pytest.raises(ValueError):
        H.cumsum([cts[0], [cts[1]]], N, engine=eng)
    with pytest.raises(ValueError):
        H.cumsum(cts)                                                                  # plain ints need the modulus


def test_public_interface_objects_and_randomizer():
    a, b = Ct(12345), Ct(N2 - 5)
    eng, rnd = ScanEngine(), Randomizer()
    got = H.cumsum([[a, b, a], [b, 77]], engine=eng, randomizer=rnd, exclusive=True)
    assert got == [[1, 12345, 12345 * (N2 - 5) % N2], [1, N2 - 5]]
    assert (a.reads, b.reads) == (1, 1)                                                # once per distinct object
    assert rnd.asked == [(N, 5)] and eng.calls[-1][4] == ("spec", N, 5)
    assert eng.calls[-1][0] == [12345, N2 - 5, 12345, N2 - 5, 77]
    assert H.cumsum([a, b], engine=eng, reverse=True) == [12345 * (N2 - 5) % N2, N2 - 5]
    assert eng.calls[-1][4] is None


def test_abi_refuses_bad_launches_before_anything_is_enqueued():
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    assert lib.mx_version() == 404
    # a descriptor that names memory which is never read, because every call below is refused first
    buf = (ctypes.c_uint32 * 64)()
    ptr = ctypes.addressof(buf)
    plan = _lib.NsquarePlan(d_plan=ptr, plan_bytes=256, limbs_n=64, n_bits=2048, geometries=1)
    no_block = _lib.NsquarePlan(d_plan=None, limbs_n=64, n_bits=2048, geometries=1)
    no_narrow = _lib.NsquarePlan(d_plan=ptr, limbs_n=64, n_bits=2048, geometries=0)
    too_wide = _lib.NsquarePlan(d_plan=ptr, limbs_n=625, n_bits=20000, geometries=1)

    ok = dict(plan=plan, rows=ptr, n_rows=5, index=ptr, pieces=3, chunk=4, crows=ptr, n_carry=3, cindex=ptr, excl=0, out=ptr,
              limbs2=128, out_bytes=1 << 40, lpl=0)

    def run(**kw):
        a = dict(ok, **kw)
        return lib.mx_scan_nsquare_run(a["plan"], a["rows"], a["n_rows"], a["index"], a["pieces"], a["chunk"], a["crows"],
                                       a["n_carry"], a["cindex"], a["excl"], a["out"], a["limbs2"], a["out_bytes"], a["lpl"], None)

    for kw in (dict(plan=None), dict(plan=no_block), dict(rows=None), dict(index=None), dict(out=None), dict(cindex=None),
               dict(n_rows=0), dict(n_rows=-1), dict(n_rows=1 << 31), dict(pieces=0), dict(pieces=-1), dict(n_carry=-1),
               dict(n_carry=1 << 31), dict(chunk=0), dict(chunk=-1), dict(chunk=65537), dict(limbs2=0), dict(limbs2=127),
               dict(lpl=18)):
        assert run(**kw) == -1, kw
    assert run(plan=no_narrow) == -2 and run(plan=too_wide, limbs2=1250) == -2
    assert run(pieces=1 << 40) == -2                                               # beyond one grid
    assert run(out_bytes=6 * 576 - 1) == -4 and run(out_bytes=0) == -4             # the row set and its one row
    assert run(crows=None, cindex=None, n_carry=-5, out_bytes=6 * 576 - 1) == -4   # a null carry set is legal: the next refusal

    ok = dict(plan=plan, rows=ptr, n_rows=5, out=ptr, limbs2=128, out_bytes=1 << 40, lpl=0)

    def store(**kw):
        a = dict(ok, **kw)
        return lib.mx_scan_nsquare_store(a["plan"], a["rows"], a["n_rows"], a["out"], a["limbs2"], a["out_bytes"], a["lpl"], None)

    for kw in (dict(plan=None), dict(plan=no_block), dict(rows=None), dict(out=None), dict(n_rows=0), dict(n_rows=-2),
               dict(n_rows=1 << 31), dict(limbs2=0), dict(limbs2=127), dict(lpl=18)):
        assert store(**kw) == -1, kw
    assert store(plan=no_narrow) == -2 and store(plan=too_wide, limbs2=1250) == -2
    assert store(out_bytes=5 * 128 * 4 - 1) == -4                                  # canonical rows

    lanes, lpl = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    count = lib.mx_scan_nsquare_instances(lanes, lpl, 8)
    assert [(lanes[i], lpl[i]) for i in range(count)] == [(kk, 9) for kk in (1, 2, 4, 8, 16, 32)]
    assert lib.mx_scan_nsquare_instances(None, None, 4) == -1


def test_no_scan_kernel_has_a_private_segment():
    """private_segment_fixed_size 0 and no spilled register for the six scan instances and the six store instances of
    the BUILT library, read the way tests/test_instances.py reads it for the modexp kernels."""
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root / "tools"))
    import scratch_report

    from protocols.distributed_keygen_amd import _lib

    rows = scratch_report.kernels_of_library(_lib.LIB_PATH)
    names = scratch_report.demangle([r[0] for r in rows])
    scan = [r for r in rows if "scan_n2_" in names[r[0]]]
    for kk in (1, 2, 4, 8, 16, 32):
        for kernel in ("scan_n2_kernel", "scan_n2_store_kernel"):
            assert any(f"mx::{kernel}<{kk}, 9, 29>" in names[r[0]] for r in scan), (kernel, kk)
    assert len(scan) == 12
    assert not [(names[r[0]], r[1], r[2]) for r in scan if r[1] or r[2]]
    assert not [names[r[0]] for r in scan if "hist_n2" in names[r[0]]]                 # the histogram's own count stays 12
