"""Host logic of the batched encrypted matrix product (multiexp_plan.plan_matmul / execute_matmul, homomorphic.matmul) on
the CPU: the planner's launches are executed by a backend over Python ints whose only arithmetic is ``pow`` and
products, laid out exactly as csrc/mx_matmul_n2.hpp reads its tables, and every result is held against ``pow``."""

from __future__ import annotations

import ctypes
import functools
import random

import numpy as np
import pytest

from protocols.distributed_keygen_amd import homomorphic as H
from protocols.distributed_keygen_amd import multiexp_plan as mp

N = ((1 << 127) - 1) * ((1 << 61) - 1)             # odd, 188 bits, two primes (the modulus of test_homomorphic_host.py)
N2 = N * N
ENTRY_BYTES = 576


def shape_fn(window=3, chunk=1 << 30):
    """The shape query's contract with a fixed window and split: the tile is the largest sample count whose tables fit."""
    def shape(n_cols, n_rows, terms, bits, batch, budget, win):
        per_sample = n_cols * (ENTRY_BYTES << window)
        tile = batch if per_sample == 0 else budget // per_sample
        return (win or window), max(1, min(batch, tile)), chunk
    return shape


class PyBackend:
    """multiexp_plan.execute_matmul over Python ints.  A column block is a list of columns (lists over the samples)."""

    def __init__(self, n):
        self.n, self.n2 = n, n * n
        self.launches = []          # (tables given, n_cols, n_shared, tile, launch, window)

    def columns(self, inputs, n_inputs, batch, cols):
        return [[inputs[b * n_inputs + i] for b in range(batch)] for i in cols]

    def invert(self, block):
        return [[pow(v, -1, self.n2) for v in col] for col in block]        # ValueError as pow

    def tile(self, block, batch, lo, hi):
        assert all(len(col) == batch for col in block)
        return [v for col in block for v in col[lo:hi]]

    def bias_rows(self, residues):
        return [(1 + b * self.n) % self.n2 for b in residues]

    def concat(self, parts):
        return [v for part in parts for v in part]

    def run_matmul(self, tables, n_cols, n_shared, tile, launch, window):
        if tables is not None:
            self.tables = tables
        assert len(self.tables) == n_cols * tile + n_shared
        self.launches.append((tables is not None, n_cols, n_shared, tile, launch, window))
        rows, terms = launch.index.shape
        w = launch.weights.reshape(rows, terms, -1)
        exps = [[int.from_bytes(w[r, t].astype("<u4").tobytes(), "little") for t in range(terms)] for r in range(rows)]
        assert all(e.bit_length() <= launch.weight_bits for row in exps for e in row)
        out = []
        for b in range(tile):
            for r in range(rows):
                acc = 1
                for t in range(terms):
                    i = int(launch.index[r, t])
                    assert -n_shared <= i < n_cols or exps[r][t] == 0
                    table = self.tables[i * tile + b] if i >= 0 else self.tables[n_cols * tile + (-1 - i)]
                    acc = acc * pow(table, exps[r][t], self.n2) % self.n2
                out.append(acc)
        return out

    def select(self, outs, picks, tile, column_major):
        width = [len(o) // tile for o in outs]
        get = lambda b, pk: 1 if pk is None else outs[pk[0]][b * width[pk[0]] + pk[1]]
        if column_major:
            return [get(b, pk) for pk in picks for b in range(tile)]
        return [get(b, pk) for b in range(tile) for pk in picks]


class Untouchable:
    """A backend no refusal may reach."""

    def __getattr__(self, name):
        raise AssertionError(f"the backend was touched ({name}) before the refusal")


class FakeEngine:
    """The engine surface homomorphic.matmul uses, with the planner in front of a backend over ints."""

    def __init__(self, backend=None, **shape):
        self.backend, self.shape, self.calls = backend, shape_fn(**shape), []

    def ciphertext_matmul_batch(self, samples, weights, n, bias=None, fixed_base=None):
        self.calls.append((samples, fixed_base))
        if not samples:
            return []
        width = len(samples[0])
        plan = mp.plan_matmul(weights, width, n, bias, len(samples), self.shape)
        be = self.backend or PyBackend(n)
        flat = mp.execute_matmul(plan, be, [int(c) % (n * n) for smp in samples for c in smp], len(samples))
        return [flat[b * plan.n_rows : (b + 1) * plan.n_rows] for b in range(len(samples))]


def oracle(samples, weights, n, bias=None):
    n2 = n * n
    out = []
    for smp in samples:
        ys = []
        for j, row in enumerate(weights):
            items = row.items() if isinstance(row, dict) else enumerate(row)
            acc = (1 + (bias[j] % n) * n) % n2 if bias is not None else 1
            for i, w in items:
                acc = acc * pow(smp[i], w, n2) % n2
            ys.append(acc)
        out.append(ys)
    return out


SPECIAL = (0, 1, -1, (1 << 63) + 5, -((1 << 64) - 3), (1 << 200) + 7, -((1 << 130) + 1), 1 << 63, -(1 << 63))


def make_weights(rng, rows, cols, kind):
    """Signed weights, mostly 12-bit, with zeros, +-1, 64-bit and beyond-int64 values sprinkled in; `kind` is "dense",
    "sparse" ({column: weight} rows), "mixed" (alternating) or "int64" (a dense block the array path takes)."""
    out = []
    for j in range(rows):
        dense = []
        for i in range(cols):
            roll = rng.random()
            if kind == "int64":
                dense.append(rng.choice((0, 1, -1, (1 << 62) + 3, -(1 << 62))) if roll < 0.2 else rng.randrange(-4096, 4096))
            else:
                dense.append(rng.choice(SPECIAL) if roll < 0.15 else rng.randrange(-4096, 4096))
        if kind == "sparse" or (kind == "mixed" and j % 2):
            keep = [i for i in range(cols) if rng.random() < 0.5]
            rng.shuffle(keep)
            out.append({i: dense[i] for i in keep})
        else:
            out.append(dense)
    return out


SHAPES = [(b, i, r) for b in (1, 5, 37) for i in (0, 1, 7, 130) for r in (1, 3)]
KINDS = ("dense", "sparse", "mixed", "int64")
BIASES = ("none", "negative", "large")


@functools.lru_cache(maxsize=None)
def case(k):
    """Case k: (samples, weights, bias, expected), the oracle computed once and shared by the three ways of running it.
    Kinds of rows and of bias cycle over the shapes so that every kind meets every B, I and R."""
    batch, cols, rows = SHAPES[k]
    rng = random.Random(1000 + k)
    kind = KINDS[(k + k // 8) % len(KINDS)]
    bias_kind = BIASES[(k + k // 3) % len(BIASES)]
    samples = [[rng.randrange(1, N2) for _ in range(cols)] for _ in range(batch)]
    weights = make_weights(rng, rows, cols, kind)
    if bias_kind == "none":
        bias = None
    elif bias_kind == "negative":
        bias = [-rng.randrange(1, 1 << 70) for _ in range(rows)]
    else:
        bias = [N * rng.randrange(1, 9) + rng.randrange(N) for _ in range(rows)]
    if bias is not None and rows > 1:
        bias[1] = 0                                   # a row without a bias among rows with one
    return samples, weights, bias, oracle(samples, weights, N, bias)


def run(samples, weights, bias, shape, budget=mp.TABLE_BUDGET_BYTES):
    width = len(samples[0])
    plan = mp.plan_matmul(weights, width, N, bias, len(samples), shape, table_budget=budget)
    be = PyBackend(N)
    flat = mp.execute_matmul(plan, be, [c for smp in samples for c in smp], len(samples))
    return plan, be, [flat[b * plan.n_rows : (b + 1) * plan.n_rows] for b in range(len(samples))]


@pytest.mark.parametrize("k", range(len(SHAPES)))
@pytest.mark.parametrize("mode", ["plain", "chunk16", "three_samples"])
def test_random_cases_match_pow(k, mode):
    samples, weights, bias, want = case(k)
    batch, cols, rows = SHAPES[k]
    if mode == "plain":
        plan, be, got = run(samples, weights, bias, shape_fn())
        assert not plan.combine
    elif mode == "chunk16":
        plan, be, got = run(samples, weights, bias, shape_fn(chunk=16))
        longest = max(len(r) if isinstance(r, dict) else sum(1 for w in r if w) for r in weights) + (bias is not None)
        if longest > 17:
            assert plan.combine and any(lch[5] == 1 and lch[2] == 0 for lch in be.launches)       # the second pass ran
        assert all(l.index.shape[1] <= 16 for l in plan.launches)
    else:
        n_cols = mp.plan_matmul(weights, cols, N, bias, batch, shape_fn()).n_cols
        budget = 3 * n_cols * (ENTRY_BYTES << 3) + 100
        plan, be, got = run(samples, weights, bias, shape_fn(), budget)
        if n_cols and plan.launches:
            assert plan.tile_batch == min(3, batch)
            assert {lch[3] for lch in be.launches} == {min(3, batch)} | ({batch % 3} if batch > 3 and batch % 3 else set())     # ragged last tile
    assert got == want
    assert all(0 <= v < N2 for ys in got for v in ys)


def _terms_of(plan):
    """pass-1 row -> [(index, weight)] with the padding dropped."""
    out = {}
    for launch in plan.launches:
        r, t = launch.index.shape
        w = launch.weights.reshape(r, t, -1)
        for k, rid in enumerate(launch.rows):
            terms = [(int(launch.index[k, c]), int.from_bytes(w[k, c].astype("<u4").tobytes(), "little")) for c in range(t)]
            assert rid not in out
            out[rid] = [(i, e) for i, e in terms if e]
    return out


def test_planner_invariants():
    rng = random.Random(7)
    rows, cols = 5, 90
    weights = make_weights(rng, rows, cols, "mixed")
    weights[3] = [0] * cols                                   # an all-zero row with a bias, and one without
    weights[4] = {}
    bias = [3, 0, -1, N + 5, 0]
    plans = {b: mp.plan_matmul(weights, cols, N, bias, b, shape_fn(chunk=16)) for b in (1, 37, 100000)}
    plan = plans[37]
    dense = [[(row.get(i, 0) if isinstance(row, dict) else row[i]) for i in range(cols)] for row in weights]
    # the inverted columns are exactly those with a negative weight, the plain ones those with a positive weight
    assert plan.inverted == [i for i in range(cols) if any(r[i] < 0 for r in dense)]
    assert plan.x_cols == [i for i in range(cols) if any(r[i] > 0 for r in dense)]
    assert plan.n_cols == len(plan.x_cols) + len(plan.inverted)
    # one shared bias table per biased row
    assert plan.bias == {0: 3, 2: N - 1, 3: 5}
    terms = _terms_of(plan)
    shared_seen = sorted(-1 - i for ts in terms.values() for i, _ in ts if i < 0)
    assert shared_seen == [0, 1, 2]
    # every non-zero term of W appears once, in exactly one piece of its row; pieces hold at most `chunk` terms
    assert sorted(terms) == list(range(plan.pass1_rows))
    assert all(len(ts) <= 16 for ts in terms.values())
    pieces = {j: [] for j in range(rows)}
    for j, (kind, v) in enumerate(plan.result):
        if kind == "p1":
            pieces[j] = [v]
        elif kind == "p2":
            launch = next(l for l in plan.combine if v in l.rows)
            k = launch.rows.index(v)
            pieces[j] = [plan.part_rows[int(c)] for c, e in zip(launch.index[k], launch.weights[k].reshape(-1)) if e]
    assert sorted(m for ms in pieces.values() for m in ms) == list(range(plan.pass1_rows))
    col_of = {c: ("x", i) for c, i in enumerate(plan.x_cols)}
    col_of.update({len(plan.x_cols) + c: ("inv", i) for c, i in enumerate(plan.inverted)})
    shared_rows = sorted(plan.bias)
    for j in range(rows):
        got = sorted((col_of[i] if i >= 0 else ("bias", shared_rows[-1 - i]), e) for m in pieces[j] for i, e in terms[m])
        want = sorted([(("x", i) if w > 0 else ("inv", i), abs(w)) for i, w in enumerate(dense[j]) if w]
                      + ([(("bias", j), 1)] if j in plan.bias else []))
        assert got == want, j
    assert plan.result[4] == ("one", 0) and plan.result[3][0] == "p1"
    # the launch arrays have rows x pieces leading entries whatever the batch is
    lead = lambda p: [l.index.shape for l in p.launches + p.combine]
    assert lead(plans[1]) == lead(plans[37]) == lead(plans[100000])
    assert sum(s[0] for s in lead(plan)[: len(plan.launches)]) == plan.pass1_rows == sum(-(-len([1 for w in r if w] + ([1] if j in plan.bias else [])) // 16) for j, r in enumerate(dense))
    for l in plan.launches + plan.combine:
        assert l.weights.shape[:2] == l.index.shape and l.index.dtype == np.int32 and l.weights.dtype == np.uint32


def test_dense_int64_blocks_take_the_array_path_and_agree_with_the_general_one():
    rng = random.Random(11)
    weights = make_weights(rng, 4, 33, "int64")
    samples = [[rng.randrange(1, N2) for _ in range(33)] for _ in range(6)]
    assert mp._dense_block(weights, 33) is not None
    as_lists = run(samples, weights, [1, 2, 3, 4], shape_fn())
    as_array = run(samples, np.array(weights, dtype=np.int64), [1, 2, 3, 4], shape_fn())
    as_dicts = run(samples, [dict(enumerate(r)) for r in weights], [1, 2, 3, 4], shape_fn())
    assert as_lists[2] == as_array[2] == as_dicts[2] == oracle(samples, weights, N, [1, 2, 3, 4])
    assert [l.index.tolist() for l in as_lists[0].launches] == [l.index.tolist() for l in as_dicts[0].launches]


def test_edge_shapes():
    rng = random.Random(3)
    eng = FakeEngine()
    assert H.matmul([], [[1, 2]], n=N, engine=eng) == []                                   # B = 0
    samples = [[rng.randrange(1, N2) for _ in range(2)] for _ in range(3)]
    assert H.matmul(samples, [], n=N, engine=eng) == [[], [], []]                           # R = 0
    assert H.matmul([[], []], [[], {}], n=N, bias=[5, 0], engine=eng) == [[1 + 5 * N, 1]] * 2     # I = 0: 1 + bias N
    assert H.matmul([[], []], [[], {}], n=N, engine=eng) == [[1, 1]] * 2
    assert H.matmul([[0, 7]], [[0, 2], {0: 0}], n=N, engine=eng) == [[49, 1]]               # a zero weight on a zero input gives 1
    assert H.matmul([[0, 7]], [[1, 2]], n=N, engine=eng) == [[0]]


def test_every_refusal_raises_before_the_backend_is_touched():
    eng = FakeEngine(backend=Untouchable())
    good = [[3, 5, 7], [9, 11, 13]]
    bound = mp.weight_bound(N)
    with pytest.raises(ValueError):
        H.matmul([[3, 5, 7], [9, 11]], [[1, 1, 1]], n=N, engine=eng)                      # a sample of the wrong length
    assert not eng.calls
    for weights, bias in (([[1, 2]], None),                                                # a row of the wrong length
                          ([[1, 2, 3, 4]], None),
                          ([{3: 1}], None), ([{-1: 1}], None),                             # a bad column
                          ([[1, bound, 1]], None), ([{0: -bound}], None),                  # a weight out of bounds
                          ([[1, 2, 3]], [1, 2]), ([[1, 2, 3]], [])):                       # a bias of the wrong length
        with pytest.raises(ValueError):
            H.matmul(good, weights, n=N, bias=bias, engine=eng)
    assert H.matmul(good, [[1, bound - 1, 1 - bound]], n=N, engine=FakeEngine()) == oracle(good, [[1, bound - 1, 1 - bound]], N)
    with pytest.raises(ValueError):
        H.matmul([[3, 5]], [[1, 1]], engine=eng)                                           # plain ints need n
    # a negative weight on a non-invertible input: ValueError as pow (this one comes from the backend's inversion)
    with pytest.raises(ValueError):
        H.matmul([[3, N]], [[1, -1]], n=N, engine=FakeEngine())
    assert H.matmul([[3, N]], [[1, 1]], n=N, engine=FakeEngine()) == [[3 * N]]


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


def test_get_value_is_called_once_per_object_and_the_randomiser_covers_every_output():
    rng = random.Random(5)
    a, b, c = (Ct(rng.randrange(1, N2)) for _ in range(3))
    eng = FakeEngine()

    class Rz:
        def spec(self, n, count):
            return ("spec", n, count)

    got = H.matmul([[a, b, a], [c, c, b]], [[1, -2, 3], {1: 5}], bias=[1, 2], engine=eng, randomizer=Rz())
    assert (a.reads, b.reads, c.reads) == (1, 1, 1)
    assert got == oracle([[a.v, b.v, a.v], [c.v, c.v, b.v]], [[1, -2, 3], {1: 5}], N, [1, 2])
    assert eng.calls[-1][1] == ("spec", N, 4)                      # B * R outputs


def test_abi_refuses_bad_arguments_without_a_launch():
    """The new entry points validate before they touch the runtime: on a machine without a GPU."""
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    assert lib.mx_version() == 404
    ints = lambda k: [ctypes.c_int() for _ in range(k)]
    i64s = lambda k: [ctypes.c_int64() for _ in range(k)]
    k, l, w = ints(3)
    tile, chunk = i64s(2)
    assert lib.mx_matmul_nsquare_shape(2048, 512, 16, 513, 16, 1024, 256 << 20, 0, 0, k, l, w, tile, chunk) == 0
    assert (k.value, l.value) == (8, 9) and 1 <= w.value <= 6
    per_sample = 512 * (2 * 8 * 9 * 4 << w.value)
    assert tile.value == min(1024, (256 << 20) // per_sample) and tile.value >= 1 and chunk.value >= 64
    assert lib.mx_matmul_nsquare_shape(2048, 512, 16, 513, 16, 1024, 1, 0, 0, k, l, w, tile, chunk) == 0
    assert (w.value, tile.value) == (1, 1)                         # a budget below one sample: the smallest window, one sample
    assert lib.mx_matmul_nsquare_shape(2048, 512, 16, 513, 16, 1024, 1 << 40, 0, 5, k, l, w, tile, chunk) == 0
    assert (w.value, tile.value, chunk.value) == (5, 1024, 513)    # an explicit window; everything fits; outputs fill the device
    for bad in ((2048, -1, 16, 513, 16, 4, 1 << 20, 0, 0), (2048, 4, -1, 5, 16, 4, 1 << 20, 0, 0), (2048, 4, 4, 5, -1, 4, 1 << 20, 0, 0),
                (2048, 4, 4, 5, 16, -1, 1 << 20, 0, 0), (2048, 4, 4, 5, 16, 4, -1, 0, 0), (2048, 4, 4, 5, 16, 4, 1 << 20, 0, 9),
                (2048, 4, 4, 5, 16, 4, 1 << 20, 18, 0)):
        assert lib.mx_matmul_nsquare_shape(*bad, k, l, w, tile, chunk) == -1, bad
    assert lib.mx_matmul_nsquare_shape(2048, 4, 4, 5, 16, 4, 1 << 20, 0, 0, None, l, w, tile, chunk) == -1
    assert lib.mx_matmul_nsquare_shape(20000, 4, 4, 5, 16, 4, 1 << 20, 0, 0, k, l, w, tile, chunk) == -2       # no narrow instance
    for huge in ((2048, (1 << 31) + 1, 4, 5, 16, 4, 1 << 20, 0, 0), (2048, 4, 1 << 62, 5, 16, 4, 1 << 20, 0, 0),
                 (2048, 4, 4, 1 << 62, 16, 4, 1 << 20, 0, 0)):
        assert lib.mx_matmul_nsquare_shape(*huge, k, l, w, tile, chunk) == -2, huge          # no overflowing products
    assert lib.mx_matmul_nsquare_shape(2048, 1 << 31, 1 << 31, 1 << 31, 16, 1 << 62, (1 << 63) - 1, 0, 0, k, l, w, tile, chunk) == 0
    assert 1 <= tile.value <= 1 << 30 and chunk.value >= 1
    assert lib.mx_matmul_nsquare_workspace_bytes(2048, 4, 1, 3, 0, 4) == lib.mx_multiexp_nsquare_workspace_bytes(2048, 13, 0, 4) > 0
    assert lib.mx_matmul_nsquare_workspace_bytes(2048, 4, 1, 0, 0, 4) == -1
    assert lib.mx_matmul_nsquare_workspace_bytes(2048, 4, 1, 3, 0, 9) == -1
    assert lib.mx_matmul_nsquare_workspace_bytes(20000, 4, 1, 3, 0, 4) == -2
    assert lib.mx_matmul_nsquare_workspace_bytes(2048, 1 << 31, 0, 1 << 30, 0, 8) == -2         # no wrapped byte count
    assert lib.mx_matmul_nsquare_workspace_bytes(2048, 1 << 31, 0, 16, 0, 1) == -2
    assert lib.mx_matmul_nsquare_workspace_bytes(2048, (1 << 31) + 1, 0, 1, 0, 1) == -1
    lanes, lpl = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    count = lib.mx_matmul_nsquare_instances(lanes, lpl, 8)
    assert [(lanes[i], lpl[i]) for i in range(count)] == [(kk, 9) for kk in (1, 2, 4, 8, 16, 32)]
    assert lib.mx_matmul_nsquare_instances(None, None, 4) == -1
    # the run: a descriptor that names device memory which is never read, because every call below is refused first
    buf = (ctypes.c_uint32 * 64)()
    ptr = ctypes.addressof(buf)
    plan = _lib.NsquarePlan(d_plan=ptr, plan_bytes=256, limbs_n=64, n_bits=2048, geometries=1)
    ok = dict(plan=plan, inputs=ptr, n_cols=4, n_shared=1, tile=3, limbs2=128, index=ptr, weights=ptr, terms=5, bits=16,
              out=ptr, rows=2, lpl=0, window=4, ws=ptr, ws_bytes=1 << 40)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mx_matmul_nsquare_run(a["plan"], a["inputs"], a["n_cols"], a["n_shared"], a["tile"], a["limbs2"], a["index"],
                                         a["weights"], a["terms"], a["bits"], a["out"], a["rows"], a["lpl"], a["window"], a["ws"],
                                         a["ws_bytes"], None)

    for kw in (dict(plan=None), dict(out=None), dict(ws=None), dict(index=None), dict(weights=None), dict(n_cols=-1), dict(n_shared=-1),
               dict(n_cols=0, n_shared=0), dict(tile=0), dict(rows=0), dict(limbs2=0), dict(terms=-1), dict(bits=-1), dict(window=0),
               dict(window=9), dict(lpl=18), dict(bits=2 * 2048 + 65), dict(limbs2=127),
               dict(plan=_lib.NsquarePlan(d_plan=None, limbs_n=64, n_bits=2048, geometries=1))):
        assert call(**kw) == -1, kw
    assert call(plan=_lib.NsquarePlan(d_plan=ptr, limbs_n=64, n_bits=2048, geometries=0)) == -2      # a plan without the narrow constants
    assert call(plan=_lib.NsquarePlan(d_plan=ptr, limbs_n=625, n_bits=20000, geometries=1), limbs2=1250) == -2
    assert call(rows=1 << 40) == -2                                                          # beyond one grid
    assert call(ws_bytes=1024) == -4


@pytest.mark.parametrize("rows,terms,splits", [(4, 200000, True), (4, 513, True), (4, 64, False), (100000, 513, False)])
def test_one_split_k_rule_for_the_linear_map_and_the_matrix_product(rows, terms, splits):
    """For one sample in a tile of one, the matrix product's outputs are the linear map's: both shape queries must cut
    the terms into the same chunks — few rows with more than 64 terms split, 64 terms or rows that fill the device do not.
    The convolution planner is the third: one 1 x `terms` kernel over `rows` positions of one image (a tile of its own
    under a budget that holds it) is cut at the same chunk, into the pieces and results of the one split-K rule."""
    from protocols.distributed_keygen_amd import _lib
    from protocols.distributed_keygen_amd import conv_plan as cp

    lib = _lib.lib()
    for n_bits in (128, 2048):
        k, l, w, k2, l2, w2 = (ctypes.c_int() for _ in range(6))
        tile, chunk, chunk2 = (ctypes.c_int64() for _ in range(3))
        assert lib.mx_matmul_nsquare_shape(n_bits, 32, rows, terms, 16, 1, 1 << 40, 0, 0, k, l, w, tile, chunk) == 0
        assert lib.mx_multiexp_nsquare_shape(n_bits, 32, rows, terms, 16, 0, 0, k2, l2, w2, chunk2) == 0
        assert tile.value == 1 and (k.value, l.value) == (k2.value, l2.value)
        assert chunk.value == chunk2.value
        assert (64 <= chunk.value < terms) if splits else chunk.value == terms

        def conv_shape(n_tables, n_outputs, n_terms, bits, win):
            kc, lc, wc, cc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
            assert lib.mx_multiexp_nsquare_shape(n_bits, n_tables, n_outputs, n_terms, bits, 0, win, kc, lc, wc, cc) == 0
            return wc.value, cc.value, 2 * kc.value * lc.value * 4

        plan = cp.plan_conv([[[[1 << 15] * terms]]], (1, 1, rows, terms), (1 << n_bits) - 1, None, conv_shape, table_budget=1 << 62)
        assert (plan.tile_images, plan.band_rows, plan.out_w) == (1, rows, 1) and plan.chunk == chunk.value
        pieces = -(-terms // chunk.value)
        assert plan.pass1_rows == pieces and all(l.index.shape[1] <= chunk.value for l in plan.launches)
        assert plan.result == [("p2", 0) if splits else ("p1", 0)]
        assert plan.part_rows == (list(range(pieces)) if splits else []) and bool(plan.combine) == splits
