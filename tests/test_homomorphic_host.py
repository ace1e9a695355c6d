"""Host logic of the homomorphic linear maps (protocols/distributed_keygen_amd/multiexp_plan.py, homomorphic.py) on the
CPU: the planner's launches are executed by a backend over Python ints whose only arithmetic is ``pow`` and products,
and every result is held against the Python oracle."""

from __future__ import annotations

import random
from typing import List

import numpy as np
import pytest

from protocols.distributed_keygen_amd import homomorphic as H
from protocols.distributed_keygen_amd import multiexp_plan as mp

N = ((1 << 127) - 1) * ((1 << 61) - 1)             # odd, 188 bits, two primes: random residues are invertible
N2 = N * N


def shape_fn(window=3, chunk=1 << 30, entry_bytes=576):
    return lambda n_tables, n_rows, terms, bits: (window, chunk, entry_bytes)


class PyBackend:
    """multiexp_plan.execute over lists of Python ints (rows = residues mod N^2)."""

    def __init__(self, n):
        self.n, self.n2 = n, n * n
        self.launches = []          # (table rows or None, n_tables, launch, window)

    def take(self, rows, positions):
        return [rows[p] for p in positions]

    def invert(self, rows):
        return [pow(v, -1, self.n2) for v in rows]        # ValueError as pow

    def bias_rows(self, residues):
        return [(1 + b * self.n) % self.n2 for b in residues]

    def gather(self, inputs, inv, bias, parts):
        src = {"x": inputs, "inv": inv, "bias": bias}
        return [src[kind][k] for kind, k in parts]

    def run(self, tables, n_tables, launch, window):
        if tables is not None:
            self.tables = tables
        assert len(self.tables) == n_tables
        self.launches.append((tables, n_tables, launch, window))
        rows, terms = launch.index.shape
        w = launch.weights.reshape(rows, terms, -1)
        out = []
        for r in range(rows):
            acc = 1
            for t in range(terms):
                e = int.from_bytes(w[r, t].astype("<u4").tobytes(), "little")
                acc = acc * pow(self.tables[int(launch.index[r, t])], e, self.n2) % self.n2
            out.append(acc)
        return out

    def rows_of(self, picks):
        return [out[r] for out, r in picks]

    def assemble(self, picks):
        return [1 if p is None else p[0][p[1]] for p in picks]


class FakeEngine:
    """The engine surface homomorphic.py uses, with the planner in front of a PyBackend."""

    def __init__(self, chunk=1 << 30, window=3, budget=mp.TABLE_BUDGET_BYTES):
        self.chunk, self.window, self.budget = chunk, window, budget
        self.backends = []

    def _map(self, cts, weights, n, bias=None):
        n2 = n * n
        vals = [int(c) % n2 for c in cts]
        plan = mp.plan_call(weights, len(vals), n, bias, shape_fn(self.window, self.chunk), table_budget=self.budget)
        be = PyBackend(n)
        self.backends.append((plan, be))
        return mp.execute(plan, be, vals)

    def ciphertext_scale_batch(self, cts, scalars, n):
        return self._map(cts, [{k: s} for k, s in enumerate(scalars)], n)

    def ciphertext_sum_batch(self, groups, n):
        flat, rows = [], []
        for g in groups:
            rows.append({len(flat) + t: 1 for t in range(len(g))})
            flat.extend(g)
        return self._map(flat, rows, n)

    def ciphertext_linear_map_batch(self, cts, weights, n, bias=None):
        return self._map(cts, weights, n, bias)

    def mulmod_batch(self, a, b, mod):
        return [x * y % mod for x, y in zip(a, b)]

    def modinv_batch(self, vals, mod):
        return [pow(v, -1, mod) for v in vals]


def oracle_map(cts, weights, n, bias=None):
    n2 = n * n
    out = []
    for j, row in enumerate(weights):
        items = row.items() if isinstance(row, dict) else enumerate(row)
        acc = (1 + (bias[j] % n) * n) % n2 if bias is not None else 1
        for i, w in items:
            acc = acc * pow(cts[i], w, n2) % n2
        out.append(acc)
    return out


def rand_cts(rng, k):
    return [rng.randrange(1, N2) | 1 for _ in range(k)]


def test_planner_covers_every_term_once_and_split_k_recombines():
    rng = random.Random(1)
    cts = rand_cts(rng, 300)
    weights = [{i: rng.randrange(-50, 50) or 1 for i in rng.sample(range(300), rng.randrange(0, 300))} for _ in range(7)]
    rows = mp.normalize_rows(weights, 300, N)
    plan = mp.plan_multiexp(rows, 300, N, None, shape_fn(chunk=40))
    # every (row, input, weight) of pass 1 appears exactly once among the launches of the first stages
    seen = []
    for stage in plan.stages[: plan.combine_from]:
        for launch in stage.launches:
            r, t = launch.index.shape
            w = launch.weights.reshape(r, t, -1)
            for a, rid in enumerate(launch.rows):
                for b in range(t):
                    e = int.from_bytes(w[a, b].astype("<u4").tobytes(), "little")
                    if e:
                        seen.append((rid, stage.sources[int(launch.index[a, b])], e))
    assert len(seen) == len(set(seen)) == sum(len(r) for r in rows)
    assert plan.combine_from < len(plan.stages), "rows of up to 300 terms with a chunk of 40 must be split"
    assert max(len(l.rows) and l.index.shape[1] for s in plan.stages[: plan.combine_from] for l in s.launches) <= 40
    assert plan.stages[-1].window == 1
    be = PyBackend(N)
    assert mp.execute(plan, be, cts) == oracle_map(cts, weights, N)


def test_ragged_groups_are_bucketed():
    lens = [1, 2, 3, 1000, 5, 700, 0, 64]
    rows = [[(i, 1) for i in range(k)] for k in lens]
    plan = mp.plan_multiexp(rows, 1000, N, None, shape_fn())
    launches = plan.stages[0].launches
    assert len(launches) >= 4
    output_of = {v: j for j, (kind, v) in enumerate(plan.result) if kind == "p1"}
    for launch in launches:
        counts = [lens[output_of[r]] for r in launch.rows]
        assert launch.index.shape[1] == max(counts)
        assert max(counts) <= 2 * max(1, min(counts)), counts        # no row padded to more than twice its length
    assert plan.result[6] == ("one", 0)


def test_negative_weights_map_to_inverted_inputs():
    rows = mp.normalize_rows([{0: -3, 1: 2}, {0: 5, 2: -1}], 3, N)
    plan = mp.plan_multiexp(rows, 3, N, None, shape_fn())
    assert plan.inverted == [0, 2]
    srcs = set(plan.stages[0].sources)
    assert {("inv", 0), ("x", 1), ("x", 0), ("inv", 2)} == srcs
    for launch in plan.stages[0].launches:
        assert launch.weights.min() >= 0


def test_errors_raise_before_any_launch():
    eng = FakeEngine()
    bound = mp.weight_bound(N)
    with pytest.raises(ValueError):
        eng.ciphertext_scale_batch([3], [bound], N)
    with pytest.raises(ValueError):
        eng.ciphertext_scale_batch([3], [-bound], N)
    with pytest.raises(ValueError):
        eng.ciphertext_linear_map_batch([1, 2, 3], [[1, 2]], N)      # row of the wrong length
    with pytest.raises(ValueError):
        eng.ciphertext_linear_map_batch([1, 2, 3], [{3: 1}], N)      # index out of range
    with pytest.raises(ValueError):
        eng.ciphertext_linear_map_batch([1, 2, 3], [[1, 2, 3]], N, bias=[1, 2])
    with pytest.raises(ValueError):
        H.scale([0], [-1], n=N, engine=eng)                          # not invertible, as pow(0, -1, N^2)
    assert [b for _, b in eng.backends if b.launches] == []          # nothing was launched
    assert eng.ciphertext_scale_batch([3], [bound - 1], N) == [pow(3, bound - 1, N2)]     # the largest weight taken
    assert H.scale([0, 0], [0, 5], n=N, engine=eng) == [1, 0]        # pow(0, 0, m) == 1


def test_even_modulus_raises_before_any_launch():
    import importlib.util

    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch missing")
    from protocols.distributed_keygen_amd.engine import Engine

    eng = Engine.__new__(Engine)                                    # no device: the check comes first
    with pytest.raises(ValueError):
        Engine.multiexp_nsquare_t(eng, None, [[1]], 10)
    with pytest.raises(ValueError):
        Engine.ciphertext_scale_batch(eng, [3], [2], 1)


class Ct:
    def __init__(self, v, n):
        self.v, self.calls = v, 0
        self.scheme = type("S", (), {"public_key": type("P", (), {"n": n})()})()

    def get_value(self):
        self.calls += 1
        return self.v


def test_get_value_is_called_once_per_distinct_object():
    rng = random.Random(2)
    objs = [Ct(v, N) for v in rand_cts(rng, 4)]
    cts = [objs[0], objs[1], objs[0], objs[2], objs[0], objs[3], objs[1]]
    eng = FakeEngine()
    got = H.linear_map(cts, [[1, 2, 3, 4, 5, 6, 7]], engine=eng)
    assert [o.calls for o in objs] == [1, 1, 1, 1]
    assert got == oracle_map([o.v for o in cts], [[1, 2, 3, 4, 5, 6, 7]], N)
    for o in objs:
        o.calls = 0
    H.sum_groups([cts[:3], cts[3:]], engine=eng)
    assert [o.calls for o in objs] == [1, 1, 1, 1]
    vals = [o.v for o in objs]
    assert H.add(objs[:2], objs[2:], engine=eng) == [vals[0] * vals[2] % N2, vals[1] * vals[3] % N2]
    assert H.neg(objs, engine=eng) == [pow(v, -1, N2) for v in vals]


@pytest.mark.parametrize("chunk,budget", [(1 << 30, mp.TABLE_BUDGET_BYTES), (16, mp.TABLE_BUDGET_BYTES), (16, 576 * 8 * 20)])
def test_random_dense_sparse_and_ragged_cases_match_the_oracle(chunk, budget):
    rng = random.Random(chunk + budget)
    eng = FakeEngine(chunk=chunk, budget=budget)
    cts = rand_cts(rng, 40) + [0, 1, N, N2 - 1, N2 + 5, -7]
    k = len(cts)
    dense = [[rng.randrange(-(1 << 64), 1 << 64) for _ in range(k - 6)] + [0, 1, 1, 2, 3, 4] for _ in range(9)]
    bias = [rng.randrange(-N, 2 * N) for _ in dense]
    assert eng.ciphertext_linear_map_batch(cts, dense, N, bias=bias) == oracle_map([c % N2 for c in cts], dense, N, bias)
    sparse = [{i: rng.randrange(-1000, 1000) for i in rng.sample(range(k - 6), rng.randrange(0, 30))} for _ in range(12)] + [{}, {k - 6: 0}]
    assert eng.ciphertext_linear_map_batch(cts, sparse, N) == oracle_map([c % N2 for c in cts], sparse, N)
    groups = [rand_cts(rng, m) for m in (0, 1, 2, 37, 100, 3)]
    want = []
    for g in groups:
        acc = 1
        for c in g:
            acc = acc * c % N2
        want.append(acc)
    assert eng.ciphertext_sum_batch(groups, N) == want
    scalars = [0, 1, -1, (1 << 64) - 1, -(1 << 64), N, N2, rng.randrange(N2)]
    base = rand_cts(rng, len(scalars))
    assert eng.ciphertext_scale_batch(base, scalars, N) == [pow(c, s, N2) for c, s in zip(base, scalars)]
    if budget < mp.TABLE_BUDGET_BYTES:
        assert len(eng.backends[0][0].stages) > 2                    # the table budget cut pass 1 into stages


def test_dense_int64_rows_are_planned_as_one_block_and_match_the_oracle():
    rng = random.Random(5)
    cts = rand_cts(rng, 24)
    W = [[rng.randrange(-(1 << 63) + 1, 1 << 63) for _ in range(24)] for _ in range(10)]
    W[3][5] = 0                                                   # a zero weight: a weight-0 term of the block
    W[4] = [abs(w) for w in W[4]]
    bias = [rng.randrange(-N, N) for _ in W]
    bias[2] = 0
    plan = mp.plan_call(W, 24, N, bias, shape_fn())
    assert len(plan.stages) == 1 and len(plan.stages[0].launches) == 1
    launch = plan.stages[0].launches[0]
    assert launch.rows == list(range(10)) and launch.index.shape == (10, 25)
    assert plan.inverted == sorted({i for row in W for i, w in enumerate(row) if w < 0})
    want = oracle_map(cts, W, N, bias)
    assert mp.execute(plan, PyBackend(N), cts) == want
    assert mp.execute(mp.plan_call(np.array(W, dtype=np.int64), 24, N, bias, shape_fn()), PyBackend(N), cts) == want
    # the same rows through the term-by-term planner give the same results
    general = mp.plan_multiexp(mp.normalize_rows(W, 24, N), 24, N, bias, shape_fn())
    assert mp.execute(general, PyBackend(N), cts) == want
    # split-K of the block: every row in pieces of 7 terms (the last one padded), a weight-1 combine pass
    plan = mp.plan_call(W, 24, N, bias, shape_fn(chunk=7))
    assert len(plan.stages) == 2 and plan.combine_from == 1 and plan.stages[1].window == 1
    assert plan.stages[0].launches[0].index.shape == (10 * 4, 7)
    assert mp.execute(plan, PyBackend(N), cts) == want


@pytest.mark.parametrize("case", ["min_int64", "beyond_int64", "sparse_rows", "budget"])
def test_dense_block_falls_back_to_the_general_planner(case):
    rng = random.Random(case)
    cts = rand_cts(rng, 16)
    W = [[rng.randrange(1, 1 << 40) for _ in range(16)] for _ in range(4)]
    kw = {}
    if case == "min_int64":
        W[1][2] = -(1 << 63)
    elif case == "beyond_int64":
        W[0][0] = 1 << 63
    elif case == "sparse_rows":
        W[2] = [0] * 14 + [1, 2]
    else:
        kw["table_budget"] = 576 * 8 * 4
    plan = mp.plan_call(W, 16, N, None, kw.pop("shape", shape_fn()), **kw)
    assert len(plan.stages) > 1 or len(plan.stages[0].launches) > 1 or plan.stages[0].launches[0].index.shape[1] < 16 \
        or case in ("min_int64", "beyond_int64")
    assert mp.execute(plan, PyBackend(N), cts) == oracle_map(cts, W, N)
    if case in ("min_int64", "beyond_int64"):
        assert mp._dense_block(W, 16) is None
