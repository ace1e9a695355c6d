"""Host logic of encrypted convolutions (conv_plan.plan_conv / execute_conv, homomorphic.conv2d / conv1d) on the CPU: the
planner's launches are executed by a backend over Python ints whose only arithmetic is ``pow`` and products, with the
tables laid out and ``index + origin`` resolved (clamp included) exactly as csrc/mx_conv_n2.hpp does, and every result
is held against ``pow``.  The geometry is checked independently against torch.nn.functional.conv2d on the plaintexts."""

from __future__ import annotations

import ctypes
import functools
import itertools
import random

import numpy as np
import pytest

import hostpow
import test_matmul_host as tm
from protocols.distributed_keygen_amd import conv_plan as cp
from protocols.distributed_keygen_amd import homomorphic as H
from protocols.distributed_keygen_amd import multiexp_plan as mp
from protocols.distributed_keygen_amd.engine import _grid_shape

N = tm.N
N2 = N * N
ENTRY_BYTES = tm.ENTRY_BYTES


def shape_fn(window=3, chunk=1 << 30):
    """The contract of mx_multiexp_nsquare_shape with a fixed window and split-K chunk."""
    def shape(n_tables, n_outputs, terms, bits, win):
        return (win or window), chunk, ENTRY_BYTES
    return shape


class PyConvBackend(tm.PyBackend):
    """conv_plan.execute_conv over Python ints.  The grids are a flat list [image][padded row][grid][padded column]."""

    def __init__(self, n):
        super().__init__(n)
        self.conv_launches = []      # (tables given, n_local, n_shared, launch, window, positions, image_positions)
        self.tabled = 0              # table inputs handed over, every tile counted

    def grids(self, inputs, shape, x_ch, inverted, padding):
        b, c, h, w = shape
        ph, pw = padding
        hp, wp = h + 2 * ph, w + 2 * pw
        chans = [(ch, False) for ch in x_ch] + [(ch, True) for ch in inverted]
        out = [1] * (b * hp * len(chans) * wp)
        for m in range(b):
            for g, (ch, inv) in enumerate(chans):
                for y in range(h):
                    for x in range(w):
                        v = inputs[((m * c + ch) * h + y) * w + x]
                        out[((m * hp + y + ph) * len(chans) + g) * wp + x + pw] = pow(v, -1, self.n2) if inv else v      # ValueError as pow
        return out, b, hp, len(chans) * wp

    def window(self, grids, m0, m1, r0, r1):
        flat, b, hp, per_row = grids
        assert 0 <= m0 < m1 <= b and 0 <= r0 < r1 <= hp
        return [v for m in range(m0, m1) for v in flat[(m * hp + r0) * per_row : (m * hp + r1) * per_row]]

    def run_conv(self, tables, n_local, n_shared, launch, window, origin, image_positions):
        if tables is not None:
            self.tables = tables
            self.tabled += len(tables)
        n_tables = n_local + n_shared
        assert len(self.tables) == n_tables
        positions = len(origin)
        assert origin.dtype == np.int64 and positions % image_positions == 0
        self.conv_launches.append((tables is not None, n_local, n_shared, launch, window, positions, image_positions))
        rows, terms = launch.index.shape
        w = launch.weights.reshape(rows, terms, -1)
        exps = [[int.from_bytes(w[r, t].astype("<u4").tobytes(), "little") for t in range(terms)] for r in range(rows)]
        assert all(e.bit_length() <= launch.weight_bits for row in exps for e in row)
        out = [None] * (positions * rows)
        for b in range(positions):
            image, within = divmod(b, image_positions)
            for r in range(rows):
                acc = 1
                for t in range(terms):
                    if exps[r][t] == 0:
                        continue                                  # a zero digit in every window: never read
                    i = int(launch.index[r, t])
                    tn = i + int(origin[b]) if i >= 0 else n_local + (-1 - i)
                    assert (0 <= tn < n_local) if i >= 0 else (n_local <= tn < n_tables)       # the host's guarantee
                    tn = min(max(tn, 0), n_tables - 1)                                          # the kernel's clamp
                    acc = acc * pow(self.tables[tn], exps[r][t], self.n2) % self.n2
                out[(image * rows + r) * image_positions + within] = acc
        return out

    def select_conv(self, outs, outs2, picks, images, image_positions, as_columns):
        rows1 = [len(o) // (images * image_positions) for o in outs]
        rows2 = [len(o) // (images * image_positions) for o in outs2]

        def get(m, q, pk):
            if pk is None:
                return 1
            which, k, r = pk
            if which == 1:
                return outs[k][(m * rows1[k] + r) * image_positions + q]
            return outs2[k][(m * image_positions + q) * rows2[k] + r]           # run_matmul's sample-major results

        if as_columns:
            return [get(m, q, pk) for pk in picks for m in range(images) for q in range(image_positions)]
        return [get(m, q, pk) for m in range(images) for pk in picks for q in range(image_positions)]

    def assemble(self, tiles, batch, n_rows, out_h, out_w):
        out = [None] * (batch * n_rows * out_h * out_w) if tiles else []
        for (m0, m1, y0, y1), rows in tiles:
            it = iter(rows)
            for m in range(m0, m1):
                for o in range(n_rows):
                    for y in range(y0, y1):
                        for x in range(out_w):
                            at = ((m * n_rows + o) * out_h + y) * out_w + x
                            assert out[at] is None                 # every output is written exactly once
                            out[at] = next(it)
            assert next(it, None) is None
        assert None not in out
        return out


class FakeEngine:
    """The engine surface homomorphic.conv2d uses, with the planner in front of a backend over ints."""

    def __init__(self, backend=None, budget=mp.TABLE_BUDGET_BYTES, **shape):
        self.backend, self.shape, self.budget, self.calls = backend, shape_fn(**shape), budget, []

    def ciphertext_conv2d_batch(self, x, weights, n, bias=None, stride=1, padding=0, dilation=1, fixed_base=None):
        self.calls.append(fixed_base)
        shape, flat = _grid_shape(x)
        self.plan = plan = cp.plan_conv(weights, shape, n, bias, self.shape, stride=stride, padding=padding, dilation=dilation,
                                        table_budget=self.budget)
        self.be = be = self.backend or PyConvBackend(n)
        vals = cp.execute_conv(plan, be, [int(c) % (n * n) for c in flat])
        o, oh, ow = plan.n_rows, plan.out_h, plan.out_w
        return [[[vals[((b * o + j) * oh + y) * ow : ((b * o + j) * oh + y + 1) * ow] for y in range(oh)] for j in range(o)]
                for b in range(shape[0])]


def oracle(x, w, n, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1)):
    """The definition, term by term, through pow."""
    n2 = n * n
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    c, h, wd = len(x[0]), len(x[0][0]), len(x[0][0][0])
    kh, kw = len(w[0][0]), len(w[0][0][0])
    oh, ow = cp.output_hw(h, wd, kh, kw, stride, padding, dilation)
    out = []
    for img in x:
        ys = []
        for o, ker in enumerate(w):
            plane = []
            for y in range(oh):
                line = []
                for xx in range(ow):
                    acc = (1 + (bias[o] % n) * n) % n2 if bias is not None else 1
                    for ch, i, j in itertools.product(range(c), range(kh), range(kw)):
                        yy, xc = y * sh - ph + i * dh, xx * sw - pw + j * dw
                        if 0 <= yy < h and 0 <= xc < wd and ker[ch][i][j]:
                            e = ker[ch][i][j]
                            base = img[ch][yy][xc] if e > 0 else pow(img[ch][yy][xc], -1, n2)
                            acc = acc * hostpow.powmod(base % n2, abs(e), n2) % n2
                    line.append(acc)
                plane.append(line)
            ys.append(plane)
        out.append(ys)
    return out


def unit(rng):
    while True:
        v = rng.randrange(1, N2)
        if v % ((1 << 127) - 1) and v % ((1 << 61) - 1):
            return v


def grid(rng, b, c, h, w):
    return [[[[unit(rng) for _ in range(w)] for _ in range(h)] for _ in range(c)] for _ in range(b)]


SPECIAL = (0, 1, -1, (1 << 63) + 5, -((1 << 64) - 3), (1 << 200) + 7, 1 << 63, -(1 << 63))


def kernel(rng, o, c, kh, kw, special=True):
    pick = lambda: rng.choice(SPECIAL) if special and rng.random() < 0.2 else rng.randrange(-4096, 4096)
    return [[[[pick() for _ in range(kw)] for _ in range(kh)] for _ in range(c)] for _ in range(o)]


# (B, C, H, W, O, kh, kw, stride, padding, dilation)
CASES = [(2, 2, 5, 6, 3, 3, 2, (1, 1), (0, 0), (1, 1)),
         (1, 3, 4, 7, 2, 2, 3, (2, 1), (1, 2), (1, 2)),
         (3, 1, 6, 5, 4, 3, 3, (2, 2), (1, 1), (1, 1)),
         (2, 1, 1, 9, 2, 1, 3, (1, 2), (0, 0), (1, 1)),
         (1, 2, 3, 3, 1, 1, 1, (1, 1), (0, 0), (1, 1)),
         (2, 2, 3, 4, 2, 5, 8, (1, 1), (1, 2), (1, 1))]            # a kernel as large as the padded grid: one position


@functools.lru_cache(maxsize=None)
def case(k):
    b, c, h, w, o, kh, kw, stride, padding, dilation = CASES[k]
    rng = random.Random(2000 + k)
    x = grid(rng, b, c, h, w)
    ker = kernel(rng, o, c, kh, kw)
    bias = [None, [-rng.randrange(1, 1 << 70) for _ in range(o)], [N * 3 + rng.randrange(N) for _ in range(o)]][k % 3]
    if bias is not None and o > 1:
        bias[1] = 0                                               # a kernel without a bias among kernels with one
    return x, ker, bias, oracle(x, ker, N, bias, stride, padding, dilation)


@pytest.mark.parametrize("k", range(len(CASES)))
@pytest.mark.parametrize("mode", ["plain", "chunk4", "bands"])
def test_planner_matches_pow(k, mode):
    x, ker, bias, want = case(k)
    b, c, h, w, o, kh, kw, stride, padding, dilation = CASES[k]
    kw_args = dict(n=N, bias=bias, stride=stride, padding=padding, dilation=dilation)
    if mode == "plain":
        eng = FakeEngine()
        got = H.conv2d(x, ker, engine=eng, **kw_args)
        assert not eng.plan.combine and len(eng.plan.tiles()) == 1
    elif mode == "chunk4":
        eng = FakeEngine(chunk=4)
        got = H.conv2d(x, ker, engine=eng, **kw_args)
        longest = max(sum(1 for ch in kr for r in ch for v in r if v) + (bias is not None and bias[j] % N != 0) for j, kr in enumerate(ker))
        assert all(l.index.shape[1] <= 4 for l in eng.plan.launches)
        if longest > 4:
            assert eng.plan.combine and eng.be.launches                      # the second pass ran, on run_matmul
            assert all(lch[5] == 1 and lch[2] == 0 for lch in eng.be.launches)
    else:
        free = cp.plan_conv(ker, (b, c, h, w), N, bias, shape_fn(), stride=stride, padding=padding, dilation=dilation)
        per_row = free.n_grids * free.padded_w
        rows = free.rows_in(2) if free.out_h > 2 else free.rows_in(1)         # a budget for a band of two output rows
        budget = (rows * per_row + len(free.bias)) * (ENTRY_BYTES << 3) + 100
        eng = FakeEngine(budget=budget)
        got = H.conv2d(x, ker, engine=eng, **kw_args)
        if free.out_h > 2:
            assert eng.plan.band_rows == 2 and eng.plan.tile_images == 1
            assert len(eng.plan.tiles()) == b * -(-free.out_h // 2)
    assert got == want
    assert all(0 <= v < N2 for img in got for pl in img for r in pl for v in r)


def plain_ct(m):
    return (1 + (m % N) * N) % N2                                  # g = N + 1, r = 1


def centred(y):
    assert (y - 1) % N == 0
    v = (y - 1) // N
    return v - N if v > N // 2 else v


GEOMETRY = [(st, pd, dl, kn) for st in (1, 2, (2, 1)) for pd in (0, 1, (1, 2)) for dl in (1, (1, 2)) for kn in ("1x1", "3x2", "full")]


@pytest.mark.parametrize("stride,padding,dilation,kind", GEOMETRY)
def test_geometry_against_torch_conv2d(stride, padding, dilation, kind):
    torch = pytest.importorskip("torch")
    rng = random.Random(f"geometry {stride} {padding} {dilation} {kind}")
    b, c, h, w, o = 2, 2, 5, 6, 2
    ph, pw = cp._pair(padding, "padding", 0)
    dh, dw = cp._pair(dilation, "dilation", 1)
    kh, kw = {"1x1": (1, 1), "3x2": (3, 2), "full": ((h + 2 * ph - 1) // dh + 1, (w + 2 * pw - 1) // dw + 1)}[kind]
    m = [[[[rng.randrange(-50, 50) for _ in range(w)] for _ in range(h)] for _ in range(c)] for _ in range(b)]
    ker = [[[[rng.randrange(-9, 10) for _ in range(kw)] for _ in range(kh)] for _ in range(c)] for _ in range(o)]
    bias = [rng.randrange(-100, 100) for _ in range(o)]
    want = torch.nn.functional.conv2d(torch.tensor(m, dtype=torch.int64), torch.tensor(ker, dtype=torch.int64),
                                      torch.tensor(bias, dtype=torch.int64), stride=stride, padding=padding, dilation=dilation)
    x = [[[[plain_ct(v) for v in r] for r in ch] for ch in img] for img in m]
    got = H.conv2d(x, ker, n=N, bias=bias, stride=stride, padding=padding, dilation=dilation, engine=FakeEngine())
    assert [[[[centred(v) for v in r] for r in pl] for pl in img] for img in got] == want.tolist()
    if kind == "full" and stride == 1:
        assert want.shape[2:] == (1 + (h + 2 * ph - 1) % dh, 1 + (w + 2 * pw - 1) % dw)


@pytest.mark.parametrize("stride,padding,dilation", [(1, 0, 1), (2, 1, 1), (2, 2, 2), (3, 0, 2)])
def test_conv1d_against_torch_conv1d(stride, padding, dilation):
    torch = pytest.importorskip("torch")
    rng = random.Random(f"conv1d {stride} {padding} {dilation}")
    m = [[[rng.randrange(-50, 50) for _ in range(9)] for _ in range(2)] for _ in range(3)]
    ker = [[[rng.randrange(-9, 10) for _ in range(3)] for _ in range(2)] for _ in range(2)]
    want = torch.nn.functional.conv1d(torch.tensor(m, dtype=torch.int64), torch.tensor(ker, dtype=torch.int64), None,
                                      stride=stride, padding=padding, dilation=dilation)
    x = [[[plain_ct(v) for v in ch] for ch in series] for series in m]
    got = H.conv1d(x, ker, n=N, stride=stride, padding=padding, dilation=dilation, engine=FakeEngine())
    assert [[[centred(v) for v in ch] for ch in series] for series in got] == want.tolist()


def _terms_of(plan):
    out = {}
    for launch in plan.launches:
        r, t = launch.index.shape
        w = launch.weights.reshape(r, t, -1)
        for k, rid in enumerate(launch.rows):
            terms = [(int(launch.index[k, c]), int.from_bytes(w[k, c].astype("<u4").tobytes(), "little")) for c in range(t)]
            assert rid not in out
            out[rid] = [(i, e) for i, e in terms if e]
    return out


def test_planner_properties():
    rng = random.Random(9)
    c, kh, kw = 3, 2, 2
    ker = kernel(rng, 3, c, kh, kw, special=False)
    for o in range(3):
        for i in range(kh):
            for j in range(kw):
                ker[o][1][i][j] = abs(ker[o][1][i][j]) or 1          # channel 1: positive taps only
                ker[o][2][i][j] = -abs(ker[o][2][i][j]) or -1        # channel 2: negative taps only
    ker[0][0][0][0], ker[0][0][1][1] = 5, -7                         # channel 0: both signs
    ker[1][0][0][1] = 0                                              # a zero tap
    ker[2] = [[[0] * kw for _ in range(kh)] for _ in range(c)]       # an all-zero kernel with a bias
    plans = {b: cp.plan_conv(ker, (b, c, 5, 6), N, [0, N + 2, 3], shape_fn(), padding=1) for b in (1, 4, 1000)}
    plan = plans[4]
    assert plan.x_ch == [0, 1] and plan.inverted == [0, 2] and plan.n_grids == 4        # no inverse grid for channel 1
    assert plan.bias == {1: 2, 2: 3}
    terms = _terms_of(plan)
    nonzero = lambda o: sum(1 for ch in ker[o] for r in ch for v in r if v)
    assert [len(terms[plan.result[o][1]]) for o in range(3)] == [nonzero(0), nonzero(1) + 1, 1]       # zero taps: no terms
    assert nonzero(1) == c * kh * kw - 1
    # the table of a tap at position 0: (i dh G + grid) Wp + j dw, and the bias tables behind the tile's own
    grid_of = {(0, 1): 0, (1, 1): 1, (0, -1): 2, (2, -1): 3}
    want = sorted(((i * 4 + grid_of[(ch, 1 if ker[0][ch][i][j] > 0 else -1)]) * 8 + j, abs(ker[0][ch][i][j]))
                  for ch in range(c) for i in range(kh) for j in range(kw) if ker[0][ch][i][j])
    assert sorted(terms[plan.result[0][1]]) == want
    assert terms[plan.result[2][1]] == [(-2, 1)]
    # one plan per call whatever the batch: the same launch arrays
    lead = lambda p: [(l.index.tolist(), l.weights.tolist()) for l in p.launches]
    assert lead(plans[1]) == lead(plans[4]) == lead(plans[1000])
    assert plan.tile_images == 4 and plan.band_rows == plan.out_h == 6 and plan.out_w == 7
    assert len(plan.origin) == 4 * 6 * 7 and plan.origin.dtype == np.int64
    assert int(plan.origin[7]) == 4 * 8 and int(plan.origin[6 * 7]) == plan.rows_in(6) * 4 * 8        # a row down; an image on
    for l in plan.launches:
        assert l.weights.shape[:2] == l.index.shape and l.index.dtype == np.int32 and l.weights.dtype == np.uint32


def test_bands_cover_every_output_row_once_with_a_ragged_last_band():
    rng = random.Random(13)
    x = grid(rng, 2, 2, 9, 4)
    ker = kernel(rng, 2, 2, 3, 2, special=False)
    free = cp.plan_conv(ker, (2, 2, 9, 4), N, [1, 2], shape_fn())
    assert free.out_h == 7 and len(free.tiles()) == 1
    per_row = free.n_grids * free.padded_w
    budget = (free.rows_in(3) * per_row + 2) * (ENTRY_BYTES << 3)             # exactly a band of three output rows
    eng = FakeEngine(budget=budget)
    got = H.conv2d(x, ker, n=N, bias=[1, 2], engine=eng)
    plan = eng.plan
    assert plan.band_rows == 3 and plan.tiles() == [(m, m + 1, y, min(7, y + 3)) for m in (0, 1) for y in (0, 3, 6)]
    assert [lch[5] for lch in eng.be.conv_launches if lch[0]] == [3 * 3, 3 * 3, 1 * 3] * 2          # the last band is ragged
    # the halo rows are tabled again by the next band: rows_in(3) + rows_in(3) + rows_in(1) input rows per image
    assert eng.be.tabled == 2 * ((5 + 5 + 3) * per_row + 3 * 2)
    assert got == oracle(x, ker, N, [1, 2])
    # one table less and the band shrinks; below one output row's band: refused before the backend is touched
    assert cp.plan_conv(ker, (2, 2, 9, 4), N, [1, 2], shape_fn(), table_budget=budget - 1).band_rows == 2
    small = (free.rows_in(1) * per_row + 2) * (ENTRY_BYTES << 1) - 1
    with pytest.raises(ValueError):
        H.conv2d(x, ker, n=N, bias=[1, 2], engine=FakeEngine(backend=tm.Untouchable(), budget=small, window=1))
    # without a forced window the planner first lowers the window, then refuses
    with pytest.raises(ValueError):
        cp.plan_conv(ker, (2, 2, 9, 4), N, [1, 2], shape_fn(), table_budget=(free.rows_in(1) * per_row + 2) * (ENTRY_BYTES << 1) - 1)
    lowered = cp.plan_conv(ker, (2, 2, 9, 4), N, [1, 2], shape_fn(), table_budget=(free.rows_in(1) * per_row + 2) * (ENTRY_BYTES << 2))
    assert lowered.window == 2 and lowered.band_rows == 1


def test_whole_images_per_tile_with_a_ragged_last_tile():
    rng = random.Random(15)
    x = grid(rng, 5, 1, 3, 4)
    ker = kernel(rng, 2, 1, 2, 2, special=False)
    free = cp.plan_conv(ker, (5, 1, 3, 4), N, None, shape_fn())
    budget = 2 * free.n_local(1, free.out_h) * (ENTRY_BYTES << 3) + 100
    eng = FakeEngine(budget=budget)
    got = H.conv2d(x, ker, n=N, engine=eng)
    assert eng.plan.tile_images == 2 and eng.plan.tiles() == [(0, 2, 0, 2), (2, 4, 0, 2), (4, 5, 0, 2)]
    assert got == oracle(x, ker, N)


def test_split_k_pieces_recombine():
    rng = random.Random(17)
    x = grid(rng, 2, 3, 4, 4)
    ker = kernel(rng, 2, 3, 3, 3)
    ker[1] = [[[0] * 3 for _ in range(3)] for _ in range(3)]
    ker[1][2][1][1] = -3                                               # a short kernel beside a split one
    eng = FakeEngine(chunk=5)
    got = H.conv2d(x, ker, n=N, bias=[7, 0], padding=1, engine=eng)
    plan = eng.plan
    terms = _terms_of(plan)
    assert plan.result[0][0] == "p2" and plan.result[1][0] == "p1"
    assert sorted(plan.part_rows) == sorted(set(range(plan.pass1_rows)) - {plan.result[1][1]})
    assert all(len(ts) <= 5 for ts in terms.values())
    assert sum(len(terms[m]) for m in plan.part_rows) == sum(1 for ch in ker[0] for r in ch for v in r if v) + 1
    assert got == oracle(x, ker, N, [7, 0], padding=(1, 1))


def test_edge_shapes():
    eng = FakeEngine()
    assert H.conv2d([], [[[[1]]]], n=N, engine=eng) == [] == H.conv2d([], [[[[1, 2], [3, 4]]]], n=N, bias=[1], engine=eng)     # B = 0
    x = [[[[3, 5], [7, 9]]]]
    assert H.conv2d(x, [], n=N, engine=eng) == [[]]                                              # O = 0
    assert H.conv2d([[], []], [[], []], n=N, bias=[5, 0], engine=eng) == [[[[1 + 5 * N]], [[1]]]] * 2      # C = 0: the bias only
    assert H.conv2d([[[[0, 7]]]], [[[[0, 2]]], [[[1, 1]]]], n=N, engine=eng) == [[[[49]], [[0]]]]  # a zero tap on a zero input gives 1
    assert H.conv1d([[[2, 3, 5, 7]]], [[[1, 0, 2]]], n=N, engine=eng) == [[[2 * 25, 3 * 49]]]


def test_every_refusal_raises_before_the_backend_is_touched():
    eng = FakeEngine(backend=tm.Untouchable())
    good = [[[[3, 5, 7], [9, 11, 13]]]]                                # 1 x 1 x 2 x 3
    k22 = [[[[1, 2], [3, 4]]]]
    bound = mp.weight_bound(N)
    with pytest.raises(ValueError):
        H.conv2d([[[[3, 5, 7], [9, 11]]]], k22, n=N, engine=eng)                                 # a ragged grid
    with pytest.raises(ValueError):
        H.conv2d([[[[3, 5], [9, 11]]], [[[3, 5], [9, 11]], [[3, 5], [9, 11]]]], k22, n=N, engine=eng)     # grids of different channel counts
    for weights, kw in (([[[1, 2], [3, 4]]], {}),                                                # rank 3
                        ([[[[1, 2], [3, 4]]] * 2], {}),                                          # two channels for one
                        ([[[[1, 2], [3]]]], {}),                                                 # a ragged kernel
                        ([[[[1, 2], [3, 4], [5, 6]]]], {}),                                      # larger than the grid
                        ([[[[1, 2, 3, 4]]]], {}),
                        ([[[[1, 2], [3, 4], [5, 6], [7, 8]]]], dict(padding=(0, 5))),            # larger than the padded grid
                        (k22, dict(dilation=(2, 1))),                                            # its span is
                        (k22, dict(stride=0)), (k22, dict(stride=(1, 0))), (k22, dict(dilation=0)), (k22, dict(dilation=(1, -1))),
                        (k22, dict(padding=-1)), (k22, dict(padding=(0, -1))), (k22, dict(stride=(1, 1, 1))),
                        (k22, dict(bias=[1, 2])), (k22, dict(bias=[])),                          # a bias of the wrong length
                        ([[[[1, bound], [3, 4]]]], {}), ([[[[1, -bound], [3, 4]]]], {})):        # a weight out of bounds
        with pytest.raises(ValueError):
            H.conv2d(good, weights, n=N, engine=eng, **kw)
    assert H.conv2d(good, [[[[1, bound - 1], [1 - bound, 0]]]], n=N, engine=FakeEngine()) == oracle(good, [[[[1, bound - 1], [1 - bound, 0]]]], N)
    with pytest.raises(ValueError):
        H.conv2d(good, k22, engine=eng)                                                          # plain ints need n
    # a negative tap on a non-invertible input: ValueError as pow (this one comes from the backend's inversion)
    with pytest.raises(ValueError):
        H.conv2d([[[[3, N]]]], [[[[1, -1]]]], n=N, engine=FakeEngine())
    assert H.conv2d([[[[3, N]]]], [[[[1, 1]]]], n=N, engine=FakeEngine()) == [[[[3 * N]]]]


def test_get_value_is_called_once_per_object_and_the_randomiser_covers_every_output():
    rng = random.Random(5)
    a, b, c = (tm.Ct(unit(rng)) for _ in range(3))
    eng = FakeEngine()

    class Rz:
        def spec(self, n, count):
            return ("spec", n, count)

    x = [[[[a, b, a], [c, c, b]]], [[[b, b, b], [a, c, a]]]]
    ker = [[[[1, -2]]], [[[0, 5]]], [[[3, 3]]]]
    got = H.conv2d(x, ker, bias=[1, 2, 3], padding=(0, 1), engine=eng, randomizer=Rz())
    assert (a.reads, b.reads, c.reads) == (1, 1, 1)
    vals = [[[[v.v for v in r] for r in ch] for ch in img] for img in x]
    assert got == oracle(vals, ker, N, [1, 2, 3], padding=(0, 1))
    assert eng.calls[-1] == ("spec", N, 2 * 3 * 2 * 4)                  # B * O * H' * W' outputs


def test_abi_refuses_bad_arguments_without_a_launch():
    """The new entry points validate before they touch the runtime: on a machine without a GPU."""
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    assert lib.mx_version() == 404
    assert lib.mx_conv_nsquare_workspace_bytes(2048, 12, 1, 0, 4) == lib.mx_multiexp_nsquare_workspace_bytes(2048, 13, 0, 4) > 0
    assert lib.mx_conv_nsquare_workspace_bytes(2048, 0, 3, 0, 4) == lib.mx_multiexp_nsquare_workspace_bytes(2048, 3, 0, 4)
    for bad in ((2048, -1, 1, 0, 4), (2048, 4, -1, 0, 4), (2048, 0, 0, 0, 4), (2048, 4, 1, 0, 0), (2048, 4, 1, 0, 9),
                (2048, (1 << 36) + 1, 0, 0, 1), (2048, 4, (1 << 31) + 1, 0, 1)):
        assert lib.mx_conv_nsquare_workspace_bytes(*bad) == -1, bad
    assert lib.mx_conv_nsquare_workspace_bytes(20000, 4, 1, 0, 4) == -2
    assert lib.mx_conv_nsquare_workspace_bytes(2048, 4, 1, 18, 4) == -2
    assert lib.mx_conv_nsquare_workspace_bytes(2048, 1 << 36, 0, 0, 1) == -2                   # more tables than one grid of the table pass
    lanes, lpl = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    count = lib.mx_conv_nsquare_instances(lanes, lpl, 8)
    assert [(lanes[i], lpl[i]) for i in range(count)] == [(kk, 9) for kk in (1, 2, 4, 8, 16, 32)]
    assert lib.mx_conv_nsquare_instances(None, None, 4) == -1
    # the run: a descriptor that names device memory which is never read, because every call below is refused first
    buf = (ctypes.c_uint32 * 64)()
    ptr = ctypes.addressof(buf)
    plan = _lib.NsquarePlan(d_plan=ptr, plan_bytes=256, limbs_n=64, n_bits=2048, geometries=1)
    ok = dict(plan=plan, inputs=ptr, n_local=12, n_shared=1, limbs2=128, index=ptr, weights=ptr, terms=5, bits=16, origin=ptr,
              positions=6, ipos=3, out=ptr, rows=2, lpl=0, window=4, ws=ptr, ws_bytes=1 << 40)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mx_conv_nsquare_run(a["plan"], a["inputs"], a["n_local"], a["n_shared"], a["limbs2"], a["index"], a["weights"],
                                       a["terms"], a["bits"], a["origin"], a["positions"], a["ipos"], a["out"], a["rows"], a["lpl"],
                                       a["window"], a["ws"], a["ws_bytes"], None)

    for kw in (dict(plan=None), dict(out=None), dict(ws=None), dict(index=None), dict(weights=None), dict(origin=None),
               dict(n_local=-1), dict(n_shared=-1), dict(n_local=0, n_shared=0), dict(positions=0), dict(positions=(1 << 30) + 3),
               dict(ipos=0), dict(ipos=4), dict(ipos=-3), dict(rows=0), dict(limbs2=0), dict(terms=-1), dict(bits=-1), dict(window=0),
               dict(window=9), dict(lpl=18), dict(bits=2 * 2048 + 65), dict(limbs2=127),
               dict(plan=_lib.NsquarePlan(d_plan=None, limbs_n=64, n_bits=2048, geometries=1))):
        assert call(**kw) == -1, kw
    assert call(plan=_lib.NsquarePlan(d_plan=ptr, limbs_n=64, n_bits=2048, geometries=0)) == -2      # a plan without the narrow constants
    assert call(plan=_lib.NsquarePlan(d_plan=ptr, limbs_n=625, n_bits=20000, geometries=1), limbs2=1250) == -2
    assert call(rows=1 << 40) == -2                                                          # beyond one grid
    assert call(n_local=1 << 36) == -2
    assert call(ws_bytes=1024) == -4
