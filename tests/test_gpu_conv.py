"""Encrypted convolutions of ciphertext grids with a public kernel on the GPU (csrc/mx_conv_n2.hpp,
Engine.conv2d_nsquare_t, homomorphic.conv2d / conv1d), bit-exact against pow and against the single-vector linear map on
the explicit Toeplitz rows."""

from __future__ import annotations

import ctypes
import itertools
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
    """Residues modulo n^2 that are coprime to n (a negative tap inverts them)."""
    out = []
    while len(out) < count:
        v = rng.randrange(1, n * n)
        if math.gcd(v, n) == 1:
            out.append(v)
    return out


def grid(rng, n, b, c, h, w):
    it = iter(units(rng, n, b * c * h * w))
    return [[[[next(it) for _ in range(w)] for _ in range(h)] for _ in range(c)] for _ in range(b)]


def pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def taps_of(x, w, stride=1, padding=0, dilation=1):
    """Per image, per output (o, y, x) in row-major order: [(flat input index c H W, weight)] of the taps inside the grid
    with a non-zero weight — the explicit Toeplitz rows of the convolution."""
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(padding), pair(dilation)
    c, h, wd = len(x[0]), len(x[0][0]), len(x[0][0][0])
    kh, kw = len(w[0][0]), len(w[0][0][0])
    oh, ow = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (wd + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    rows = []
    for ker in w:
        for y in range(oh):
            for xx in range(ow):
                row = []
                for ch, i, j in itertools.product(range(c), range(kh), range(kw)):
                    yy, xc = y * sh - ph + i * dh, xx * sw - pw + j * dw
                    if 0 <= yy < h and 0 <= xc < wd and ker[ch][i][j]:
                        row.append(((ch * h + yy) * wd + xc, ker[ch][i][j]))
                rows.append(row)
    return rows, (len(w), oh, ow)


def flat_of(img):
    return [v for ch in img for r in ch for v in r]


def want_conv(x, w, n, bias=None, **geometry):
    """[B][O][H'][W'] of the definition through hostpow (inverses for the negative taps)."""
    n2 = n * n
    rows, (o, oh, ow) = taps_of(x, w, **geometry)
    jobs = []
    for img in x:
        flat = flat_of(img)
        for row in rows:
            jobs += [(flat[i] % n2 if wt > 0 else pow(flat[i], -1, n2), abs(wt), n2) for i, wt in row]
    powers = iter(hostpow.powmod_many(jobs))
    out = []
    for img in x:
        vals = []
        for k, row in enumerate(rows):
            acc = (1 + (bias[k // (oh * ow)] % n) * n) % n2 if bias is not None else 1
            for _ in row:
                acc = acc * next(powers) % n2
            vals.append(acc)
        out.append([[vals[(j * oh + y) * ow : (j * oh + y + 1) * ow] for y in range(oh)] for j in range(o)])
    return out


def toeplitz_map(eng, x, w, n, bias=None, **geometry):
    """The same through ciphertext_linear_map_batch: one sparse map per image."""
    rows, (o, oh, ow) = taps_of(x, w, **geometry)
    row_bias = [bias[k // (oh * ow)] for k in range(len(rows))] if bias is not None else None
    out = []
    for img in x:
        vals = eng.ciphertext_linear_map_batch(flat_of(img), [dict(r) for r in rows], n, bias=row_bias)
        out.append([[vals[(j * oh + y) * ow : (j * oh + y + 1) * ow] for y in range(oh)] for j in range(o)])
    return out


def nest(vals, b, o, oh, ow):
    return [[[vals[((m * o + j) * oh + y) * ow : ((m * o + j) * oh + y + 1) * ow] for y in range(oh)] for j in range(o)] for m in range(b)]


def run_t(eng, x, w, n, **kw):
    """conv2d_nsquare_t on uploaded rows, as nested ints."""
    from protocols.distributed_keygen_amd import limbs

    n2 = n * n
    b, c, h, wd = len(x), len(x[0]), len(x[0][0]), len(x[0][0][0])
    x_t = eng.to_device(limbs.pack_reduced([v for img in x for v in flat_of(img)], limbs.limbs_for(n2), n2))
    vals = limbs.unpack(eng.to_host(eng.conv2d_nsquare_t(x_t, (b, c, h, wd), w, n, **kw)))
    geometry = {k: v for k, v in kw.items() if k in ("stride", "padding", "dilation")}
    _, (o, oh, ow) = taps_of(x, w, **geometry)
    return nest(vals, b, o, oh, ow)


@pytest.mark.parametrize("key_length", [128, 2048, "odd"])
def test_matches_pow_and_the_toeplitz_linear_map(eng, key_length):
    rng = random.Random(f"conv {key_length}")
    n = key_n(key_length) if key_length != "odd" else odd_modulus(1531, rng)
    n2 = n * n
    if key_length == 2048:
        x = grid(rng, n, 1, 1, 4, 4)                                  # 9 positions: hostpow stays in seconds
        w = [[[[rng.randrange(-(1 << 63), 1 << 63), (1 << 64) - 1], [-(1 << 64), 0]]],
             [[[1, -1], [rng.randrange(n2), -rng.randrange(n2)]]],
             [[[rng.randrange(-1000, 1000) for _ in range(2)] for _ in range(2)]]]
    else:
        x = grid(rng, n, 2, 2, 5, 6)                                  # 15 positions per image, 30 per call: no multiple of 64 / K
        i64 = lambda: rng.randrange(-(1 << 63), 1 << 63)
        w = [[[[i64(), i64()], [(1 << 63) - 1, -(1 << 63)], [i64(), i64()]], [[i64(), i64()], [i64(), i64()], [i64(), i64()]]],
             [[[0, 1], [-1, (1 << 64) - 1], [-(1 << 64), rng.randrange(n2)]], [[-rng.randrange(n2), 0], [1, -1], [0, 0]]],
             [[[rng.randrange(-1000, 1000) for _ in range(2)] for _ in range(3)] for _ in range(2)]]
    bias = [rng.randrange(n), -5, n + 7]
    got = eng.ciphertext_conv2d_batch(x, w, n, bias=bias)
    assert got == want_conv(x, w, n, bias)
    assert got == toeplitz_map(eng, x, w, n, bias)
    assert eng.ciphertext_conv2d_batch(x, w, n) == toeplitz_map(eng, x, w, n)


def test_stride_padding_and_dilation(eng):
    from protocols.distributed_keygen_amd import homomorphic

    rng = random.Random("conv geometry")
    n = key_n(128)
    x = grid(rng, n, 2, 2, 7, 8)
    w = [[[[rng.randrange(-(1 << 15), 1 << 15) for _ in range(2)] for _ in range(3)] for _ in range(2)] for _ in range(2)]
    geometry = dict(stride=(2, 1), padding=(1, 2), dilation=(1, 2))
    got = eng.ciphertext_conv2d_batch(x, w, n, bias=[3, -4], **geometry)
    assert [len(got), len(got[0]), len(got[0][0]), len(got[0][0][0])] == [2, 2, 4, 10]
    assert got == want_conv(x, w, n, [3, -4], **geometry)
    # conv1d: a series of 9 under 3 taps with stride 2
    series = [[units(rng, n, 9)] for _ in range(2)]
    taps = [[[rng.randrange(-(1 << 15), 1 << 15) for _ in range(3)]], [[5, 0, -1]]]
    got1 = homomorphic.conv1d(series, taps, n=n, bias=[0, 9], stride=2, engine=eng)
    want1 = want_conv([[[ch] for ch in s] for s in series], [[[t] for t in ker] for ker in taps], n, [0, 9], stride=(1, 2))
    assert got1 == [[pl[0] for pl in img] for img in want1] and len(got1[0][0]) == 4


@pytest.mark.parametrize("window", [1, 4])
@pytest.mark.parametrize("out_hw", [(5, 8), (8, 9)])
def test_ragged_wavefronts_and_zero_digits_match_pow(eng, window, out_hw):
    """Values only (that zero digits are skipped is a matter of time: tools/conv_probe.py): an all-zero kernel, a kernel
    of signed powers of two (most digits zero) and a dense random kernel.  key_length 128 runs groups of one lane, 64
    positions per wavefront: 40 positions leave every wavefront ragged (3 x 40 outputs would put two kernels into one
    wavefront if the positions of a kernel were not padded), 72 give a full and a ragged wavefront per kernel."""
    rng = random.Random(f"conv vote {window} {out_hw}")
    n = key_n(128)
    oh, ow = out_hw
    x = grid(rng, n, 1, 1, oh + 1, ow + 1)
    w = [[[[0, 0], [0, 0]]],
         [[[1 << rng.randrange(16), -(1 << rng.randrange(16))], [-(1 << 15), 1 << rng.randrange(16)]]],
         [[[rng.randrange(-(1 << 15), 1 << 15) for _ in range(2)] for _ in range(2)]]]
    plan = eng._conv_plan(n, (1, 1, oh + 1, ow + 1), w, [0, 3, 0], 1, 0, 1, window)
    assert len(plan.tiles()) == 1 and plan.out_h * plan.out_w == oh * ow            # one tile
    assert run_t(eng, x, w, n, bias=[0, 3, 0], window=window) == want_conv(x, w, n, [0, 3, 0])


def test_every_instance_has_a_parity_case(eng):
    from protocols.distributed_keygen_amd import limbs

    lib = eng.lib
    cnt = lib.mx_conv_nsquare_instances(None, None, 0)
    lanes, lpls = (ctypes.c_int * cnt)(), (ctypes.c_int * cnt)()
    assert lib.mx_conv_nsquare_instances(lanes, lpls, cnt) == cnt
    want = {(lanes[i], lpls[i]) for i in range(cnt)}
    rng = random.Random(19)
    seen = set()
    for bits in (130, 200, 400, 900, 2000, 3000, 4000, 6000, 8000):
        n = odd_modulus(bits, rng)
        n2 = n * n
        k, l, w_out, ch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        assert lib.mx_multiexp_nsquare_shape(bits, 6, 8, 3, 70, 0, 0, k, l, w_out, ch) == 0
        seen.add((k.value, l.value))
        series = [[rng.randrange(n2) for _ in range(5)] + [n2 + 3]]                   # C = 1, length 6
        taps = [[[rng.getrandbits(70) for _ in range(3)]], [[0, 1, 2]]]               # O = 2
        want_y = [v for pl in want_conv([[series]], [[[t] for t in ker] for ker in taps], n)[0] for v in pl[0]]
        x_t = eng.to_device(limbs.pack_reduced(series[0], limbs.limbs_for(n2), n2))
        for window in (0, 1, 8):
            got = limbs.unpack(eng.to_host(eng.conv2d_nsquare_t(x_t, (1, 1, 1, 6), [[[t] for t in ker] for ker in taps], n, window=window)))
            assert got == want_y, (bits, window)
    assert seen == want


def test_bands_and_split_k_on_the_device(eng):
    rng = random.Random(23)
    n = key_n(128)
    c = 15
    x = grid(rng, n, 1, c, 8, 8)
    w = [[[[rng.randrange(-(1 << 15), 1 << 15) or 1 for _ in range(3)] for _ in range(3)] for _ in range(c)]]
    want = want_conv(x, w, n, [5])
    free = eng._conv_plan(n, (1, c, 8, 8), w, [5], 1, 0, 1, table_budget=1 << 40)
    assert len(free.tiles()) == 1 and free.out_h == free.out_w == 6
    lanes = ctypes.c_int()
    assert eng.lib.mx_multiexp_nsquare_shape(n.bit_length(), 1, 1, 1, 1, 0, 0, lanes, ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()) == 0
    per_row = free.n_grids * free.padded_w                            # tables of one input row
    table_bytes = (2 * lanes.value * 9 * 4) << free.window
    # three input rows of tables: a band is one output row, six bands; 135 taps and a bias are split by the library's own rule
    budget = (3 * per_row + 1) * table_bytes
    plan = eng._conv_plan(n, (1, c, 8, 8), w, [5], 1, 0, 1, window=free.window, table_budget=budget)
    assert plan.band_rows == 1 and len(plan.tiles()) == 6 and plan.combine and len(plan.part_rows) >= 2
    assert run_t(eng, x, w, n, bias=[5], window=free.window, table_budget=budget) == want
    # six input rows: bands of four and of two output rows — the last band is ragged
    budget = (6 * per_row + 1) * table_bytes
    plan = eng._conv_plan(n, (1, c, 8, 8), w, [5], 1, 0, 1, window=free.window, table_budget=budget)
    assert plan.band_rows == 4 and plan.tiles() == [(0, 1, 0, 4), (0, 1, 4, 6)] and plan.combine
    assert run_t(eng, x, w, n, bias=[5], window=free.window, table_budget=budget) == want
    with pytest.raises(ValueError):
        eng._conv_plan(n, (1, c, 8, 8), w, [5], 1, 0, 1, window=free.window, table_budget=(3 * per_row + 1) * table_bytes - 1)


def test_refusals_and_empty_shapes(eng):
    n = key_n(128)
    with pytest.raises(ValueError):
        eng.ciphertext_conv2d_batch([[[[3, 5], [7, n]]]], [[[[1, -1]]]], n)          # a negative tap on a non-invertible input
    with pytest.raises(ValueError):
        eng.ciphertext_conv2d_batch([[[[3, 5], [7]]]], [[[[1, 1]]]], n)
    with pytest.raises(ValueError):
        eng.ciphertext_conv2d_batch([[[[3, 5]]]], [[[[1, 1, 1]]]], n)
    with pytest.raises(ValueError):
        eng.ciphertext_conv2d_batch([[[[3, 5]]]], [[[[1, 1]]]], n, bias=[1, 2])
    assert eng.ciphertext_conv2d_batch([], [[[[1, 1]]]], n) == []                     # B = 0
    assert eng.ciphertext_conv2d_batch([[[[3, 5]]], [[[7, 9]]]], [], n) == [[], []]    # O = 0
    assert eng.ciphertext_conv2d_batch([[], []], [[], []], n, bias=[4, 0]) == [[[[1 + 4 * n]], [[1]]]] * 2      # C = 0: the bias only
    assert eng.ciphertext_conv2d_batch([[[[0, 7]]]], [[[[0, 2]]], [[[1, 1]]]], n) == [[[[49]], [[0]]]]         # a zero tap on a zero input gives 1


@pytest.fixture(scope="module")
def round_trip_case():
    from protocols.distributed_keygen_amd import synthetic

    rng = random.Random(29)
    key = synthetic.make_key(1024, 3, 1)
    m = [[[rng.randrange(key.n) for _ in range(6)] for _ in range(6)]]
    cts = [[[[synthetic.encrypt(key, v, rng) for v in r] for r in ch] for ch in [m[0]]]]
    w = [[[[rng.randrange(-(1 << 63), 1 << 63) for _ in range(3)] for _ in range(3)]] for _ in range(2)]
    b = [rng.randrange(key.n) for _ in range(2)]
    want = []
    for o in range(2):
        for y in range(6):
            for xx in range(6):
                s = b[o]
                for i in range(3):
                    for j in range(3):
                        yy, xc = y - 1 + i, xx - 1 + j
                        if 0 <= yy < 6 and 0 <= xc < 6:
                            s += w[o][0][i][j] * m[0][yy][xc]
                want.append(s % key.n)
    return key, cts, w, b, want


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


def test_encrypted_convolution_round_trip(eng, round_trip_case):
    from protocols.distributed_keygen_amd import homomorphic
    from protocols.distributed_keygen_amd.randomizer import FastRandomizer, generate_base

    key, cts, w, b, want = round_trip_case
    rng = random.Random(31)
    plain = homomorphic.conv2d(cts, w, n=key.n, bias=b, padding=1, engine=eng)
    flat = [v for pl in plain[0] for r in pl for v in r]
    assert len(flat) == 72
    fresh = eng.randomize_batch(flat, [rng.randrange(1, key.n) for _ in flat], key.n)
    assert threshold_decrypt(eng, key, fresh) == want
    # the same with a FastRandomizer: the ciphertexts differ, the plaintexts do not
    fr = FastRandomizer(key.n, generate_base(key.n, rng=random.Random(37), engine=eng), engine=eng)
    fast = homomorphic.conv2d(cts, w, n=key.n, bias=b, padding=1, engine=eng, randomizer=fr)
    fast_flat = [v for pl in fast[0] for r in pl for v in r]
    assert len(fast_flat) == 72 and all(f != p for f, p in zip(fast_flat, flat))
    assert threshold_decrypt(eng, key, fast_flat) == want
