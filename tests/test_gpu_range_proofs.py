"""The kernels of the range proofs (csrc/mx_multiexp.hpp, csrc/mx_response.hpp) and the proofs over them on the GPU —
Engine.multiexp_mod_t / response_rows_t / range_prove_t / range_verify_t and range_proof.py — bit for bit against Python
pow (tests/hostpow.py for the wide moduli), Python ints and tools/range_model.py.

The statement needs l + 258 <= bits(N) - 1, so the smallest golden key that carries a proof is the 1024-bit one; the
row-by-row comparison runs there with the 128-bit auxiliary modulus of golden/range_params.json, the end-to-end cases
at N = 1024 with Nh = 2048 and at N = 2048 with Nh = 1024."""

from __future__ import annotations

import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

import hostpow  # noqa: E402
import range_cases as rc  # noqa: E402
from range_cases import rm  # noqa: E402
from range_engine import tamperings  # noqa: E402

N1K = rc.modulus(1024)
BITS = 64


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def rows_of(eng, values, width):
    from protocols.distributed_keygen_amd import limbs

    return eng.to_device(limbs.pack(values, width).reshape(len(values), width))


def ints_of(eng, rows_t):
    from protocols.distributed_keygen_amd import limbs

    return limbs.unpack(eng.to_host(rows_t))


# ------------------------------------------------------------------ the multi-exponentiation over a generic modulus
@pytest.mark.parametrize("name", [c[0] for c in rc.MULTIEXP_CASES])
def test_multiexp_mod_equals_pow(eng, name):
    import torch

    from protocols.distributed_keygen_amd import limbs

    mod, inputs, index, weights, terms, window, wbits, counts = rc.multiexp_case(name)
    width = limbs.limbs_for(mod)
    ww = (wbits + 31) // 32
    want = []
    for idx, ws in zip(index, weights):
        acc = 1
        for i, w in zip(idx, ws):
            acc = acc * hostpow.powmod(inputs[i], w, mod) % mod
        want.append(acc)
    assert want[0] == (1 if terms == 1 else want[0]) and inputs[0] == 0 and weights[0][0] == 0          # 0^0 = 1 is among the terms
    inputs_t = rows_of(eng, inputs, width)
    index_t = torch.tensor(index, dtype=torch.int32, device=eng.device)
    weights_t = rows_of(eng, [w for row in weights for w in row], ww).view(len(weights), terms * ww)
    for count in counts:
        got_t = eng.multiexp_mod_t(inputs_t, index_t[:count].contiguous(), weights_t[:count].contiguous(), terms, wbits, mod, window=window)
        assert tuple(got_t.shape) == (count, width)
        assert ints_of(eng, got_t) == want[:count], (name, count)
    # term lengths: the longest weight of every term over the rows (windows above it are skipped) — and a term of length 0
    count = max(counts)
    tb = [max(1, max(row[j].bit_length() for row in weights)) for j in range(terms)]
    got_t = eng.multiexp_mod_t(inputs_t, index_t, weights_t, terms, wbits, mod, window=window, term_bits=tb)
    assert ints_of(eng, got_t) == want, (name, tb)
    short = [[w if j == 0 else w & 1 for j, w in enumerate(row)] for row in weights]
    short_t = rows_of(eng, [w for row in short for w in row], ww).view(len(short), terms * ww)
    want_short = [1] * len(short)
    for r, (idx, ws) in enumerate(zip(index, short)):
        for i, w in zip(idx, ws):
            want_short[r] = want_short[r] * hostpow.powmod(inputs[i], w, mod) % mod
    got_t = eng.multiexp_mod_t(inputs_t, index_t, short_t, terms, wbits, mod, window=window, term_bits=[wbits] + [1] * (terms - 1))
    assert ints_of(eng, got_t) == want_short, name
    zeroed = [[w if j == 0 else 0 for j, w in enumerate(row)] for row in weights]
    zeroed_t = rows_of(eng, [w for row in zeroed for w in row], ww).view(len(zeroed), terms * ww)
    got_t = eng.multiexp_mod_t(inputs_t, index_t, zeroed_t, terms, wbits, mod, window=window, term_bits=[wbits] + [0] * (terms - 1))
    assert ints_of(eng, got_t) == [hostpow.powmod(inputs[idx[0]], row[0], mod) for idx, row in zip(index, zeroed)], name
    # the automatic window gives the same rows, and so does the int-level entry (per-row bases)
    count = min(counts)
    assert ints_of(eng, eng.multiexp_mod_t(inputs_t, index_t[:count].contiguous(), weights_t[:count].contiguous(), terms, wbits, mod)) == want[:count]
    assert eng.multiexp_mod_batch([[inputs[i] for i in idx] for idx in index[:count]], weights[:count], mod) == want[:count]


def test_multiexp_mod_refusals_launch_nothing(eng):
    import torch

    from protocols.distributed_keygen_amd import _lib

    mod = rc.modulus(128)
    inputs_t = rows_of(eng, [3, 5], 4)
    index_t = torch.tensor([[0, 1]], dtype=torch.int32, device=eng.device)
    weights_t = rows_of(eng, [7, 9], 1).view(1, 2)
    assert ints_of(eng, eng.multiexp_mod_t(inputs_t, index_t, weights_t, 2, 32, mod)) == [pow(3, 7, mod) * pow(5, 9, mod) % mod]
    for bad in (lambda: eng.multiexp_mod_t(inputs_t, index_t, weights_t, 2, 32, mod + 1),                       # even
                lambda: eng.multiexp_mod_t(inputs_t, index_t, weights_t, 2, 32, 1),
                lambda: eng.multiexp_mod_t(inputs_t[:, :3].contiguous(), index_t, weights_t, 2, 32, mod),       # rows narrower than M
                lambda: eng.multiexp_mod_t(inputs_t, index_t, weights_t, 2, 0, mod),
                lambda: eng.multiexp_mod_t(inputs_t, index_t, weights_t, 2, 16385, mod),
                lambda: eng.multiexp_mod_t(inputs_t, index_t, weights_t, 2, 33, mod),                           # two words per weight expected
                lambda: eng.multiexp_mod_t(inputs_t, index_t, weights_t, 1, 32, mod),
                lambda: eng.multiexp_mod_t(inputs_t, index_t, weights_t, 2, 32, mod, window=9),
                lambda: eng.multiexp_mod_t(inputs_t, index_t, weights_t, 2, 32, mod, term_bits=(32,)),
                lambda: eng.multiexp_mod_t(inputs_t, index_t, weights_t, 2, 32, mod, term_bits=(32, 33)),
                lambda: eng.multiexp_mod_t(inputs_t, index_t + 1, weights_t, 2, 32, mod),                       # index out of range
                lambda: eng.multiexp_mod_t(inputs_t, index_t.to(torch.int64), weights_t, 2, 32, mod),
                lambda: eng.multiexp_mod_batch([[3, 5]], [[7, -9]], mod),
                lambda: eng.multiexp_mod_batch([[3, 5], [3]], [[7, 9], [1]], mod)):
        with pytest.raises(ValueError):
            bad()
    assert tuple(eng.multiexp_mod_t(inputs_t, index_t[:0].contiguous(), weights_t[:0].contiguous(), 2, 32, mod).shape) == (0, 4)
    # the C entries themselves: bad arguments come back as a status, before anything is planned or launched
    lib = eng.lib
    h_mod = (ctypes.c_uint32 * 4)(*[(mod >> (32 * k)) & 0xFFFFFFFF for k in range(4)])
    h_even = (ctypes.c_uint32 * 4)(2, 0, 0, 1)
    h_one = (ctypes.c_uint32 * 4)(1, 0, 0, 0)
    out_t = torch.empty((1, 4), dtype=torch.int32, device=eng.device)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=eng.device)
    good = [ctypes.addressof(h_mod), 4, inputs_t.data_ptr(), 2, index_t.data_ptr(), weights_t.data_ptr(), 2, 32, None, out_t.data_ptr(), 1, 4,
            ws.data_ptr(), ws.numel(), None]
    too_long, negative = (ctypes.c_int32 * 2)(32, 33), (ctypes.c_int32 * 2)(-1, 4)

    def run(**change):
        names = ("h_mod", "limbs", "inputs", "n_inputs", "index", "weights", "terms", "weight_bits", "term_bits", "out", "n_outputs", "window", "ws", "ws_bytes", "stream")
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.mx_multiexp_run(*args)

    for change in (dict(h_mod=None), dict(inputs=None), dict(index=None), dict(weights=None), dict(out=None), dict(ws=None), dict(limbs=0),
                   dict(n_inputs=0), dict(n_outputs=0), dict(terms=0), dict(terms=65537), dict(weight_bits=0), dict(weight_bits=16385),
                   dict(window=0), dict(window=9), dict(n_inputs=1 << 31), dict(n_outputs=-1),
                   dict(term_bits=ctypes.addressof(too_long)), dict(term_bits=ctypes.addressof(negative))):
        assert run(**change) == -1, change
    assert run(h_mod=ctypes.addressof(h_even)) == -3 and run(h_mod=ctypes.addressof(h_one)) == -3
    assert run(ws_bytes=64) == -4
    wide = (ctypes.c_uint32 * 523)(*([1] + [0] * 521 + [1 << 28]))          # 16733 bits: beyond the widest geometry
    assert run(h_mod=ctypes.addressof(wide), limbs=523) == -2
    rho_t, e_t = rows_of(eng, [5], 3), rows_of(eng, [2], 1)
    st = torch.zeros(1, dtype=torch.uint8, device=eng.device)
    for args in ((None, e_t.data_ptr(), e_t.data_ptr(), rho_t.data_ptr(), st.data_ptr(), 3, 1, 1, 1),
                 (rho_t.data_ptr(), None, e_t.data_ptr(), rho_t.data_ptr(), st.data_ptr(), 3, 1, 1, 1),
                 (rho_t.data_ptr(), e_t.data_ptr(), None, rho_t.data_ptr(), st.data_ptr(), 3, 1, 1, 1),
                 (rho_t.data_ptr(), e_t.data_ptr(), e_t.data_ptr(), None, st.data_ptr(), 3, 1, 1, 1),
                 (rho_t.data_ptr(), e_t.data_ptr(), e_t.data_ptr(), rho_t.data_ptr(), None, 3, 1, 1, 1),
                 (rho_t.data_ptr(), e_t.data_ptr(), e_t.data_ptr(), rho_t.data_ptr(), st.data_ptr(), 0, 1, 1, 1),
                 (rho_t.data_ptr(), e_t.data_ptr(), e_t.data_ptr(), rho_t.data_ptr(), st.data_ptr(), 3, 0, 1, 1),
                 (rho_t.data_ptr(), e_t.data_ptr(), e_t.data_ptr(), rho_t.data_ptr(), st.data_ptr(), 3, 1, 0, 1),
                 (rho_t.data_ptr(), e_t.data_ptr(), e_t.data_ptr(), rho_t.data_ptr(), st.data_ptr(), 3, 1, 1, -1)):
        assert lib.mx_response_rows(*args, None) == -1, args
    assert lib.mx_response_rows(rho_t.data_ptr(), e_t.data_ptr(), e_t.data_ptr(), rho_t.data_ptr(), st.data_ptr(), (1 << 20) + 1, 1, 1, 1, None) == -2
    eng.synchronize()
    assert ints_of(eng, rho_t) == [5] and _lib.MX_MULTIEXP_MAX_WEIGHT_BITS == 16384


# ------------------------------------------------------------------ the per-row response
def response(rho, e, x, wz):
    full = [r + k * v for r, k, v in zip(rho, e, x)]
    return [f & ((1 << (32 * wz)) - 1) for f in full], [1 if f >> (32 * wz) else 0 for f in full]


@pytest.mark.parametrize("wz,ew,wx", [(11, 4, 11), (17, 4, 8), (5, 1, 1), (140, 4, 131)])
def test_response_rows_equal_python_ints(eng, wz, ew, wx):
    rnd = random.Random(wz * 1000 + wx)
    for count in (1, 63, 64, 65, 300):
        # rho < 2^(32 wz - 1) and e x < 2^(32 wz - 1): the sum fits
        xb = min(32 * wx, 32 * wz - 1 - 32 * ew)
        rho = [rnd.getrandbits(32 * wz - 1) for _ in range(count)]
        e = [rnd.getrandbits(32 * ew) for _ in range(count)]
        x = [rnd.getrandbits(xb) | 1 << (xb - 1) for _ in range(count)]
        want, status = response(rho, e, x, wz)
        assert not any(status)
        z_t, status_t = eng.response_rows_t(rows_of(eng, rho, wz), rows_of(eng, e, ew), rows_of(eng, x, wx))
        assert ints_of(eng, z_t) == want and [int(s) for s in status_t.cpu()] == status, count


def test_response_rows_directed_carries_extremes_and_the_forced_overflow(eng):
    wz, ew, wx = 12, 4, 8
    ones_x = (1 << (32 * wx)) - 1
    e_max = (1 << 128) - 1
    e_odd = random.Random(7).getrandbits(128) | 1
    x_inv = pow(e_odd, -1, 1 << (32 * wx))                 # e x = ...0001 in its low 32 wx bits
    cases = [  # (rho, e, x): one row each, all in ONE launch — every row its own secret
        *[((1 << k) - 1, e_odd, x_inv) for k in (1, 32, 33, 64, 255, 256, 32 * wx, 32 * wz - 1)],      # a carry through k bits
        (0, e_max, ones_x), ((1 << (32 * wz - 1)) - 1, e_max, ones_x), (12345, 0, ones_x), ((1 << (32 * wz)) - 1, 0, ones_x),
        (12345, e_max, 0), ((1 << (32 * wz)) - 1, e_max, 0), (0, 0, 0), ((1 << (32 * wz)) - 1, 1, 1), ((1 << (32 * wz)) - 1, e_max, ones_x),
    ]
    rho, e, x = ([c[k] for c in cases] for k in range(3))
    want, status = response(rho, e, x, wz)
    assert status[-2:] == [1, 1] and status[:8] == [0] * 8
    z_t, status_t = eng.response_rows_t(rows_of(eng, rho, wz), rows_of(eng, e, ew), rows_of(eng, x, wx))
    assert ints_of(eng, z_t) == want and [int(s) for s in status_t.cpu()] == status
    # the forced overflow: row 40 of 70 does not fit — through the last carry, and through a column above wz (wx + ew > wz)
    for wx2, x40 in ((8, ones_x), (10, (1 << 320) - 1)):
        rho = [random.Random(k).getrandbits(32 * wz - 2) for k in range(70)]
        e = [random.Random(100 + k).getrandbits(64 if wx2 == 8 else 30) for k in range(70)]
        x = [random.Random(200 + k).getrandbits(32 * wx2) for k in range(70)]
        rho[40], e[40], x[40] = (1 << (32 * wz)) - 1, (1 if wx2 == 8 else e_max), x40
        want, status = response(rho, e, x, wz)
        assert status == [0] * 40 + [1] + [0] * 29
        z_t, status_t = eng.response_rows_t(rows_of(eng, rho, wz), rows_of(eng, e, ew), rows_of(eng, x, wx2))
        assert [int(s) for s in status_t.cpu()] == status and ints_of(eng, z_t) == want
    with pytest.raises(ValueError):
        eng.response_rows_t(rows_of(eng, [1, 2], wz), rows_of(eng, [1, 2], ew), rows_of(eng, [1], wx))          # one secret row per proof
    z_t, status_t = eng.response_rows_t(rows_of(eng, [], wz), rows_of(eng, [], ew), rows_of(eng, [], wx))
    assert tuple(z_t.shape) == (0, wz) and tuple(status_t.shape) == (0,)


# ------------------------------------------------------------------ the proofs
def test_proofs_at_the_smallest_key_equal_the_model_row_for_row(eng):
    from protocols.distributed_keygen_amd import DeviceRng, range_proof

    params, _, mpar = rc.parameters(128)
    msgs, rands, cts = rc.statements(N1K, BITS, 7)
    proofs = range_proof.prove_batch(N1K, params, BITS, msgs, rands, rc.LABEL, rng=DeviceRng(key=rc.KEY, first_call=40), engine=eng)
    want = rc.model_proofs(N1K, mpar, BITS, rc.LABEL, msgs, rands, 40)
    got = proofs.to_ints()
    for name, g, w in zip(range_proof.RangeProofs.FIELDS, got, want):
        assert g == w, name
    assert range_proof.verify_batch(N1K, params, BITS, cts, proofs, rc.LABEL, engine=eng) == [True] * 7
    # verdicts per row: every tampering spoils row 1 of the first three rows and nothing else
    ints = tuple(list(col[:3]) for col in got)
    for name, tcts, *cols in tamperings(N1K, params, ints, cts[:3], rm.encrypt(N1K, 5, 77)):
        spoiled = range_proof.RangeProofs.from_ints(*cols, N1K, params, BITS)
        assert range_proof.verify_batch(N1K, params, BITS, tcts, spoiled, rc.LABEL, engine=eng) == [True, False, True], name
    assert range_proof.verify_batch(N1K, params, BITS, cts, proofs, b"another session", engine=eng) == [False] * 7
    assert range_proof.verify_batch(N1K, params, BITS + 1, cts, proofs, rc.LABEL, engine=eng) == [False] * 7
    # the bounds of z1 and z3, where they are enforced
    sh = range_proof.shape(N1K, params.nh, BITS)
    for which, top in ((3, 1 << sh["z1_bits"]), (5, 1 << sh["z3_bits"])):
        cols = [list(col) for col in ints]
        cols[which][0], cols[which][1] = top - 1, top
        spoiled = range_proof.RangeProofs.from_ints(*cols, N1K, params, BITS)
        ok = eng.range_bounds_t(rows_of(eng, cts[:3], sh["limbs2"]), *(eng.to_device(t) for t in spoiled.rows()), N1K, params.nh, BITS)
        assert [bool(v) for v in ok.cpu()] == [True, False, True]
    # a 128-bit N carries no proof at all
    with pytest.raises(ValueError):
        range_proof.prove_batch(rc.modulus(128), params, 1, [0], [3], rc.LABEL, engine=eng)


def test_both_routes_of_the_products_give_the_models_proofs(eng):
    """Below 2085 bits of auxiliary modulus the shared-base products are one modexp per term, above it one
    multi-exponentiation (Engine.RANGE_MULTIEXP_MIN_BITS, from the measurements): an odd 2100-bit modulus — the mechanics
    need no safe primes — takes the kernel, and both routes of both helpers agree with pow on the same rows."""
    from protocols.distributed_keygen_amd import DeviceRng, range_proof

    nh = random.Random(21).getrandbits(2100) | (1 << 2099) | 1
    assert eng.range_uses_multiexp(nh) and not eng.range_uses_multiexp(rc.modulus(2048))
    params = range_proof.RangeParameters(nh, pow(3, 12345, nh), 9)
    mpar = rm.Parameters(*params.to_ints())
    msgs, rands, cts = rc.statements(N1K, BITS, 3)
    proofs = range_proof.prove_batch(N1K, params, BITS, msgs, rands, rc.LABEL, rng=DeviceRng(key=rc.KEY, first_call=40), engine=eng)
    assert proofs.to_ints() == rc.model_proofs(N1K, mpar, BITS, rc.LABEL, msgs, rands, 40)
    assert range_proof.verify_batch(N1K, params, BITS, cts, proofs, rc.LABEL, engine=eng) == [True] * 3
    rnd = random.Random(3)
    for mod in (rc.modulus(1024), nh):
        width = (mod.bit_length() + 31) // 32
        w0, w1 = [rnd.getrandbits(70) for _ in range(9)], [rnd.getrandbits(300) for _ in range(9)]
        want = [pow(5, a, mod) * pow(7, b, mod) % mod for a, b in zip(w0, w1)]
        for route in ("multiexp", "modexps"):
            assert ints_of(eng, eng._shared_pair_t(5, 7, rows_of(eng, w0, 3), rows_of(eng, w1, 10), mod, 70, 300, route=route)) == want, route
        first, second, e = ([rnd.randrange(mod) for _ in range(9)] for _ in range(3))
        e = [v & ((1 << 128) - 1) for v in e]
        want = [a * pow(b, k, mod) % mod for a, b, k in zip(first, second, e)]
        for route in ("multiexp", "modexps"):
            assert ints_of(eng, eng._own_pair_t(rows_of(eng, first, width), rows_of(eng, second, width), rows_of(eng, e, 4), mod, route=route)) == want, route
    with pytest.raises(ValueError):
        range_proof.prove_batch(N1K, params, BITS, msgs, rands, rc.LABEL, engine=eng, draws=None, rng=DeviceRng(), ciphertexts=cts[:1])
    m_t = rows_of(eng, [1 << 70, 1], range_proof.shape(N1K, nh, BITS)["z1_words"])
    with pytest.raises(ValueError):          # a message longer than the promised message_bits is refused, not exponentiated short
        eng.range_prove_t(rows_of(eng, cts[:2], 64), m_t, rows_of(eng, rands[:2], 32), N1K, nh, params.s, params.t, BITS, bytes(32),
                          rng=DeviceRng(), message_bits=BITS)


@pytest.mark.parametrize("key_length,aux_bits", [(1024, 2048), (2048, 1024)])
def test_end_to_end_at_mixed_widths(eng, key_length, aux_bits):
    from protocols.distributed_keygen_amd import DeviceRng, range_proof

    n = rc.modulus(key_length)
    params, _, mpar = rc.parameters(aux_bits)
    bits = 40
    msgs = [0, (1 << bits) - 1, 123456789]
    cts, proofs = range_proof.encrypt_with_proof(n, params, bits, msgs, rc.LABEL, rng=DeviceRng(key=rc.KEY, first_call=5), engine=eng)
    assert range_proof.verify_batch(n, params, bits, cts, proofs, rc.LABEL, engine=eng) == [True] * 3
    cols = proofs.to_ints()
    assert rm.verify(n, mpar, bits, rc.LABEL, cts[0], [col[0] for col in cols])          # the model accepts the engine's first proof
    spoiled = [list(col) for col in cols]
    spoiled[3][2] += 1                                                                    # z1 of row 2
    received = range_proof.RangeProofs.from_ints(*spoiled, n, params, bits)
    assert range_proof.verify_batch(n, params, bits, cts, received, rc.LABEL, engine=eng) == [True, True, False]
