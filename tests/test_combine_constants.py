"""Share recombination with every per-key constant built on the host (csrc/mx_combine.hpp, mx_combine_prepare): the
product of the np raw partials and ONE product by R^np mod N^2 instead of a conversion of every partial, a product by
one and R^2 derived on the device.  Bit-exact against CPython integers (tests/combine_cases.py builds the inputs with
pow); the rows the recombination refuses against what the library wrote for them before the change
(tests/golden/combine_bad_rows.json).  np = 9 is beyond the constants a plan holds and takes the general route."""

from __future__ import annotations

import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

import combine_cases as cc

GOLDEN = Path(__file__).resolve().parent / "golden" / "combine_bad_rows.json"
NP_MAX = 8            # include/mxpaillier.h: MX_COMBINE_NP_MAX


# ------------------------------------------------------------------ host constants (no GPU)
@pytest.mark.parametrize("key_length", cc.KEY_LENGTHS)
def test_host_constants_against_python(key_length):
    from protocols.distributed_keygen_amd import _lib, limbs as Lm

    lib = _lib.lib()
    key = cc.make_key(key_length)
    n, n2 = key.n, key.n_square
    limbs, limbs2 = Lm.limbs_for(n), Lm.limbs_for(n2) + 1      # rows one word wider than N^2: the padding stays zero
    k, l, w, b2 = (ctypes.c_int() for _ in range(4))
    assert lib.mx_geometry(n2.bit_length(), k, l, w, b2) == 0
    per_block = w.value * l.value
    r2 = 1 << (per_block * b2.value)
    r1 = 1 << (per_block * -(-(n.bit_length() + 4) // per_block))
    assert r2 >= 16 * n2 and r1 >= 16 * n
    rows = np.zeros((3 + NP_MAX, limbs2), dtype=np.uint32)
    h_n, h_t = Lm.pack_one(n, limbs), Lm.pack_one(key.theta_inv, limbs)
    assert lib.mx_combine_constants(h_n.ctypes.data, h_t.ctypes.data, limbs, limbs2, rows.ctypes.data, rows.size) == 0
    got = Lm.unpack(rows)
    assert got[:3] == [n, n2, key.theta_inv * r1 % n]
    assert got[3] == r2 % n2
    assert got[4] == r2 * r2 % n2                               # R^2: the general route's conversion constant
    for np_ in range(1, NP_MAX + 1):
        assert got[3 + np_ - 1] == pow(r2, np_, n2), np_
    assert lib.mx_combine_plan_bytes(limbs, limbs2) >= rows.size * 4
    # errors: short buffer, even modulus, rows too narrow for N^2
    assert lib.mx_combine_constants(h_n.ctypes.data, h_t.ctypes.data, limbs, limbs2, rows.ctypes.data, rows.size - 1) == -4
    even = Lm.pack_one(n - 1, limbs)
    assert lib.mx_combine_constants(even.ctypes.data, h_t.ctypes.data, limbs, limbs2, rows.ctypes.data, rows.size) == -3
    assert lib.mx_combine_constants(h_n.ctypes.data, h_t.ctypes.data, limbs, limbs, rows.ctypes.data, rows.size) == -1
    assert lib.mx_combine_constants(h_n.ctypes.data, h_t.ctypes.data, limbs, limbs2, None, rows.size) == -1


# ------------------------------------------------------------------ the kernel
@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine()


def _device_rows(eng, key, rows, np_):
    from protocols.distributed_keygen_amd import limbs as Lm

    limbs2 = Lm.limbs_for(key.n_square)
    return eng.to_device(np.stack([Lm.pack([r[i] for r in rows], limbs2) for i in range(np_)]))


@pytest.mark.gpu
@pytest.mark.parametrize("np_", cc.NPS + (cc.NP_GENERAL,))
@pytest.mark.parametrize("key_length", cc.KEY_LENGTHS)
def test_recombination_against_python(eng, key_length, np_):
    from protocols.distributed_keygen_amd import limbs as Lm

    key = cc.make_key(key_length)
    rows, want = cc.good_case(key_length, np_)
    limbs = Lm.limbs_for(key.n)
    for batch in (1, 5, 64):
        t = _device_rows(eng, key, rows[:batch], np_)
        out_t, status_t = eng.combine_t(t, key.n, key.theta_inv)
        assert status_t.cpu().numpy().tolist() == [0] * batch, (key_length, np_, batch)
        assert Lm.unpack(eng.to_host(out_t)) == want[:batch], (key_length, np_, batch)
        # one row per ciphertext, out_stride = limbs + 1: the plaintext words, then the status word
        packed = eng.to_host(eng.combine_t(t, key.n, key.theta_inv, packed=True))
        assert packed.shape == (batch, limbs + 1)
        assert Lm.unpack(packed[:, :limbs]) == want[:batch] and not packed[:, limbs].any(), (key_length, np_, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cc.bad_cases()))
def test_refused_rows_as_before(eng, name):
    """Rows whose product is not 1 modulo N (or is 0): status 1 and the output words the library wrote before, beside
    good rows in the same launch, which are not disturbed."""
    from protocols.distributed_keygen_amd import limbs as Lm

    key_length, np_ = cc.bad_cases()[name]
    golden = json.loads(GOLDEN.read_text())[name]
    key = cc.make_key(key_length)
    bad = cc.bad_rows(key_length, np_)
    good, want = cc.good_case(key_length, np_)
    rows = bad + good[:5]
    limbs = Lm.limbs_for(key.n)
    t = _device_rows(eng, key, rows, np_)
    out_t, status_t = eng.combine_t(t, key.n, key.theta_inv)
    out = eng.to_host(out_t)
    assert status_t.cpu().numpy().tolist() == golden["status"] + [0] * 5 == [1] * len(bad) + [0] * 5
    assert out[: len(bad)].tolist() == golden["plain_words"]
    assert Lm.unpack(out[len(bad):]) == want[:5]
    packed = eng.to_host(eng.combine_t(t, key.n, key.theta_inv, packed=True))
    assert packed[: len(bad)].tolist() == golden["packed_words"]
    assert packed[: len(bad), limbs].tolist() == [1] * len(bad)
    assert Lm.unpack(packed[len(bad):, :limbs]) == want[:5] and not packed[len(bad):, limbs].any()
