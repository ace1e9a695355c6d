"""Directed operands for modinv_kernel<LPL> (csrc/mx_modinv.hpp), every instance at its widest and at a small size: the cases
that tests/modinv_cases.py chose with the lane-level model, which between them take every carry-propagate, zero-word, in-lane
ripple, exit and tail path the model knows of (tests/test_modinv_model_host.py holds that condition).  The reference is
pow(v, -1, m)."""

from __future__ import annotations

import math
from functools import lru_cache

import pytest

import modinv_cases as cases
import modinv_model as model

pytestmark = pytest.mark.gpu

KEYS = [(lpl, size) for lpl in model.LPLS for size in cases.SIZES]


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine()


@lru_cache(maxsize=None)
def _by_modulus(lpl, size):
    """{modulus: (invertible values, non-invertible values)} of the selected cases of (instance, size)"""
    out = {}
    for m, v, _ in cases.load()[(lpl, size)]:
        out.setdefault(m, ([], []))[0 if math.gcd(v, m) == 1 else 1].append(v)
    return out


def _direct(eng, vals, m, limbs=None):
    from protocols.distributed_keygen_amd import limbs as L

    limbs = limbs or L.limbs_for(m)
    return L.unpack(eng.to_host(eng.modinv_direct_t(eng.to_device(L.pack(vals, limbs)), m)))


@pytest.mark.parametrize("lpl,size", KEYS)
def test_modinv_direct_selected_cases(eng, lpl, size):
    for m, (good, bad) in _by_modulus(lpl, size).items():
        assert model.dispatch(m.bit_length(), (m.bit_length() + 31) // 32) == lpl
        assert len(good) <= cases.MAX_CASES
        if good:
            assert _direct(eng, good, m) == [pow(v, -1, m) for v in good]
        for v in bad:                                        # one per call: alone, and as the last row behind invertible ones
            with pytest.raises(ValueError):
                _direct(eng, [v], m)
            with pytest.raises(ValueError):
                _direct(eng, [2, m - 2, v], m)


@pytest.mark.parametrize("lpl,size", KEYS)
def test_modinv_direct_refuses_zero_and_common_factors(eng, lpl, size):
    """v = 0 (no trip of the loop) and v = u > 1 reached inside the loop (the `equal` exit with u != 1), each as the only row
    and as the last row; the same rows without the offender invert."""
    m = next(m for _, m in cases.moduli(lpl, size) if m % 3 == 0)
    good = [2, m - 2, (m + 1) // 2]
    assert _direct(eng, good, m) == [pow(v, -1, m) for v in good]
    for v in (0, 3, m - 3, m // 3):
        assert math.gcd(v, m) != 1
        with pytest.raises(ValueError):
            _direct(eng, [v], m)
        with pytest.raises(ValueError):
            _direct(eng, good + [v], m)
    assert "equal_exit_u_not_one" in model.modinv(m // 3, m)[2]
    assert "v_zero_on_entry" in model.modinv(0, m)[2]


@pytest.mark.parametrize("lpl,size", KEYS)
def test_modinv_batch_product_tree_over_special_moduli(eng, lpl, size):
    """Engine.modinv_batch in batches of 1, 2, 3 (direct) and 17 (the product tree, whose root the wave kernel inverts)"""
    for m in list(_by_modulus(lpl, size))[:3]:
        units = [v for _, v in cases.values(lpl, m) if math.gcd(v, m) == 1]
        units = (units + [(7919 * k + 1) % m for k in range(1, 18) if math.gcd(7919 * k + 1, m) == 1])[:17]
        assert len(units) == 17
        for batch in (1, 2, 3, 17):
            assert eng.modinv_batch(units[-batch:], m) == [pow(v, -1, m) for v in units[-batch:]], (m.bit_length(), batch)


def test_modinv_dispatch_boundaries(eng):
    """both sides of need = 64/65, 128/129, 192/193, 320/321 and the last size taken, 576; 577 words: the size error"""
    from protocols.distributed_keygen_amd._lib import MxError

    seen = set()
    for need, limbs, m, lpl in cases.dispatch_boundary_moduli():
        h = m.bit_length() // 2
        vals = [v for v in (2, 3, m - 2, (m + 1) // 2, (1 << h) - 1, 1 << h, m - (1 << 64)) if math.gcd(v, m) == 1]
        if lpl is None:
            with pytest.raises(MxError) as err:
                _direct(eng, vals, m, limbs)
            assert err.value.code == -2                      # MX_ERR_SIZE
        else:
            assert _direct(eng, vals, m, limbs) == [pow(v, -1, m) for v in vals], need
        seen.add((need, lpl))
    assert seen == {(64, 1), (65, 2), (128, 2), (129, 3), (192, 3), (193, 5), (320, 5), (321, 9), (576, 9), (577, None)}
