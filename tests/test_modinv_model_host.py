"""The lane-level host model of modinv_kernel<LPL> (tests/modinv_model.py) against pow(v, -1, m), and the condition the
directed GPU tests rest on: for every instance, the cases kept by tests/modinv_cases.py reach every event of the model's list."""

from __future__ import annotations

import random
from functools import lru_cache

import pytest

import modinv_cases as cases
import modinv_model as model

# Events no candidate of the families reaches, per instance, with the reason.  At most two per instance.
UNCOVERED = {lpl: {"bound_reached": "no operand pair found keeps v != 0 until k >= 64 * limbs + 8 (k <= 2 * bits(M) for v < M)"}
             for lpl in model.LPLS}


def _pow_or_none(v, m):
    try:
        return pow(v, -1, m)
    except ValueError:
        return None


@lru_cache(maxsize=None)
def _selected(lpl, size):
    """[(modulus, value, recorded events, (inverse, k, events) of the model)] — computed once, shared by the tests below"""
    return [(m, v, ev, model.modinv(v, m)) for m, v, ev in cases.load()[(lpl, size)]]


@pytest.mark.parametrize("lpl", model.LPLS)
def test_model_matches_pow_on_selected_cases(lpl):
    for size in cases.SIZES:
        sel = _selected(lpl, size)
        assert 0 < len(sel) <= cases.MAX_CASES
        for m, v, recorded, (inv, k, ev) in sel:
            assert model.dispatch(m.bit_length(), (m.bit_length() + 31) // 32) == lpl
            assert m.bit_length() <= cases.size_bits(lpl, size)
            assert inv == _pow_or_none(v, m), (lpl, size, hex(m)[:40], hex(v)[:40])
            assert ev == recorded, "tests/golden/modinv_directed_cases.json is stale: run python tests/modinv_cases.py"
            assert k <= 2 * m.bit_length()
        assert any(m.bit_length() == cases.size_bits(lpl, size) for m, _, _, _ in sel)


def test_model_matches_pow_on_random_cases():
    rng = random.Random(576)
    for t in range(200):
        bits = rng.choice([2, 3, 5, 31, 32, 33, 63, 64, 65, 96, 100, 520, 1027, 2014, 2015, 2100] + [4062, 4070] * (t % 4 == 0))
        m = max(3, rng.getrandbits(bits) | (1 << (bits - 1)) | 1)
        v = rng.randrange(m)
        if t % 6 == 0:
            d = rng.choice([3, 5, 7, 2**31 - 1])
            m, v = m * d, (v * d) % (m * d)
        inv, k, ev = model.modinv(v, m)
        assert inv == _pow_or_none(v, m), (v, m)
        assert ev <= set(model.EVENTS) and "bound_reached" not in ev
        # rows wider than the modulus: the dispatch and the bound follow the row width, the inverse does not change
        wide = (m.bit_length() + 31) // 32 + rng.choice([1, 7, 70])
        assert model.modinv(v, m, limbs=wide)[0] == inv


@pytest.mark.parametrize("lpl", model.LPLS)
def test_model_matches_pow_on_the_families(lpl):
    """every candidate of the small size (for LPL >= 2 a sample of them: a run is 10 ms to 0.4 s)"""
    cand = cases.candidates(lpl, "small")
    step = 1 if lpl == 1 else max(1, len(cand) * lpl * lpl // 150)
    for _, _, mname, vname, m, v in cand[::step]:
        inv, _, ev = model.modinv(v, m)
        assert inv == _pow_or_none(v, m), (lpl, mname, vname)
        assert "bound_reached" not in ev


@pytest.mark.parametrize("lpl", model.LPLS)
def test_selected_cases_reach_every_event(lpl):
    reached = set()
    for size in cases.SIZES:
        for _, _, _, (_, _, ev) in _selected(lpl, size):
            reached |= ev
    expected = set(model.EVENTS) - (set(model.IN_LANE_EVENTS) if lpl == 1 else set())
    uncovered = UNCOVERED[lpl]
    assert len(uncovered) <= 2
    missing = expected - reached
    assert missing == set(uncovered), f"LPL = {lpl}: not reached: {sorted(missing - set(uncovered))}; listed as uncovered but reached: {sorted(set(uncovered) - missing)}"


def test_dispatch_and_size_error():
    assert [model.dispatch(32 * need - 40, need - 1) for need in (64, 65, 128, 129, 192, 193, 320, 321)] == [1, 2, 2, 3, 3, 5, 5, 9]
    assert model.dispatch(100, 576) == 9 and model.dispatch(100, 577) is None
    assert model.dispatch(model.MAX_MOD_BITS, 522) == 9 and model.dispatch(model.MAX_MOD_BITS + 1, 523) is None
    with pytest.raises(model.SizeError):
        model.modinv(2, 3, limbs=577)
    assert {(need, lpl) for need, _, _, lpl in cases.dispatch_boundary_moduli()} == {
        (64, 1), (65, 2), (128, 2), (129, 3), (192, 3), (193, 5), (320, 5), (321, 9), (576, 9), (577, None)}
    for need, limbs, m, lpl in cases.dispatch_boundary_moduli()[:4]:
        assert model.modinv(m - 2, m, limbs=limbs)[0] == pow(m - 2, -1, m)


def _keep_top_run(wv, P):
    """P with every lane cleared that does not belong to the unbroken run of set lanes ending at lane 63"""
    notp = P ^ wv.ONES0
    if not notp:
        return P
    cut = wv.B * ((notp.bit_length() - 1) // wv.B + 1)
    return P >> cut << cut


@pytest.mark.parametrize("mutant", ["no_propagate", "propagate_only_through_the_empty_top_lanes"])
def test_selected_cases_notice_a_ripple_that_loses_its_propagate_ballot(monkeypatch, mutant):
    """Two arithmetic-only mutants of WaveInt::ripple in the model: P dropped (cin = G << 1), and P honoured only in the run
    of lanes that ends at the top lane (the empty lanes above both operands, through which every borrow of u < v has to travel
    — the one use of P that any operand pair makes).  Under either, the selected cases of every instance give a wrong result."""
    ripple = model.Wave.ripple
    if mutant == "no_propagate":
        monkeypatch.setattr(model.Wave, "ripple", lambda self, G, P: ripple(self, G, 0))
    else:
        monkeypatch.setattr(model.Wave, "ripple", lambda self, G, P: ripple(self, G, _keep_top_run(self, P)))
    for lpl in model.LPLS:
        assert any(model.modinv(v, m)[0] != _pow_or_none(v, m) for m, v, _ in cases.load()[(lpl, "small")]), lpl
