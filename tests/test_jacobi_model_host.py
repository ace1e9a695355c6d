"""The host models of the Jacobi kernels (tests/jacobi_model.py) against oracle.jacobi_symbol, and the condition the directed
GPU tests rest on: the operands chosen for every instance reach every path of both kernels that the models know of."""

from __future__ import annotations

import random
from functools import lru_cache

import pytest

import jacobi_model as jm
from oracle import oracle


@lru_cache(maxsize=None)
def _directed(nl: int):
    rows, mods = jm.directed_groups(nl)
    want = [[oracle.jacobi_symbol(v, m) for v in r] for r, m in zip(rows, mods)]
    return rows, mods, want, jm.launch_model(rows, mods), jm.launch_model(rows, mods, knob=1)


def test_models_match_the_oracle_on_random_operands():
    rng = random.Random(4100)
    for t in range(300):
        bits = rng.choice([2, 3, 5, 8, 31, 32, 33, 64, 65, 96, 131, 257, 520, 1028])
        n = rng.getrandbits(bits) | 1
        x = rng.randrange(n) if n > 1 else 0
        if t % 5 == 0:
            d = rng.choice([3, 5, 7, 15, 2**31 - 1])
            n, x = n * d, (x * d) % (n * d)
        if t % 7 == 0:
            x = (x << 32) % n
        want = oracle.jacobi_symbol(x, n)
        limbs = max(1, (n.bit_length() + 31) // 32)
        nl = jm.instance_for(limbs)
        res, _, _ = jm.divstep_wave_model([(x, n)], nl, 1 << 20)
        assert res == [want], (x, n)
        if n > 1 and x:
            assert jm.fallback_model(x, n, nl)[0] == want, (x, n)
        if t % 4 == 0:
            assert jm.launch_model([[x]], [n])[0] == [[want]]
            assert jm.launch_model([[x]], [n], knob=1)[0] == [[want]]


@pytest.mark.parametrize("nl", jm.INSTANCES)
def test_directed_operands_match_the_oracle_and_reach_every_path(nl):
    rows, mods, want, (got, dev, fev, most), (got1, dev1, fev1, _) = _directed(nl)
    assert all(len(r) <= 40 for r in rows)
    assert jm.instance_for(max((m.bit_length() + 31) // 32 for m in mods)) == nl
    assert any(m.bit_length() == 32 * nl for m in mods)                       # a modulus fills the instance's limbs
    assert got == want and got1 == want
    # the divstep kernel, with the launcher's own batch bound
    expected = set(jm.DIVSTEP_EVENTS)
    if nl <= jm.JC:
        expected.discard("live_chunk_crossed")             # one chunk: there is no boundary to cross
    if nl == 3:
        # 96 bits: the worst operands found (jacobi_model.worst_batches) need 20 batches, the bound is 22
        expected.discard("unfinished_at_max_batches")
    assert expected - dev == set(), f"NL = {nl}: divstep paths not reached: {sorted(expected - dev)}"
    # the safety net: from the original operands with the batches cut to none, and (NL >= 5) as the production path it is
    assert "unfinished_at_max_batches" in dev1
    assert set(jm.FALLBACK_EVENTS) - fev1 == set(), f"NL = {nl}: fallback paths not reached: {sorted(set(jm.FALLBACK_EVENTS) - fev1)}"
    if nl >= 5:
        assert fev and most == jm.max_batches_for(max((m.bit_length() + 31) // 32 for m in mods))


def test_structured_operands_exceed_the_batch_bound():
    """What csrc/mx_jacobi.hpp and DESIGN.md say of the safety net: it is a production path for (n - 1 / 2^k - 3) and its like."""
    for bits in (160, 1028):
        batches, _, _ = jm.worst_batches(bits)
        assert batches > jm.max_batches_for((bits + 31) // 32)
