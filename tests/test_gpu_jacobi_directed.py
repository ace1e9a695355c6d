"""Directed operands for jacobi_kernel<NL> and jacobi_fallback_kernel<NL> (csrc/mx_jacobi.hpp), every instance: moduli that
exactly fill the instance's limbs and moduli one bit over a chunk boundary, numerators chosen with tests/jacobi_model.py so
that every path the models know of is taken (tests/test_jacobi_model_host.py holds that condition).  Each instance runs once
with the launcher's batch bound — which these operands exceed, so that the safety net finishes them — and once with the
divstep batches cut to none, so that the safety net starts every symbol from its original operands.  The reference is
oracle.jacobi_symbol."""

from __future__ import annotations

import pytest

import jacobi_model as jm
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine()


@pytest.mark.parametrize("nl", jm.INSTANCES)
def test_jacobi_directed_operands(eng, nl):
    rows, mods = jm.directed_groups(nl)
    assert all(len(r) <= 40 for r in rows)
    want = [[oracle.jacobi_symbol(v, m) for v in r] for r, m in zip(rows, mods)]
    assert eng.jacobi_batch(rows, mods) == want
    try:
        eng.debug_knob("jacobi_max_batches", 1)              # no divstep batch at all
        assert eng.jacobi_batch(rows, mods) == want
    finally:
        eng.debug_knob("jacobi_max_batches", 0)
