"""The lifted tape of the N^2 modexp on the device (csrc/mx_powmod_n2.hpp: N2_SQR0 / N2_MUL0 / N2_CLR1):
one-wavefront launches with the lifted tape (MX_KNOB_N2_LIFT = 1) against pow() and, row for row, against the classic
tape of the same plan (= 0), at 9 and 18 limbs per lane, with segment boundaries inside phase 1, on the build of the
second table and inside phase 2; the two-wavefront form of the same plan still reads the classic tape."""

from __future__ import annotations

import random

import pytest

pytestmark = pytest.mark.gpu

P521, Q508 = (1 << 521) - 1, (1 << 508) - 0x1BD          # tests/test_n2_lift_tape.py: the 1029-bit modulus with a known factor
COUNT = 33                                               # a full wavefront's groups plus a tail group at every geometry but K = 1


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine()


def _case(bits: int):
    rng = random.Random(1000 + bits)
    if bits == 1029:
        n, factor = P521 * Q508, P521
    else:
        n, factor = rng.getrandbits(bits) | (1 << (bits - 1)) | 1, 3
    n2 = n * n
    bases = [0, 1, n, n + 1, n2 - 1, factor * rng.randrange(1, n) % n2]
    bases += [rng.randrange(n2) for _ in range(COUNT - len(bases))]
    ebits = int(2.05 * bits)
    exps = {"kN": (rng.getrandbits(bits // 2) | 1) * n, "N+1": n + 1, "2.05x": rng.getrandbits(ebits) | (1 << (ebits - 1))}
    return n, bases, exps, {name: [pow(b, e, n2) for b in bases] for name, e in exps.items()}


@pytest.mark.parametrize("bits", [131, 1029, 2051])
def test_lifted_tape_matches_pow_and_the_classic_tape(eng, bits):
    n, bases, exps, want = _case(bits)
    try:
        eng.set_wavefronts_per_group(1)
        for name, e in exps.items():
            desc = eng.nsquare_plan(n, e).desc
            assert desc.lift & 1 and desc.ntape_lift > 0, name             # every exponent here is above N
            assert bool(desc.lift & 2) == (name != "N+1"), name            # ... and long enough to pay, but for N + 1
            for lpl in (9, 18):
                eng.set_limbs_per_lane(lpl)
                eng.set_segments(3)
                eng.debug_knob("n2_lift", 0)
                classic = eng.powmod_nsquare_batch(bases, e, n)          # (its segments are the existing suite's business)
                eng.debug_knob("n2_lift", 1)
                for seg in (1, 3, 4, 7):
                    eng.set_segments(seg)
                    lifted = eng.powmod_nsquare_batch(bases, e, n)
                    assert lifted == want[name], (bits, name, lpl, seg)
                    assert classic == lifted, (bits, name, lpl, seg)
        # the planner's choice (the default) on the library's own segments, and a tail-only launch
        eng.debug_knob("n2_lift", 2)
        eng.set_segments(0)
        eng.set_limbs_per_lane(18)
        assert eng.powmod_nsquare_batch(bases[:17], exps["2.05x"], n) == want["2.05x"][:17]
        # two wavefronts per group on the same plan: the classic tape is intact beside the lifted one
        eng.debug_knob("n2_lift", 1)
        eng.set_wavefronts_per_group(2)
        eng.set_limbs_per_lane(9)
        assert eng.powmod_nsquare_batch(bases[:17], exps["2.05x"], n) == want["2.05x"][:17]
    finally:
        eng.debug_knob("n2_lift", 2)
        eng.set_segments(0)
        eng.set_limbs_per_lane(0)
        eng.set_wavefronts_per_group(0)
