"""The symmetric product of the squaring pass at an even number of limbs per lane (csrc/mx_mont.hpp: slot_weight): the
half-way pairs a_u a_v, (v - u) mod L == L/2, are multiplied once with the doubled multiplier limb, from the step below
L/2, instead of once from each side.  Squarings at 18 limbs per lane through every kernel family that runs them, bit-exact
against CPython integers; 9 limbs per lane (odd: no half-way pairs) pinned beside them.

Moduli of 500, 1030 and 2051 bits give groups of 1, 2 and 4 lanes at 18 limbs per lane (one block per lane each), so the
partner of a half-way pair lies in the same lane, in the neighbouring lane and up to three lanes away.  Exponents 2^k are
squarings only; the 70-bit exponent mixes them with the table's multiplications.  The 18 bases run as one launch of 17
(a last workgroup with surplus groups) and launches of one."""

from __future__ import annotations

import random

import pytest

pytestmark = pytest.mark.gpu

BITS = (500, 1030, 2051)
LANES = {500: 1, 1030: 2, 2051: 4}
EXPONENTS = (1 << 1, 1 << 2, 1 << 17, random.Random(70).getrandbits(70) | (1 << 69) | 1)


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    e = Engine()
    yield e
    e.set_limbs_per_lane(0)
    e.set_wavefronts_per_group(0)
    e.debug_knob("n2_friendly_1w", 0)


def _modulus(bits: int) -> int:
    rng = random.Random(bits)
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def _bases(n: int, modulus: int):
    """0, 1, N - 1, N^2 - 1, the largest number below the modulus whose 29-bit limbs are all ones, 13 random residues —
    reduced modulo the modulus of the path (for the generic kernel, whose modulus is N itself, N^2 - 1 is N - 1 again)."""
    rng = random.Random(n % 1000003)
    ones = (1 << (29 * ((modulus.bit_length() - 1) // 29))) - 1
    assert 0 < ones < modulus and ones.bit_length() % 29 == 0
    return [b % modulus for b in (0, 1, n - 1, n * n - 1, ones)] + [rng.randrange(modulus) for _ in range(13)]


def _launches(bases):
    """one launch of 17, then launches of one: the base left over and the all-ones base"""
    return [bases[:17], bases[17:], [bases[4]]]


def _nsquare(eng, bases, n, e, lpl, wpg):
    from protocols.distributed_keygen_amd import limbs as Lm

    n2 = n * n
    rows = eng.to_device(Lm.pack(bases, Lm.limbs_for(n2)))
    return Lm.unpack(eng.to_host(eng.powmod_nsquare_t(rows, n, e, shape=(lpl, wpg))))


def _instance(bits, batch, lpl, wpg):
    from instance_cases import _instance as query
    from protocols.distributed_keygen_amd import _lib

    return query(_lib.lib(), bits, batch, lpl, wpg)


@pytest.mark.parametrize("wpg", [1, 2])
@pytest.mark.parametrize("bits", BITS)
def test_pair_kernel_squarings_18_limbs(eng, bits, wpg):
    n = _modulus(bits)
    n2 = n * n
    bases = _bases(n, n2)
    want = {e: [pow(b, e, n2) for b in bases] for e in EXPONENTS}
    for launch, lo in zip(_launches(bases), (0, 17, 4)):
        inst = _instance(bits, len(launch), 18, wpg)
        assert inst is not None and inst[:3] == (LANES[bits], 18, wpg), inst
        for e in EXPONENTS:
            assert _nsquare(eng, launch, n, e, 18, wpg) == want[e][lo : lo + len(launch)], (bits, wpg, len(launch), e.bit_length())


def test_pair_kernel_squarings_18_limbs_friendly_and_plain_instance(eng):
    """At 2051 bits the host takes the friendly-modulus instance of the one-wavefront kernel (the modulus leaves the room);
    the runs above went through it.  Here the plain instance of the same geometry on the same inputs."""
    bits = 2051
    n = _modulus(bits)
    n2 = n * n
    bases = _bases(n, n2)
    assert _instance(bits, 17, 18, 1)[3] == 1                 # friendly by the host's choice
    eng.debug_knob("n2_friendly_1w", 1)
    try:
        assert _instance(bits, 17, 18, 1)[3] == 0
        for launch, lo in zip(_launches(bases), (0, 17, 4)):
            for e in EXPONENTS:
                assert _nsquare(eng, launch, n, e, 18, 1) == [pow(b, e, n2) for b in bases[lo : lo + len(launch)]], (len(launch), e.bit_length())
    finally:
        eng.debug_knob("n2_friendly_1w", 0)


@pytest.mark.parametrize("bits", BITS)
def test_generic_kernel_squarings_18_limbs(eng, bits):
    from protocols.distributed_keygen_amd import limbs as Lm

    mod = _modulus(bits)
    bases = _bases(mod, mod)
    eng.set_limbs_per_lane(18)
    try:
        for launch, lo in zip(_launches(bases), (0, 17, 4)):
            assert eng.geometry(bits, len(launch), 1)[:2] == (LANES[bits], 18)
            rows = eng.to_device(Lm.pack(launch, Lm.limbs_for(mod)))
            for e in EXPONENTS:
                got = Lm.unpack(eng.to_host(eng.powmod_shared_t(rows, mod, e)))
                assert got == [pow(b, e, mod) for b in bases[lo : lo + len(launch)]], (bits, len(launch), e.bit_length())
    finally:
        eng.set_limbs_per_lane(0)


@pytest.mark.parametrize("path", ["pair-1", "pair-2", "generic"])
def test_nine_limbs_per_lane_unchanged(eng, path):
    """Odd L has no half-way pairs: one case per path at 9 limbs per lane (groups of 8 lanes at 2051 bits)."""
    from protocols.distributed_keygen_amd import limbs as Lm

    bits = 2051
    n = _modulus(bits)
    modulus = n if path == "generic" else n * n
    bases = _bases(n, modulus)[:17]
    e = EXPONENTS[2] * 3                                       # 17 squarings and a multiplication
    if path == "generic":
        eng.set_limbs_per_lane(9)
        try:
            assert eng.geometry(bits, len(bases), 1)[:2] == (8, 9)
            got = Lm.unpack(eng.to_host(eng.powmod_shared_t(eng.to_device(Lm.pack(bases, Lm.limbs_for(n))), n, e)))
        finally:
            eng.set_limbs_per_lane(0)
    else:
        wpg = int(path[-1])
        assert _instance(bits, len(bases), 9, wpg)[:3] == (8, 9, wpg)
        got = _nsquare(eng, bases, n, e, 9, wpg)
    assert got == [pow(b, e, modulus) for b in bases]
