"""Host logic of packed threshold decryption (protocols/distributed_keygen_amd/packing.py) on the CPU: the slot layout,
unpacking against sums built with Python ints, and the protocol step with three stand-in parties whose packing comes
from a pure-Python test double of Engine.ciphertext_pack_batch."""

from __future__ import annotations

import asyncio
import ctypes
import random

import pytest

from protocols.distributed_keygen_amd import packing


class PyPackEngine:
    """Engine.ciphertext_pack_batch over Python ints: prod_i c_(j k + i)^(2^(b i)) mod N^2."""

    def __init__(self):
        self.calls = []

    def ciphertext_pack_batch(self, cts, n, slot_bits, slots):
        self.calls.append((len(cts), slot_bits, slots))
        n2 = n * n
        out = []
        for j in range(0, len(cts), slots):
            acc = 1
            for i, c in enumerate(cts[j : j + slots]):
                acc = acc * pow(c % n2, 1 << (slot_bits * i), n2) % n2
            out.append(acc)
        return out


def odd_modulus(bits, rng):
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def packed_plaintexts(values, slot_bits, n):
    """sum_i m_i 2^(b i) mod N for every group of k values, the last one ragged."""
    k = packing.slots_per_ciphertext(n, slot_bits)
    return [sum(m << (slot_bits * i) for i, m in enumerate(values[j : j + k])) % n for j in range(0, len(values), k)]


def test_slots_per_ciphertext_depends_on_n_and_slot_bits_only():
    rng = random.Random(1)
    for bits in (5, 64, 130, 1027, 2050, 4097):
        n = odd_modulus(bits, rng)
        for b in (1, 2, 7, 31, 32, 64, 100, bits - 2):
            if b < 1 or b > bits - 2:
                continue
            assert packing.slots_per_ciphertext(n, b) == (bits - 2) // b
        assert packing.slots_per_ciphertext(n, bits - 2) == 1
        with pytest.raises(ValueError):
            packing.slots_per_ciphertext(n, bits - 1)
        with pytest.raises(ValueError):
            packing.slots_per_ciphertext(n, 0)
    n = odd_modulus(2048, rng)                          # a 2048-bit N: 63 slots of 32 bits, 31 of 64
    assert packing.slots_per_ciphertext(n, 32) == 63 and packing.slots_per_ciphertext(n, 64) == 31


@pytest.mark.parametrize("slot_bits", [1, 7, 32, 63, 64, 65, 200])
@pytest.mark.parametrize("signed", [True, False])
def test_unpack_against_host_sums(slot_bits, signed):
    rng = random.Random(f"{slot_bits}{signed}")
    for bits in (300, 1030, 2050):
        n = odd_modulus(bits, rng)
        if slot_bits > bits - 2:
            continue
        k = packing.slots_per_ciphertext(n, slot_bits)
        lo, hi = (-(1 << (slot_bits - 1)), 1 << (slot_bits - 1)) if signed else (0, 1 << slot_bits)
        for count in sorted({1, max(k - 1, 1), k, k + 1, 3 * k + 5}):
            vals = [rng.randrange(lo, hi) for _ in range(count)]
            vals[0] = lo                                       # the range boundaries
            vals[-1] = hi - 1
            if count > 2:
                vals[1] = hi - 1
                vals[2] = lo
            pts = packed_plaintexts(vals, slot_bits, n)
            assert len(pts) == -(-count // k)
            assert packing.unpack(pts, slot_bits, count, n, signed=signed) == vals, (bits, count)
            assert packing.unpack(pts, slot_bits, count, n, signed=signed, use_numpy=False) == vals
            if slot_bits <= 64:
                assert packing.unpack(pts, slot_bits, count, n, signed=signed, use_numpy=True) == vals


def test_unpack_numpy_path_equals_plain_path_on_arbitrary_plaintexts():
    rng = random.Random(3)
    n = odd_modulus(2050, rng)
    for b in (1, 3, 8, 13, 32, 33, 57, 63, 64):
        k = packing.slots_per_ciphertext(n, b)
        count = 5 * k - 2
        pts = [rng.randrange(n) for _ in range(5)]            # any residue: values outside their range included
        for signed in (True, False):
            assert packing.unpack(pts, b, count, n, signed, use_numpy=True) == packing.unpack(pts, b, count, n, signed, use_numpy=False)


def test_unpack_refuses_a_wrong_number_of_plaintexts():
    n = odd_modulus(1030, random.Random(4))
    k = packing.slots_per_ciphertext(n, 32)
    with pytest.raises(ValueError):
        packing.unpack([1, 2], 32, k, n)
    with pytest.raises(ValueError):
        packing.unpack([1], 32, k + 1, n)
    with pytest.raises(ValueError):
        packing.unpack([1], 65, 1, n, use_numpy=True)
    assert packing.unpack([], 32, 0, n) == []


def test_pack_reads_every_object_once_and_uses_the_layout():
    class Ct:
        def __init__(self, v, n):
            self.v, self.reads = v, 0
            self.scheme = type("S", (), {"public_key": type("P", (), {"n": n})()})()

        def get_value(self):
            self.reads += 1
            return self.v

    rng = random.Random(5)
    n = odd_modulus(300, rng)
    n2 = n * n
    a = Ct(rng.randrange(n2), n)
    cts = [a, rng.randrange(n2), a] + [rng.randrange(n2) for _ in range(20)]
    eng = PyPackEngine()
    got = packing.pack(cts, 64, engine=eng)
    k = packing.slots_per_ciphertext(n, 64)
    assert eng.calls == [(23, 64, k)] and a.reads == 1
    vals = [c if isinstance(c, int) else c.v for c in cts]
    assert got == PyPackEngine().ciphertext_pack_batch(vals, n, 64, k)
    assert packing.pack([], 64, n=n, engine=eng) == []


def run_parties(parties, cts, slot_bits, signed, eng):
    async def run():
        return await asyncio.gather(*[packing.decrypt_sequence_packed(dp, cts, slot_bits, signed=signed, engine=eng)
                                      for dp in parties])

    return asyncio.run(run())


@pytest.mark.parametrize("slot_bits,signed", [(32, True), (16, False), (3, True)])
def test_decrypt_sequence_packed_with_three_standin_parties(slot_bits, signed):
    import standin_harness as sh

    from protocols.distributed_keygen_amd import synthetic

    rng = random.Random(slot_bits)
    key = synthetic.make_key(128, 3, 1)
    n = key.n
    k = packing.slots_per_ciphertext(n, slot_bits)
    count = 3 * k + 2
    lo, hi = (-(1 << (slot_bits - 1)), 1 << (slot_bits - 1)) if signed else (0, 1 << slot_bits)
    values = [rng.randrange(lo, hi) for _ in range(count)]
    values[0], values[-1] = lo, hi - 1
    cts = sh.ciphertexts(key, [synthetic.encrypt(key, m % n, rng) for m in values])
    parties = sh.parties_for_key(key)
    assert any(key.exponent(i) < 0 for i in (1, 2, 3))           # a party with a negative Lagrange exponent
    sizes = []
    for dp in parties:
        orig = dp._decrypt_sequence_raw

        async def recording(seq, receivers=None, _orig=orig):
            seq = list(seq)
            sizes.append(len(seq))
            return await _orig(seq, receivers)

        dp._decrypt_sequence_raw = recording
    eng = PyPackEngine()
    got = run_parties(parties, cts, slot_bits, signed, eng)
    assert got == [values] * 3
    assert sizes == [-(-count // k)] * 3
    assert [c[2] for c in eng.calls] == [k] * 3


def test_decrypt_sequence_packed_returns_none_for_a_party_that_is_not_a_receiver():
    rng = random.Random(9)
    n = odd_modulus(300, rng)

    class Scheme:
        public_key = type("P", (), {"n": n})()

        def __init__(self):
            self.seen = None

        async def _decrypt_sequence_raw(self, seq, receivers=None):
            self.seen = (list(seq), receivers)
            if receivers is not None and "self" not in receivers:
                return None
            return [type("E", (), {"value": 0})() for _ in seq]

    s = Scheme()
    cts = [rng.randrange(n * n) for _ in range(10)]
    assert asyncio.run(packing.decrypt_sequence_packed(s, cts, 8, receivers=["p2"], engine=PyPackEngine())) is None
    assert s.seen[1] == ["p2"] and len(s.seen[0]) == 1 and s.seen[0][0].n == n      # plain ints: PlainCiphertext
    assert asyncio.run(packing.decrypt_sequence_packed(s, cts, 8, signed=False, engine=PyPackEngine())) == [0] * 10


def test_pack_instances_are_the_six_narrow_ones():
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    cnt = lib.mx_pack_nsquare_instances(None, None, 0)
    assert cnt == 6
    lanes, lpls = (ctypes.c_int * cnt)(), (ctypes.c_int * cnt)()
    assert lib.mx_pack_nsquare_instances(lanes, lpls, cnt) == cnt
    assert sorted(zip(lanes, lpls)) == [(1, 9), (2, 9), (4, 9), (8, 9), (16, 9), (32, 9)]
    assert lib.mx_pack_nsquare_instances(None, None, 3) == -1
