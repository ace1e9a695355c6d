"""slots.py on a Python-int double of the two engine methods (tests/slots_engine.py): the layout against its definition
and against packing.unpack, every ValueError, the bound of slot_bits_for by brute force, and encrypt against pow.  No GPU."""

from __future__ import annotations

import asyncio
import itertools
import random

import numpy as np
import pytest

from slots_engine import SlotsEngine

from protocols.distributed_keygen_amd import packing, slots
from protocols.distributed_keygen_amd.randomizer import FastRandomizer

N = (random.Random(41).getrandbits(200) | (1 << 199) | 1)           # any odd modulus: the codec needs no factorisation


def definition(values, n, b):
    k = packing.slots_per_ciphertext(n, b)
    return [sum(m << (b * i) for i, m in enumerate(values[j : j + k])) % n for j in range(0, len(values), k)]


def ragged_counts(k):
    return sorted({0, 1, max(k - 1, 0), k, k + 1, 3 * k + 5})


@pytest.mark.parametrize("b,signed", [(b, True) for b in (1, 7, 32, 63, 64)] + [(b, False) for b in (1, 7, 32, 63)])
def test_encode_is_the_definition_and_round_trips(b, signed):
    eng = SlotsEngine()
    rng = random.Random(b * 2 + signed)
    k = packing.slots_per_ciphertext(N, b)
    lo, hi = (-(1 << (b - 1)), (1 << (b - 1)) - 1) if signed else (0, (1 << b) - 1)
    for count in ragged_counts(k):
        vals = [rng.randint(lo, hi) for _ in range(count)]
        if count:
            vals[0], vals[-1] = lo, hi
        got = slots.encode(vals, N, b, signed=signed, engine=eng)
        assert got == definition(vals, N, b)
        assert len(got) == -(-count // k)
        assert packing.unpack(got, b, count, N, signed=signed, use_numpy=False) == vals
        assert slots.decode(got, N, b, count, signed=signed, engine=eng) == vals
        # a numpy array and a sequence of ints are the same input
        assert slots.encode(np.array(vals, dtype=np.int64), N, b, signed=signed, engine=eng) == got


def test_every_value_error():
    eng = SlotsEngine()
    k = packing.slots_per_ciphertext(N, 8)
    vals = [1] * (2 * k + 3)
    vals[k + 4] = 128
    vals[-1] = -129
    with pytest.raises(ValueError, match=rf"\b{k + 4}\b"):                 # the FIRST offender's index
        slots.encode(vals, N, 8, engine=eng)
    with pytest.raises(ValueError, match=r"\b3\b"):
        slots.encode([0, 1, 2, 256], N, 8, signed=False, engine=eng)
    with pytest.raises(ValueError, match="packing.unpack"):
        slots.encode([1], N, 65, engine=eng)
    with pytest.raises(ValueError, match="packing.unpack"):
        slots.encode([1], N, 64, signed=False, engine=eng)
    with pytest.raises(ValueError, match="packing.unpack"):
        slots.decode([1], N, 65, 1, engine=eng)
    with pytest.raises(ValueError):
        slots.encode([1], N, 0, engine=eng)
    calls = len(eng.calls)
    with pytest.raises(ValueError, match=r"\b2\b.*int64"):                 # before any upload: the engine is not reached
        slots.encode([0, 1, 1 << 63], N, 64, engine=eng)
    with pytest.raises(ValueError, match="int64"):
        slots.encode([-(1 << 63) - 1], N, 64, engine=eng)
    with pytest.raises(ValueError, match="int64"):
        slots.encode(np.array([1 << 63], dtype=np.uint64), N, 64, engine=eng)
    assert len(eng.calls) == calls
    with pytest.raises(ValueError, match="packed plaintexts"):             # a wrong plaintext count
        slots.decode([1, 2], N, 8, k, engine=eng)
    with pytest.raises(ValueError, match="packed plaintexts"):
        slots.decode([], N, 8, 1, engine=eng)
    assert slots.decode([], N, 8, 0, engine=eng) == []


def brute_force_ok(v, wb, t, bb, b, eng):
    """Whether every extreme map decodes slot by slot at slot width b.  Inputs at both ends of their range, weights at both
    ends of theirs (weight_bits = 0: the weight 1), the bias at both ends; two slots so that an overflow of slot 0 shows
    in slot 1 as well."""
    xs = (-(1 << (v - 1)), (1 << (v - 1)) - 1)
    ws = (-((1 << wb) - 1), (1 << wb) - 1) if wb else (1,)
    betas = (-((1 << bb) - 1), (1 << bb) - 1) if bb else (0,)
    k = 2
    lo, hi = -(1 << (b - 1)), (1 << (b - 1)) - 1
    for x in itertools.product(xs, repeat=t):
        for w in itertools.product(ws, repeat=t):
            for beta in betas:
                want = [sum(wi * xi for wi, xi in zip(w, x)) + beta, 0]
                # the plaintexts: the definition itself (encode would refuse inputs wider than b, rightly)
                plain = [sum(m << (b * i) for i, m in enumerate((xi, 0))) % N for xi in x]
                bias = ((beta << 0) + (0 << b)) % N
                res = (sum(wi * p for wi, p in zip(w, plain)) + bias) % N
                got = slots.decode([res], N, b, k, engine=eng)
                assert got == packing.unpack([res], b, k, N, use_numpy=False)
                if got != want:
                    assert not lo <= want[0] <= hi                            # only an overflow may decode wrong
                    return False
    return True


@pytest.mark.parametrize("v,wb,t,bb", [(v, wb, t, bb) for v in (1, 2, 4) for wb in (0, 1, 3) for t in (1, 2, 3, 4) for bb in (0, 2)])
def test_slot_bits_for_is_safe_and_tight(v, wb, t, bb):
    eng = SlotsEngine()
    b = slots.slot_bits_for(v, wb, t, bb)
    assert packing.slots_per_ciphertext(N, b) >= 2
    assert brute_force_ok(v, wb, t, bb, b, eng)
    if b > 1:
        assert not brute_force_ok(v, wb, t, bb, b - 1, eng)               # one bit less overflows in some extreme case
    # the expected shape bounds it from above (a bias of fewer bits than the sum itself)
    shape = v + wb + (t - 1).bit_length()
    assert b <= shape + (1 if bb else 0) or bb >= shape


def test_slot_bits_for_through_encode():
    """The same map on encoded plaintexts, bias encoded once per slot: sum_i w_i encode(x_i) + encode(bias)."""
    eng = SlotsEngine()
    rng = random.Random(43)
    v, wb, t, bb = 4, 3, 4, 2
    b = slots.slot_bits_for(v, wb, t, bb)
    k = packing.slots_per_ciphertext(N, b)
    count = k + 3
    x = [[rng.randint(-8, 7) for _ in range(count)] for _ in range(t)]
    x[0][:2], x[1][:2], x[2][:2], x[3][:2] = [-8, -8], [-8, -8], [-8, -8], [-8, -8]
    w = [7, 7, -7, 7]
    w_hi = [-7, -7, -7, -7]
    beta = -3
    enc = [slots.encode(xi, N, b, engine=eng) for xi in x]
    bias = slots.encode([beta] * count, N, b, engine=eng)
    for ws in (w, w_hi):
        res = [(sum(wi * e[j] for wi, e in zip(ws, enc)) + bias[j]) % N for j in range(len(bias))]
        want = [sum(wi * xi[s] for wi, xi in zip(ws, x)) + beta for s in range(count)]
        assert slots.decode(res, N, b, count, engine=eng) == want


def test_encrypt_is_the_pow_formula():
    eng = SlotsEngine()
    rng = random.Random(47)
    n2 = N * N
    h_s = rng.randrange(2, n2)
    rz = FastRandomizer(N, h_s, exp_bits=70, engine=eng)
    b = 16
    k = packing.slots_per_ciphertext(N, b)
    vals = [rng.randint(-(1 << 15), (1 << 15) - 1) for _ in range(2 * k + 1)]
    exps = [rng.getrandbits(70) for _ in range(3)]
    plain = definition(vals, N, b)
    want = [(1 + p * N) * pow(h_s, a, n2) % n2 for p, a in zip(plain, exps)]
    assert slots.encrypt(vals, rz, b, exponents=exps) == want
    # the host draw: exponents from the byte source, one per packed plaintext
    drawn = []
    rz2 = FastRandomizer(N, h_s, exp_bits=70, engine=eng, urandom=lambda nb: drawn.append(nb) or bytes(range(nb)))
    got = slots.encrypt(vals, rz2, b)
    assert drawn == [3 * 9]
    a = [int.from_bytes(bytes(range(27))[i * 9 : (i + 1) * 9], "little") & ((1 << 70) - 1) for i in range(3)]
    assert got == [(1 + p * N) * pow(h_s, e, n2) % n2 for p, e in zip(plain, a)]
    with pytest.raises(ValueError):
        slots.encrypt(vals, rz, b, exponents=exps[:2])
    assert slots.encrypt([], rz, b) == []


class _Result:
    def __init__(self, value):
        self.value = value


class _Scheme:
    """Decrypts by table: what _decrypt_sequence_raw needs to be for decrypt_sequence_slots."""

    def __init__(self, n, table, receiver=True):
        self.public_key = type("PK", (), {"n": n})()
        self.table, self.receiver, self.seen = table, receiver, []

    async def _decrypt_sequence_raw(self, cts, receivers=None):
        self.seen.append([int(c.get_value()) for c in cts])
        return [_Result(self.table[int(c.get_value())]) for c in cts] if self.receiver else None


def test_decrypt_sequence_slots_decodes_without_packing():
    eng = SlotsEngine()
    b = 12
    k = packing.slots_per_ciphertext(N, b)
    vals = [((-1) ** i) * (i % 2000) for i in range(2 * k + 7)]
    plain = slots.encode(vals, N, b, engine=eng)
    cts = [1000 + j for j in range(len(plain))]                       # stand-ins: the scheme decrypts by table
    sch = _Scheme(N, dict(zip(cts, plain)))
    assert asyncio.run(slots.decrypt_sequence_slots(sch, cts, b, len(vals), engine=eng)) == vals
    assert sch.seen == [cts]                                          # the ciphertexts as they are: no pack step
    assert asyncio.run(slots.decrypt_sequence_slots(_Scheme(N, dict(zip(cts, plain)), receiver=False), cts, b, len(vals),
                                                    receivers=["other"], engine=eng)) is None
    assert asyncio.run(slots.decrypt_sequence_slots(sch, [], b, 0, engine=eng)) == []
