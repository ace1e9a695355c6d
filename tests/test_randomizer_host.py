"""Host logic of the fixed-base randomiser (protocols/distributed_keygen_amd/randomizer.py) on the CPU, with a
pure-Python double of the engine's fixed_base_* calls: every expected value comes from CPython's pow."""

from __future__ import annotations

import json
import random
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle
from protocols.distributed_keygen_amd import homomorphic, packing, randomizer, synthetic

GOLDEN = Path(__file__).resolve().parent / "golden"


def unhex(s):
    return -int(s[1:], 16) if s.startswith("-") else int(s, 16)


def exponent_ints(exps):
    """Exponent rows (uint32 little-endian words) or ints -> ints."""
    if isinstance(exps, np.ndarray):
        return [int.from_bytes(np.ascontiguousarray(row, dtype="<u4").tobytes(), "little") for row in exps]
    return [int(e) for e in exps]


class TodayEngine:
    """The int-level ciphertext functions with the signatures they had before the randomiser existed (no keyword for
    it): what homomorphic.* and packing.pack must keep calling when no randomizer is given."""

    def ciphertext_scale_batch(self, cts, scalars, n):
        return [pow(c, k, n * n) for c, k in zip(cts, scalars)]

    def mulmod_batch(self, a, b, mod):
        return [x * y % mod for x, y in zip(a, b)]

    def modinv_batch(self, values, mod):
        return [pow(v, -1, mod) for v in values]

    def ciphertext_sum_batch(self, groups, n):
        out = []
        for g in groups:
            acc = 1
            for c in g:
                acc = acc * c % (n * n)
            out.append(acc)
        return out

    def ciphertext_linear_map_batch(self, cts, weights, n, bias=None):
        n2 = n * n
        out = []
        for j, row in enumerate(weights):
            items = row.items() if isinstance(row, dict) else enumerate(row)
            acc = 1 + ((bias[j] % n) * n if bias is not None else 0)
            for i, w in items:
                acc = acc * pow(cts[i], w, n2) % n2
            out.append(acc % n2)
        return out

    def ciphertext_pack_batch(self, cts, n, slot_bits, slots):
        n2 = n * n
        out = []
        for j in range(0, len(cts), slots):
            acc = 1
            for i, c in enumerate(cts[j : j + slots]):
                acc = acc * pow(c % n2, 1 << (slot_bits * i), n2) % n2
            out.append(acc)
        return out


class PyFixedBaseEngine(TodayEngine):
    """Engine.fixed_base_*_batch, powmod_nsquare_batch and the `fixed_base` keyword over Python ints."""

    def __init__(self):
        self.calls = []

    def powmod_nsquare_batch(self, bases, exp, n):
        return [pow(b, exp, n * n) for b in bases]

    def _powers(self, exps, n, base, exp_bits):
        vals = exponent_ints(exps)
        assert all(0 <= e < 1 << exp_bits for e in vals)
        return [pow(base, e, n * n) for e in vals]

    def fixed_base_power_batch(self, exponents, n, base, exp_bits, window=0):
        self.calls.append(("power", len(exponents), exp_bits, window))
        return self._powers(exponents, n, base, exp_bits)

    def fixed_base_encrypt_batch(self, messages, exponents, n, base, exp_bits, window=0):
        self.calls.append(("encrypt", len(messages), exp_bits, window))
        return [(1 + (m % n) * n) * h % (n * n) for m, h in zip(messages, self._powers(exponents, n, base, exp_bits))]

    def fixed_base_randomize_batch(self, ciphertexts, exponents, n, base, exp_bits, window=0):
        self.calls.append(("randomize", len(ciphertexts), exp_bits, window))
        return [c % (n * n) * h % (n * n) for c, h in zip(ciphertexts, self._powers(exponents, n, base, exp_bits))]

    def _fresh(self, values, fixed_base):
        if fixed_base is None:
            return values
        n, base, exp_bits, window, exps = fixed_base
        assert len(exps) == len(values)
        return self.fixed_base_randomize_batch(values, exps, n, base, exp_bits, window)

    def ciphertext_scale_batch(self, cts, scalars, n, fixed_base=None):
        return self._fresh(super().ciphertext_scale_batch(cts, scalars, n), fixed_base)

    def mulmod_batch(self, a, b, mod, fixed_base=None):
        return self._fresh(super().mulmod_batch(a, b, mod), fixed_base)

    def modinv_batch(self, values, mod, fixed_base=None):
        return self._fresh(super().modinv_batch(values, mod), fixed_base)

    def ciphertext_sum_batch(self, groups, n, fixed_base=None):
        return self._fresh(super().ciphertext_sum_batch(groups, n), fixed_base)

    def ciphertext_linear_map_batch(self, cts, weights, n, bias=None, fixed_base=None):
        return self._fresh(super().ciphertext_linear_map_batch(cts, weights, n, bias), fixed_base)

    def ciphertext_pack_batch(self, cts, n, slot_bits, slots, fixed_base=None):
        return self._fresh(super().ciphertext_pack_batch(cts, n, slot_bits, slots), fixed_base)


class ByteSource:
    """A deterministic stand-in for os.urandom that records what was asked of it."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.asked = []
        self.given = []

    def __call__(self, nbytes):
        self.asked.append(nbytes)
        raw = self.rng.randbytes(nbytes)
        self.given.append(raw)
        return raw


class FixedRng:
    def __init__(self, *values):
        self.values = list(values)

    def randrange(self, lo, hi):
        v = self.values.pop(0)
        assert lo <= v < hi
        return v


def test_generate_base_is_minus_y_squared_to_the_n():
    key = synthetic.make_key(128)
    n, n2 = key.n, key.n_square
    y = 0x1234567
    eng = PyFixedBaseEngine()
    assert randomizer.generate_base(n, rng=FixedRng(y), engine=eng) == pow((-y * y) % n, n, n2)
    with pytest.raises(ValueError):
        randomizer.generate_base(n, rng=FixedRng(key.p * 5), engine=eng)
    # without an injected rng: some unit's base, an N-th power whose Jacobi symbol modulo N is +1
    h_s = randomizer.generate_base(n, engine=eng)
    assert 0 < h_s < n2 and pow(h_s, (key.p - 1) * (key.q - 1), n2) == 1
    assert oracle.jacobi_symbol(h_s % n, n) == 1


def test_default_exp_bits_and_argument_checks():
    eng = PyFixedBaseEngine()
    for bits in (131, 132, 1027, 2050):
        n = random.Random(bits).getrandbits(bits) | (1 << (bits - 1)) | 1
        fr = randomizer.FastRandomizer(n, 5, engine=eng)
        assert fr.exp_bits == -(-bits // 2)
        assert randomizer.FastRandomizer(n, 5, exp_bits=bits + 64, engine=eng).exp_bits == bits + 64
        with pytest.raises(ValueError):
            randomizer.FastRandomizer(n, 5, exp_bits=0, engine=eng)
        with pytest.raises(ValueError):
            randomizer.FastRandomizer(n, 5, exp_bits=2 * bits + 65, engine=eng)
        with pytest.raises(ValueError):
            randomizer.FastRandomizer(n, 5, window=9, engine=eng)

    class Scheme:
        class public_key:
            n = 1000003 * 1000033

    assert randomizer.FastRandomizer.from_scheme(Scheme, 7, engine=eng).n == Scheme.public_key.n


def test_exponents_out_of_range_raise():
    key = synthetic.make_key(128)
    fr = randomizer.FastRandomizer(key.n, 5, exp_bits=20, engine=PyFixedBaseEngine())
    for bad in ([1 << 20], [-1], [3, 1 << 21]):
        with pytest.raises(ValueError):
            fr.encrypt([1] * len(bad), exponents=bad)
        with pytest.raises(ValueError):
            fr.randomize([1] * len(bad), exponents=bad)
        with pytest.raises(ValueError):
            fr.randomizers(len(bad), exponents=bad)
    with pytest.raises(ValueError):
        fr.encrypt([1, 2], exponents=[1])
    assert fr.encrypt([3], exponents=[(1 << 20) - 1]) == [(1 + 3 * key.n) * pow(5, (1 << 20) - 1, key.n_square) % key.n_square]


def test_get_value_is_called_once_per_distinct_object():
    key = synthetic.make_key(128)

    class Ct:
        def __init__(self, v):
            self.v, self.reads = v, 0

        def get_value(self):
            self.reads += 1
            return self.v

    a, b = Ct(11), Ct(12)
    fr = randomizer.FastRandomizer(key.n, 5, engine=PyFixedBaseEngine())
    out = fr.randomize([a, b, a, 13, a], exponents=[1, 2, 3, 4, 5])
    assert (a.reads, b.reads) == (1, 1)
    assert out == [v * pow(5, e, key.n_square) % key.n_square for v, e in zip([11, 12, 11, 13, 11], [1, 2, 3, 4, 5])]


@pytest.mark.parametrize("exp_bits", [1, 7, 8, 9, 31, 32, 33, 65, 515, 1024])
def test_drawn_exponents_use_exactly_the_bytes_they_need(exp_bits):
    key = synthetic.make_key(1024)
    src = ByteSource(exp_bits)
    eng = PyFixedBaseEngine()
    fr = randomizer.FastRandomizer(key.n, 5, exp_bits=exp_bits, engine=eng, urandom=src)
    count = 37
    nbytes = -(-exp_bits // 8)
    rows = fr.draw(count)
    assert src.asked == [count * nbytes]
    assert rows.dtype == np.dtype("<u4") and rows.shape == (count, -(-exp_bits // 32))
    vals = exponent_ints(rows)
    raw = src.given[0]
    want = [int.from_bytes(raw[i * nbytes : (i + 1) * nbytes], "little") & ((1 << exp_bits) - 1) for i in range(count)]
    assert vals == want and all(v < 1 << exp_bits for v in vals)
    if exp_bits > 8:
        assert any(v >> (exp_bits - 1) for v in vals)          # the top bit is in use
    # the three operations draw the same way: one string per call
    src.asked.clear()
    fr.randomizers(5)
    fr.encrypt([1, 2, 3])
    fr.randomize([4, 5])
    assert src.asked == [5 * nbytes, 3 * nbytes, 2 * nbytes]
    assert [c[:2] for c in eng.calls] == [("power", 5), ("encrypt", 3), ("randomize", 2)]


def _key_groups():
    groups = []
    for name, grp in json.loads((GOLDEN / "ref_keys.json").read_text()).items():
        groups.append((name, unhex(grp["n"]), grp["degree"], unhex(grp["n_fac"]), unhex(grp["theta_inv"]),
                       {int(i): unhex(v) for i, v in grp["shares"].items()}))
    for kl in (128, 1024):
        key = synthetic.make_key(kl)
        groups.append((f"synthetic{kl}", key.n, key.degree, key.n_fac, key.theta_inv, dict(key.shares)))
    return groups


@pytest.mark.parametrize("group", _key_groups(), ids=lambda g: g[0])
def test_fixed_base_encryptions_decrypt_to_their_messages(group):
    name, n, degree, n_fac, theta_inv, shares = group
    eng = PyFixedBaseEngine()
    rng = random.Random(name)
    h_s = randomizer.generate_base(n, rng=rng, engine=eng)
    fr = randomizer.FastRandomizer(n, h_s, engine=eng, urandom=ByteSource(name))
    messages = [0, 1, n - 1, -5, 424242]
    cts = fr.encrypt(messages)
    assert len(set(cts)) == len(cts)
    for m, c in zip(messages, cts):
        partials = {i: oracle.partial_decrypt(c, n, i, degree, n_fac, s) for i, s in shares.items()}
        assert oracle.decrypt_combine(partials, n, degree, theta_inv) == m % n, name
    # re-randomised: another ciphertext of the same plaintext
    again = fr.randomize(cts)
    assert all(a != c for a, c in zip(again, cts))
    partials = {i: oracle.partial_decrypt(again[4], n, i, degree, n_fac, s) for i, s in shares.items()}
    assert oracle.decrypt_combine(partials, n, degree, theta_inv) == 424242


def test_homomorphic_and_pack_are_unchanged_without_a_randomizer_and_fresh_with_one():
    key = synthetic.make_key(128)
    n, n2 = key.n, key.n_square
    rng = random.Random(9)
    cts = [synthetic.encrypt(key, m, rng) for m in (3, 1 << 20, 7, 11, 13, 0)]
    today, eng = TodayEngine(), PyFixedBaseEngine()
    h_s = randomizer.generate_base(n, rng=rng, engine=eng)
    weights = [[1, -2, 3, 0, 5, 1], {0: 4, 5: -1}]
    calls = {
        "scale": (homomorphic.scale, (cts, [2, -3, 0, 1, 5, 7]), {}),
        "add": (homomorphic.add, (cts[:3], cts[3:]), {}),
        "neg": (homomorphic.neg, (cts,), {}),
        "sum_groups": (homomorphic.sum_groups, ([cts[:2], [], cts[2:]],), {}),
        "linear_map": (homomorphic.linear_map, (cts, weights), {"bias": [5, -6]}),
        "pack": (packing.pack, (cts, 40), {}),
    }
    for name, (fn, args, kw) in calls.items():
        plain = fn(*args, n=n, engine=today, **kw)                  # the old signatures: no keyword reaches the engine
        assert fn(*args, n=n, engine=today, randomizer=None, **kw) == plain
        assert fn(*args, n=n, engine=eng, **kw) == plain
        src = ByteSource(name)
        fr = randomizer.FastRandomizer(n, h_s, engine=eng, urandom=src)
        fresh = fn(*args, n=n, engine=eng, randomizer=fr, **kw)
        nbytes = -(-fr.exp_bits // 8)
        assert src.asked == [len(plain) * nbytes], name
        exps = [int.from_bytes(src.given[0][i * nbytes : (i + 1) * nbytes], "little") & ((1 << fr.exp_bits) - 1)
                for i in range(len(plain))]
        assert fresh == [c * pow(h_s, a, n2) % n2 for c, a in zip(plain, exps)], name
    with pytest.raises(ValueError):
        homomorphic.neg(cts, n=n, engine=eng, randomizer=randomizer.FastRandomizer(n + 2, h_s, engine=eng))
