"""Host side of the prime search (primes.py, PaillierPrivateKey.generate / check_primes) and the model the GPU tests compare
against (tools/mr_model.py): the model against synthetic.is_probable_prime and against known strong pseudoprimes, the
host decisions of is_probable_prime_batch, the argument checks, key generation over the model's engine (tests/mr_engine.py)
and the default batch of the search against its Poisson bound.  No GPU."""

from __future__ import annotations

import math
import random
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import mr_model as mm  # noqa: E402
from crt_engine import MARKERS, _ints  # noqa: E402
from mr_engine import FakeRng, MrEngine  # noqa: E402

from protocols.distributed_keygen_amd import DeviceRng, PaillierPrivateKey, limbs, primes, synthetic  # noqa: E402

KNOWN_PRIMES = (3, 5, 7, 65537, 2**61 - 1, 2**64 - 2**32 + 1)
PSP = 3215031751          # the smallest strong pseudoprime to the bases 2, 3, 5 and 7 at once


def model_is_prime(n, bases):
    return all(mm.round_passes(n, b % n) for b in bases)


def test_split_is_exact():
    for n in (3, 5, 9, 17, 561, 2**32 + 1, 2**64 + 1, 3 * 2**70 + 1, 2**61 - 1):
        d, s = mm.split(n)
        assert d % 2 == 1 and s >= 1 and d << s == n - 1
    for bad in (1, 2, 4, -3, 0):
        with pytest.raises(ValueError):
            mm.split(bad)


def test_model_on_known_values():
    for p in KNOWN_PRIMES:
        for b in (2, 3, 5, 7, 11, p - 1, 1, 0):
            assert mm.round_passes(p, b % p), (p, b)
        assert mm.base2(p) and mm.base2(p, p.bit_length() + 37)
    # 561 = 3 * 11 * 17: 2^560 = 1 (a Fermat liar), yet 2^35 = 263, 2^70 = 166, 2^140 = 67, 2^280 = 1: a strong witness
    assert pow(2, 560, 561) == 1 and not mm.round_passes(561, 2) and not mm.base2(561)
    # 2047 = 23 * 89: 2^1023 = 1, a strong liar
    assert mm.round_passes(2047, 2) and mm.base2(2047) and mm.base2(2047, 64)
    for b in (2, 3, 5, 7):
        assert mm.round_passes(PSP, b)
    assert not mm.round_passes(PSP, 11)
    assert mm.base2(PSP)


def test_tail_cases():
    n = 13 * 2**5 + 1            # 417 = 3 * 139
    d, s = mm.split(n)
    assert (d, s) == (13, 5)
    assert mm.tail(n, 1, 5, s) and mm.tail(n, n - 1, 5, s)
    assert mm.tail(n, 7, 0, s) and mm.tail(n, 7, n, s)               # a vacuous round
    p = 97                       # 3 * 2^5 + 1, prime: a non-residue reaches -1 only at the last squaring that counts
    d, s = mm.split(p)
    b = next(b for b in range(2, p) if pow(b, (p - 1) // 2, p) == p - 1)
    x0 = pow(b, d, p)
    assert pow(x0, 2 ** (s - 1), p) == p - 1 and all(pow(x0, 2**i, p) != p - 1 for i in range(s - 1))
    assert mm.tail(p, x0, b, s) and not mm.tail(p, x0, b, s - 1)
    # only x^(2^s) == 1: a Fermat liar that is a strong witness must fail
    assert not mm.tail(561, pow(2, 35, 561), 2, 4)


def test_model_agrees_with_synthetic():
    rng = random.Random(11)
    for bits in (20, 33, 64, 100):
        for _ in range(150):
            n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
            bases = [rng.randrange(2, n - 1) for _ in range(12)]
            want = synthetic.is_probable_prime(n, random.Random(5))
            assert model_is_prime(n, bases) == want, n
            assert mm.base2(n) == mm.round_passes(n, 2)
            assert mm.base2(n, bits + 17) == mm.round_passes(n, 2)


def test_model_pipeline_is_reproducible_and_right():
    key = bytes(range(32))
    a, va = mm.prime_search(3, 64, mm.chacha_draws(key, 7), 8, 256)
    b, vb = mm.prime_search(3, 64, mm.chacha_draws(key, 7), 8, 256)
    assert a == b and va == vb and len(a) == 3
    for p in a:
        assert p.bit_length() == 64 and p >> 62 == 3 and synthetic.is_probable_prime(p, random.Random(1))
    cands = [mm.force_bits(r, 64) for r in mm.chacha_draws(key, 7)(256, 64, 2)]
    assert [synthetic.is_probable_prime(n, random.Random(1)) for n in cands] == va[0]


def test_host_decisions_need_no_engine():
    vals = [-7, -2, 0, 1, 2, 3, 4, 9, 15, 17, 25, 65537, 65536, 16381, 16381 * 16381, 16381 * 16369, 2**27 - 39, 10**8 + 7]
    want = [False, False, False, False, True, True, False, False, False, True, False, True, False, True, False, False, True, True]
    assert primes.is_probable_prime_batch(vals, engine=object()) == want
    small = list(range(-3, 3000))
    assert primes.is_probable_prime_batch(small, engine=object()) == [n >= 2 and all(n % k for k in range(2, math.isqrt(n) + 1)) for n in small]
    assert primes.is_probable_prime_batch([]) == []
    with pytest.raises(ValueError):
        primes.is_probable_prime_batch([5], rounds=0)


def test_device_decisions_over_the_model_engine():
    eng = MrEngine()
    big = [2**61 - 1, 2**64 - 2**32 + 1, (2**61 - 1) * (2**31 - 1), 2**89 - 1, 561 * (2**61 - 1), PSP * 2**33 + 1, (2**31 - 1) ** 2]
    vals = [7, 8] + big + [16381 * 16369]
    out = primes.is_probable_prime_batch(vals, rounds=16, rng=FakeRng(3), engine=eng)
    assert out == [True, False, True, True, False, True, False, synthetic.is_probable_prime(big[5], random.Random(2)), False, False]
    sieved = [n for n in big if not mm.sieve_hit(n)]                      # the stages of the model: each drops something
    left = [n for n in sieved if mm.base2(n)]
    assert len(big) > len(sieved) > len(left) >= 3
    assert eng.calls == [("probable_prime", len(big), 16), ("sieve", len(big)), ("base2", len(sieved)),
                         ("generator_shares", len(left), 16), ("miller_rabin", len(left), 16)]


def counted_draws(key, first_call):
    """(draw, asked): the model's draws of DeviceRng(key, first_call) and the list of what was asked of them."""
    draw, asked = mm.chacha_draws(key, first_call), []

    def counted(count, bits, row_words=0):
        asked.append((count, bits))
        return draw(count, bits, row_words)

    return counted, asked


def test_shipped_search_equals_the_model():
    """The comparison the end-to-end run makes on the device: the shipped search over the kernels' models, draw for draw —
    ONE draw of bases per batch with survivors, none otherwise."""
    key = bytes(range(32))
    eng = MrEngine()
    rng = DeviceRng(key, first_call=7)
    draw, asked = counted_draws(key, 7)
    want, verdicts = mm.prime_search(3, 64, draw, 8, 256)
    assert _ints(eng.prime_search_t(3, 64, rng, rounds=8, batch=256)) == want and rng.next_call == 7 + len(asked)
    assert eng.calls[0] == ("prime_search", 3, 64, 256) and [c[0] for c in eng.calls if c[0] in MARKERS] == ["prime_search"]
    assert [c for c in eng.calls if c[0] == "sieve"] == [("sieve", 256)] * len(verdicts)
    assert [c for c in eng.calls if c[0] == "generator_shares"] == [("generator_shares", count // 8, 8) for count, bits in asked if bits == 128]
    assert eng.prime_search_t(0, 64, rng).shape == (0, 2) and rng.next_call == 7 + len(asked)      # a search for nothing draws nothing


@pytest.mark.parametrize("words,bits", [(2, 33), (2, 63), (2, 64), (2, 32), (3, 33), (3, 63), (1, 32)])
def test_candidate_range_check(words, bits):
    """_mr_candidates: odd, at least `above`, at most `bits` bits — at widths that end inside a word, at a word boundary
    below the rows' width and at the rows' full width, where the top bit is the int32's sign."""
    eng = MrEngine()
    rows_t = lambda *values: eng.to_device(limbs.pack(list(values), words))
    top = (1 << bits) - 1
    for legal in (top, (1 << (bits - 1)) + 1, 0x80000001, 3):
        assert eng._mr_candidates(rows_t(legal, top), bits) == (2, words, bits)
    refused = [top - 1, 0x80000000, 1]                                   # even rows, a row below 3
    if bits < 32 * words:
        refused += [(1 << bits) | 1, (1 << (32 * words - 1)) | 1]       # one bit above `bits`; the rows' top bit, a sign
    if (bits + 31) // 32 < words:
        refused.append((1 << (32 * ((bits + 31) // 32))) | 1)            # a set word above the top word of `bits`
    for bad in refused:
        for rows in (rows_t(bad), rows_t(top, bad), rows_t(bad, top)):
            with pytest.raises(ValueError, match="odd, at least 3 and of at most"):
                eng._mr_candidates(rows, bits)
        assert eng._mr_candidates(rows_t(top, bad), bits, checked=True) == (2, words, bits)      # the caller made the rows
    above = primes.SIEVE_BOUND
    assert eng._mr_candidates(rows_t(above + 1), bits, above=above) == (1, words, bits)
    with pytest.raises(ValueError, match=f"at least {above}"):
        eng._mr_candidates(rows_t(top, above - 1), bits, above=above)
    for bad_bits in (1, 32 * words + 1):
        with pytest.raises(ValueError, match="bits must lie"):
            eng._mr_candidates(rows_t(top), bad_bits)
    assert eng._mr_candidates(rows_t(top), None) == (1, words, 32 * words)
    assert eng.calls == []


@pytest.mark.parametrize("bits", [32, 64])
def test_forced_bits_where_the_sign_of_the_word_lies(bits):
    """_force_bits sets bit 31 of a word as the int32 it is: positions 31 and 63, next to 30, 62 and 0, on rows that have
    the bits clear, set, and at random.  The rows read as unsigned are the model's."""
    rnd = random.Random(bits)
    eng = MrEngine()
    whole = [0, (1 << bits) - 1, 1 << (bits - 1), 1 << (bits - 2)] + [rnd.getrandbits(bits) for _ in range(12)]
    rows = eng._force_bits(eng.to_device(limbs.pack(whole, bits // 32)), (bits - 1, bits - 2, 0))
    assert rows.dtype == eng.torch.int32 and _ints(rows) == [mm.force_bits(r, bits) for r in whole]
    rows = eng._force_bits(eng.to_device(limbs.pack(whole, bits // 32)), (bits - 1, bits - 2, 0))      # the halves of bits + 1
    assert _ints(rows) == [mm.force_half_bits(r, bits + 1) for r in whole]
    for position in (0, 30, 31, bits - 1):
        rows = eng._force_bits(eng.to_device(limbs.pack(whole, bits // 32)), (position,))
        assert _ints(rows) == [r | (1 << position) for r in whole]


def test_generate_argument_checks():
    eng = MrEngine()
    for bad in (63, 129, 0, -128, 32):
        with pytest.raises(ValueError):
            PaillierPrivateKey.generate(bad, rng=FakeRng(1), engine=eng)
    with pytest.raises(ValueError):
        PaillierPrivateKey.generate(128, rng=FakeRng(1), rounds=0, engine=eng)
    with pytest.raises(ValueError):
        PaillierPrivateKey.generate_batch(-1, 128, rng=FakeRng(1), engine=eng)
    assert PaillierPrivateKey.generate_batch(0, 128, rng=FakeRng(1), engine=eng) == []
    assert eng.calls == []
    with pytest.raises(ValueError):
        primes.random_primes(-1, 64, rng=FakeRng(1), engine=eng)
    with pytest.raises(ValueError):
        eng.prime_search_t(1, 8, FakeRng(1))


@pytest.mark.parametrize("key_length", [128, 192])
def test_generate_over_the_model_engine(key_length):
    eng = MrEngine()
    key = PaillierPrivateKey.generate(key_length, rng=FakeRng(key_length), rounds=8, engine=eng)
    assert key.p.bit_length() == key.q.bit_length() == key_length // 2
    assert key.n.bit_length() == key_length and key.p != key.q
    assert synthetic.is_probable_prime(key.p, random.Random(1)) and synthetic.is_probable_prime(key.q, random.Random(1))
    assert eng.calls[0][:3] == ("prime_search", 2, key_length // 2)
    assert key.check_primes(rounds=8, rng=FakeRng(9)) is True
    msgs = [0, 1, key.n - 1, 123456789]
    assert key.decrypt_batch(key.encrypt_batch(msgs, rng=FakeRng(4))) == msgs


def test_generate_batch_takes_one_search():
    eng = MrEngine()
    keys = PaillierPrivateKey.generate_batch(3, 128, rng=FakeRng(2), rounds=4, engine=eng)
    assert [c[0] for c in eng.calls if c[0] in MARKERS] == ["prime_search"] and eng.calls[0][1] == 6
    found = [x for k in keys for x in (k.p, k.q)]
    assert len(set(found)) == 6 and all(x.bit_length() == 64 for x in found)


def test_check_primes_refuses_composites():
    eng = MrEngine()
    p = 2**89 - 1
    good = PaillierPrivateKey(p, 2**107 - 1, engine=eng)
    assert good.check_primes(rounds=4, rng=FakeRng(1))
    for bad_q in (PSP * (2**31 - 1), (2**31 - 1) * (2**61 - 1)):
        key = PaillierPrivateKey(p, bad_q, engine=eng)          # the constructor takes them: odd, coprime to (p-1)(q-1)
        assert key.check_primes(rounds=8, rng=FakeRng(1)) is False
    # a Carmichael factor: p - 1 must avoid 3, 11 and 17 for the constructor to take 561 r
    p2 = next(n for n in range(2**80 + 1, 2**80 + 10**5, 2)
              if n % 3 == 2 and n % 11 != 1 and n % 17 != 1 and synthetic.is_probable_prime(n, random.Random(3)))
    key = PaillierPrivateKey(p2, 561 * (2**61 - 1), engine=eng)
    assert key.check_primes(rounds=8, rng=FakeRng(1)) is False
    assert PaillierPrivateKey(561 * (2**61 - 1), p2, engine=eng).check_primes(rounds=8, rng=FakeRng(1)) is False
    small_bad = PaillierPrivateKey(2**61 - 1, 43 * 47, engine=eng)          # decided on the host
    calls = len([c for c in eng.calls if c[0] in MARKERS])
    assert small_bad.check_primes() is False and len([c for c in eng.calls if c[0] in MARKERS]) == calls + 1      # only p went to the engine


@pytest.mark.parametrize("bits", [512, 1024, 2048])
@pytest.mark.parametrize("count", [1, 2, 6, 128])
def test_default_batch_meets_its_bound(bits, count):
    batch = primes.default_batch(count, bits)
    mean = batch * 2.0 / (bits * math.log(2.0))
    shortfall = sum(math.exp(-mean + k * math.log(mean) - math.lgamma(k + 1)) for k in range(count))
    assert batch % 64 == 0 and shortfall <= 0.02
    # and not grossly more than needed: half of it would miss the bound
    half = mean / 2
    assert sum(math.exp(-half + k * math.log(half) - math.lgamma(k + 1)) for k in range(count)) > 0.02
