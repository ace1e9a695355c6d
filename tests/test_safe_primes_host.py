"""Host side of the safe-prime search (primes.py, PaillierPrivateKey.generate / check_primes with safe=True) and the model
the GPU tests compare against (tools/mr_model.py): the model's joint sieve against the two-residue definition, its verdict
against an independent pow-based test, the forced bits, the density formula and the default batch, the host decisions of
is_safe_prime_batch, and the safe=True paths over the model's engine (tests/safe_engine.py).  No GPU."""

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
from safe_engine import FakeRng, SafeEngine  # noqa: E402
from test_primes_host import counted_draws  # noqa: E402

from protocols.distributed_keygen_amd import DeviceRng, PaillierPrivateKey, limbs, primes, synthetic  # noqa: E402


def host_prime(n):
    return synthetic.is_probable_prime(n, random.Random(1))


def host_safe(p):
    return p % 2 == 1 and host_prime(p) and host_prime((p - 1) // 2)


def no_draw(count, bits, row_words=0):
    raise AssertionError("nothing should reach the random rounds")


# ------------------------------------------------------------------ the model
def test_model_sieve_is_the_two_residue_definition():
    rng = random.Random(5)
    plist = mm.odd_primes_below(mm.SIEVE_BOUND)
    assert len(plist) == 1899 and plist == primes.sieve_primes()
    hit = 0
    for _ in range(2000):
        h = rng.getrandbits(96)
        want = any(h % l == 0 or h % l == (l - 1) // 2 for l in plist)
        assert mm.safe_sieve_hit(h) == want, h
        hit += want
    assert 1900 < hit < 2000                              # about 0.9 % pass
    for l in (3, 5, 16381):
        assert mm.safe_sieve_hit(l) and mm.safe_sieve_hit((l - 1) // 2) and mm.safe_sieve_hit(7 * l) and mm.safe_sieve_hit((9 * l - 1) // 2)


def test_model_verdict_against_pow():
    """Every odd h below 2^16 shifted above the sieve bound, and the safe primes the model finds at 61 and 64 bits."""
    base = 1 << 20
    halves = [base + h for h in range(1, 1 << 16, 2)]
    got = mm.safe_prime(halves, 22, 6, mm.chacha_draws(bytes(range(32))))
    want = [host_prime(h) and host_prime(2 * h + 1) for h in halves]
    assert got == want and sum(want) > 100                # the density formula predicts about 410
    for bits in (61, 64):
        found, verdicts = mm.safe_prime_search(3, bits, mm.chacha_draws(bytes([bits]) * 32), 5, 2048)
        assert len(found) == 3 and all(host_safe(p) and p.bit_length() == bits for p in found)
        again, _ = mm.safe_prime_search(3, bits, mm.chacha_draws(bytes([bits]) * 32), 5, 2048)
        assert again == found
        halves = [mm.force_half_bits(r, bits) for r in mm.chacha_draws(bytes([bits]) * 32)(2048, bits - 1, (bits + 31) // 32)]
        assert [host_safe(2 * h + 1) for h in halves] == verdicts[0]
    psp = mm.pseudoprime_half()                            # a composite the base 2 keeps: it must fall later
    assert mm.base2(psp) and not host_prime(psp)
    stages = mm.safe_prime_stages([psp], 64, 8, mm.chacha_draws(bytes(32)))
    assert stages[0] == [0] and stages[1] == [0] and stages[3] == []


def test_pocklington_leaves_no_random_round_for_p():
    """h prime, 3 not dividing p = 2h + 1: the base 2 on p alone decides p, for every such h of 20 bits."""
    checked = 0
    for h in range((1 << 19) + 1, (1 << 19) + 40000, 2):
        if host_prime(h) and (2 * h + 1) % 3:
            assert mm.base2(2 * h + 1) == host_prime(2 * h + 1), h
            checked += 1
    assert checked > 500


@pytest.mark.parametrize("bits", [16, 63, 64, 65, 256, 1024])
def test_forced_bits_give_the_width(bits):
    rng = random.Random(bits)
    for row in [0, (1 << (bits - 1)) - 1] + [rng.getrandbits(bits - 1) for _ in range(20)]:
        h = mm.force_half_bits(row, bits)
        p = 2 * h + 1
        assert h.bit_length() == bits - 1 and p.bit_length() == bits and p >> (bits - 2) == 3 and p % 4 == 3
    a, b = 2 * mm.force_half_bits(0, bits) + 1, 2 * mm.force_half_bits((1 << (bits - 1)) - 1, bits) + 1
    assert (a * a).bit_length() == (b * b).bit_length() == 2 * bits


# ------------------------------------------------------------------ density and batch
@pytest.mark.parametrize("bits,found,predicted", [(64, 276, 277), (128, 142, 136), (256, 24, 25)])
def test_density_against_the_counts(bits, found, predicted):
    """Counts of safe primes among random draws against the formula: draws = predicted / density, and the
    count lies within three Poisson deviations of the mean the formula gives."""
    density = primes.safe_prime_density(bits)
    assert density == pytest.approx(4 * 0.6601618 / ((bits - 1) * math.log(2)) ** 2, rel=1e-6)
    draws = predicted / density
    mean = draws * density
    assert abs(found - mean) <= 3 * math.sqrt(mean)
    assert primes.safe_prime_density(1024) == pytest.approx(1 / 190000, rel=0.02)


@pytest.mark.parametrize("bits", [64, 256, 512, 1024, 1536, 4096])
@pytest.mark.parametrize("count", [1, 2, 6, 128])
def test_default_safe_batch(bits, count):
    batch = primes.default_safe_batch(count, bits)
    row_bytes = 4 * limbs.limbs_for_bits(bits)
    assert batch % 64 == 0 and 64 <= batch and batch * row_bytes <= primes.SAFE_BATCH_BYTES
    mean = batch * primes.safe_prime_density(bits)
    shortfall = sum(math.exp(-mean + k * math.log(mean) - math.lgamma(k + 1)) for k in range(count))
    capped = (batch + 64) * row_bytes > primes.SAFE_BATCH_BYTES
    assert capped or shortfall <= 0.02                    # Poisson's rule wherever the cap does not bind
    if bits >= 1024:
        assert capped
    for bad in ((0, 64), (1, 2)):
        with pytest.raises(ValueError):
            primes.default_safe_batch(*bad)


# ------------------------------------------------------------------ the public layer
def test_host_decisions_need_no_engine():
    vals = [5, 7, 11, 23, 47, 13, 17, 2, 1, 0, -7, 3, 9, 59, 83, 107, 2879, 2903, 16381 * 16369, 16382]
    want = [True] * 5 + [False] * 8 + [True] * 5 + [False] * 2
    assert [host_safe(p) for p in vals[13:]] == want[13:]
    assert primes.is_safe_prime_batch(vals, engine=object()) == want
    small = list(range(-3, 4000))
    assert primes.is_safe_prime_batch(small, engine=object()) == [
        p >= 5 and all(p % k for k in range(2, math.isqrt(p) + 1)) and all(((p - 1) // 2) % k for k in range(2, math.isqrt((p - 1) // 2) + 1))
        and p % 2 == 1 for p in small]
    big_1_mod_4 = 2**61 - 1 + 2                            # 1 mod 4 above the host's range: its half is even
    assert big_1_mod_4 % 4 == 1 and primes.is_safe_prime_batch([big_1_mod_4, 2**64], engine=object()) == [False, False]
    assert primes.is_safe_prime_batch([]) == []
    with pytest.raises(ValueError):
        primes.is_safe_prime_batch([5], rounds=0)


def test_device_decisions_over_the_model_engine():
    eng = SafeEngine()
    found, _ = mm.safe_prime_search(2, 64, mm.chacha_draws(bytes(32)), 5, 2048)
    half_only = next(p for p in range(2**40 + 3, 2**41, 4) if host_prime((p - 1) // 2) and not host_prime(p))
    full_only = next(p for p in range(2**40 + 3, 2**41, 4) if host_prime(p) and not host_prime((p - 1) // 2))
    vals = [found[0], 23, half_only, full_only, found[1], found[0] + 4, 2 * mm.pseudoprime_half() + 1]
    assert primes.is_safe_prime_batch(vals, rounds=6, rng=FakeRng(2), engine=eng) == [True, True, False, False, True, False, False]
    device = [p for p in vals if p != 23]                                 # 23 is decided on the host
    left = [len(stage) for stage in mm.safe_prime_stages([(p - 1) // 2 for p in device], limbs.max_bits(device), 6, mm.chacha_draws(bytes(32)))]
    assert 6 > left[0] >= left[1] >= left[2] >= 3                         # the pseudoprime half reaches the random rounds
    assert eng.calls == [("safe_prime", 6, 6), ("safe_sieve", 6), ("base2", left[0]), ("safe_double", left[1]), ("base2", left[1]),
                         ("generator_shares", left[2], 6), ("miller_rabin", left[2], 6)]


def test_shipped_search_equals_the_model():
    """The comparison the end-to-end run makes on the device: the shipped safe-prime search over the kernels' models."""
    key = bytes(range(32))
    eng = SafeEngine()
    rng = DeviceRng(key, first_call=3)
    draw, asked = counted_draws(key, 3)
    want, verdicts = mm.safe_prime_search(2, 64, draw, 4, 2048)
    assert _ints(eng.safe_prime_search_t(2, 64, rng, rounds=4, batch=2048)) == want and rng.next_call == 3 + len(asked)
    assert all(host_safe(p) for p in want)
    assert eng.calls[0] == ("safe_prime_search", 2, 64, 2048) and [c[0] for c in eng.calls if c[0] in MARKERS] == ["safe_prime_search"]
    assert [c for c in eng.calls if c[0] == "safe_sieve"] == [("safe_sieve", 2048)] * len(verdicts)
    assert [c for c in eng.calls if c[0] == "generator_shares"] == [("generator_shares", count // 4, 4) for count, bits in asked if bits == 63 + 64]
    assert [c for c in eng.calls if c[0] == "safe_double"][-1] == ("safe_double", sum(verdicts[-1]))      # 2h + 1 of what the last batch kept


def test_shipped_stages_equal_the_model():
    """safe_prime_t stage by stage on halves of every kind that passes the joint sieve, a composite that passes both rounds
    to the base 2, and random halves, most of which the sieve drops: every stage leaves something and drops something."""
    bits, rounds, key = 64, 3, bytes([64]) * 32
    kinds = mm.safe_cases(bits)
    rnd = random.Random(bits)
    psp = mm.pseudoprime_half()
    assert mm.base2(psp) and mm.base2(2 * psp + 1) and not host_prime(psp) and not mm.safe_sieve_hit(psp)
    halves = [h for kind in mm.SAFE_KINDS for h in kinds[kind]] + [psp] + [mm.force_half_bits(rnd.getrandbits(bits - 1), bits) for _ in range(8)]
    rnd.shuffle(halves)
    draw, asked = counted_draws(key, 5)
    want = mm.safe_prime_stages(halves, bits, rounds, draw)
    left = [len(stage) for stage in want]
    assert len(halves) > left[0] > left[1] > left[2] > left[3] >= 1 and asked == [(left[2] * rounds, bits - 1 + 64)]
    eng, rng, stages = SafeEngine(), DeviceRng(key, first_call=5), []
    got = eng.safe_prime_t(eng.to_device(limbs.pack(halves, 2)), bits, rounds, rng, _stages=stages)
    assert [stage.tolist() for stage in stages] == want
    assert got.tolist() == [int(i in want[3]) for i in range(len(halves))] and rng.next_call == 6
    assert eng.calls == [("safe_prime", len(halves), rounds), ("safe_sieve", len(halves)), ("base2", left[0]), ("safe_double", left[1]),
                         ("base2", left[1]), ("generator_shares", left[2], rounds), ("miller_rabin", left[2], rounds)]
    # nothing past the base 2 on h: no draw, no call number taken
    del eng.calls[:]
    composite = kinds["full"] + kinds["neither"]
    assert eng.safe_prime_t(eng.to_device(limbs.pack(composite, 2)), bits, rounds, rng).tolist() == [0] * len(composite)
    assert eng.calls == [("safe_prime", len(composite), rounds), ("safe_sieve", len(composite)), ("base2", len(composite))] and rng.next_call == 6
    # nothing past the base 2 on p
    del eng.calls[:]
    assert eng.safe_prime_t(eng.to_device(limbs.pack(kinds["half"], 2)), bits, rounds, rng).tolist() == [0] * len(kinds["half"])
    assert [c[0] for c in eng.calls] == ["safe_prime", "safe_sieve", "base2", "safe_double", "base2"] and rng.next_call == 6


def test_argument_checks_reach_no_engine():
    eng = SafeEngine()
    for bad in (63, 129, 0, -128, 32):
        with pytest.raises(ValueError):
            PaillierPrivateKey.generate(bad, rng=FakeRng(1), engine=eng, safe=True)
    with pytest.raises(ValueError):
        PaillierPrivateKey.generate(128, rng=FakeRng(1), rounds=0, engine=eng, safe=True)
    with pytest.raises(ValueError):
        PaillierPrivateKey.generate_batch(-1, 128, rng=FakeRng(1), engine=eng, safe=True)
    assert PaillierPrivateKey.generate_batch(0, 128, rng=FakeRng(1), engine=eng, safe=True) == []
    with pytest.raises(ValueError):
        primes.random_safe_primes(-1, 64, rng=FakeRng(1), engine=eng)
    assert primes.random_safe_primes(0, 64, rng=FakeRng(1), engine=eng) == []
    with pytest.raises(ValueError):
        primes.safe_prime_density(2)
    assert eng.calls == []
    rng = FakeRng(1)
    rows_t = lambda values: eng.to_device(limbs.pack(values, 2))
    for call in (lambda: eng.safe_prime_search_t(1, 8, rng), lambda: eng.safe_prime_search_t(1, 64, rng, rounds=0),
                 lambda: eng.safe_prime_t(rows_t([2**61 - 1]), 64, 0, rng), lambda: eng.safe_prime_t(rows_t([2**61 - 1]), 65, 4, rng),
                 lambda: eng.safe_prime_t(rows_t([2**61]), 64, 4, rng), lambda: eng.safe_prime_t(rows_t([8191]), 64, 4, rng),
                 lambda: eng.safe_double_t(rows_t([2**63])), lambda: eng.safe_sieve_t(rows_t([5]), [3, 9, 4])):
        with pytest.raises(ValueError):
            call()
    assert eng.calls == [] and rng.calls == []


def test_double_of_the_kernels():
    eng = SafeEngine()
    vals = [0, 1, 2**63 - 1, 2**31, 0x8000000080000000 >> 1]
    assert _ints(eng.safe_double_t(eng.to_device(limbs.pack(vals, 2)))) == [2 * h + 1 for h in vals]
    assert eng.safe_sieve_t(eng.to_device(limbs.pack([15, 7, 17, 8], 2)), [3, 5]).tolist() == [1, 1, 1, 0]          # 7 = (15 - 1) / 2, 17 = 2 mod 5 = (5 - 1) / 2


@pytest.mark.parametrize("key_length", [128, 192])
def test_generate_safe_over_the_model_engine(key_length):
    eng = SafeEngine()
    key = PaillierPrivateKey.generate(key_length, rng=FakeRng(key_length), rounds=6, engine=eng, safe=True)
    assert key.p.bit_length() == key.q.bit_length() == key_length // 2
    assert key.n.bit_length() == key_length and key.p != key.q
    assert host_safe(key.p) and host_safe(key.q) and math.gcd(key.n, (key.p - 1) * (key.q - 1)) == 1
    assert eng.calls[0] == ("safe_prime_search", 2, key_length // 2, primes.default_safe_batch(2, key_length // 2))
    assert key.check_primes(rounds=6, rng=FakeRng(9), safe=True) is True and key.check_primes(rounds=6, rng=FakeRng(9)) is True
    msgs = [0, 1, key.n - 1, 123456789]
    assert key.decrypt_batch(key.encrypt_batch(msgs, rng=FakeRng(4))) == msgs


def test_generate_batch_safe_takes_one_search_and_the_default_stays():
    eng = SafeEngine()
    keys = PaillierPrivateKey.generate_batch(2, 128, rng=FakeRng(2), rounds=4, engine=eng, safe=True)
    assert [c[0] for c in eng.calls if c[0] in MARKERS] == ["safe_prime_search"] and eng.calls[0][1] == 4
    found = [x for k in keys for x in (k.p, k.q)]
    assert len(set(found)) == 4 and all(host_safe(x) and x.bit_length() == 64 for x in found)
    # without the flag: the ordinary search, the same primes as an engine without the safe-prime methods finds
    from mr_engine import MrEngine

    plain = PaillierPrivateKey.generate(128, rng=FakeRng(7), rounds=4, engine=SafeEngine())
    before = PaillierPrivateKey.generate(128, rng=FakeRng(7), rounds=4, engine=MrEngine())
    assert (plain.p, plain.q) == (before.p, before.q)


def test_check_primes_safe_refuses_ordinary_primes():
    eng = SafeEngine()
    ordinary = PaillierPrivateKey(2**89 - 1, 2**107 - 1, engine=eng)
    assert ordinary.check_primes(rounds=4, rng=FakeRng(1)) is True
    assert ordinary.check_primes(rounds=4, rng=FakeRng(1), safe=True) is False
    found, _ = mm.safe_prime_search(2, 64, mm.chacha_draws(bytes(32)), 5, 2048)
    mixed = PaillierPrivateKey(found[0], 2**89 - 1, engine=eng)
    assert mixed.check_primes(rounds=4, rng=FakeRng(1), safe=True) is False
    assert PaillierPrivateKey(found[0], found[1], engine=eng).check_primes(rounds=4, rng=FakeRng(1), safe=True) is True
