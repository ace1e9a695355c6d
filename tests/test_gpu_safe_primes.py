"""The safe-prime kernels (csrc/mx_sieve.hpp, csrc/mx_safe.hpp) and the search over them on the GPU — Engine.safe_sieve_t / safe_double_t /
safe_prime_t / safe_prime_search_t, primes.random_safe_primes / is_safe_prime_batch, PaillierPrivateKey.generate(...,
safe=True) / check_primes(safe=True) — every verdict bit for bit against tools/mr_model.py.

Joint sieve: per row width one list of 151 rows — directed rows for l in {3, 5, 16381} and a prime of the last, partly
padded block of 64 (h = 0 only, h = (l - 1) / 2 only, both through two primes, neither), all-ones rows, rows of
0x80000000 words, random rows behind them; batches are prefixes of the list.  The halves of 512 and 1024 bits of the
safe_prime_t cases are kept in tests/golden/safe_prime_cases.json (tools/mr_model.py safe 512 1024)."""

from __future__ import annotations

import json
import math
import random
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import mr_model as mm  # noqa: E402

BATCHES = (1, 7, 8, 9, 151)          # around SIEVE_C = 8 candidates per wavefront
ROWS = 151
WIDTHS = (2, 3, 16, 32, 64)          # words per row
MERSENNE31 = 2147483647


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def rows_of(eng, values, width):
    from protocols.distributed_keygen_amd import limbs

    return eng.to_device(limbs.pack(values, width))


def ints_of(eng, rows_t):
    from protocols.distributed_keygen_amd import limbs

    return limbs.unpack(eng.to_host(rows_t))


def flags_of(t):
    return [int(v) for v in t.cpu().numpy()]


def sieve_list():
    from protocols.distributed_keygen_amd import primes

    return primes.sieve_primes()


class Launches:
    """Counts the calls that reach the library while it is active."""

    def __init__(self, eng):
        self.eng, self.count = eng, 0

    def __enter__(self):
        inner = self.eng._call

        def counted(*args, **kwargs):
            self.count += 1
            return inner(*args, **kwargs)

        self.eng._call = counted
        return self

    def __exit__(self, *exc):
        del self.eng._call


# ------------------------------------------------------------------ the joint sieve
def hits(h, prime_list):
    """The two-residue definition: the primes that divide h, the primes that divide 2h + 1."""
    return [l for l in prime_list if h % l == 0], [l for l in prime_list if h % l == (l - 1) // 2]


def directed_rows(width, rng):
    """[(h, expected flag)]: per directed prime a row with h = 0 only, one with h = (l - 1) / 2 only and one with both
    through two different primes; then rows that no prime hits."""
    plist = sieve_list()
    assert len(plist) == 1899 == 29 * 64 + 43 and plist[-1] == 16381
    product = math.prod(plist)
    bits = 32 * width - 1
    directed = [3, 5, 16381, plist[29 * 64 + 5]]
    out = []
    for i, l in enumerate(directed):
        while True:                                   # l divides h and nothing else of the list divides h (2h + 1)
            h = l * (rng.getrandbits(bits - l.bit_length()) | 1)
            if math.gcd(h * (2 * h + 1), product) == l:
                break
        assert hits(h, plist) == ([l], [])
        out.append((h, 1))
        while True:                                   # l divides 2h + 1 and nothing else
            h = (l * (rng.getrandbits(bits - l.bit_length()) | 1) - 1) // 2
            if math.gcd(h * (2 * h + 1), product) == l:
                break
        assert hits(h, plist) == ([], [l])
        out.append((h, 1))
        l2 = directed[(i + 1) % len(directed)]        # l divides h, l2 divides 2h + 1
        k = (-pow(2 * l, -1, l2)) % l2 + l2 * rng.getrandbits(bits - l.bit_length() - l2.bit_length())
        h = l * k
        assert l in hits(h, plist)[0] and l2 in hits(h, plist)[1]
        out.append((h, 1))
    safe = mm.safe_cases(64)["safe"]                  # h and 2h + 1 both prime, in rows of any width
    out += [(h, 0) for h in safe]
    while len(out) < 3 * len(directed) + len(safe) + 4:          # full-width rows that nothing hits
        h = rng.getrandbits(bits) | 1
        if math.gcd(h * (2 * h + 1), product) == 1:
            out.append((h, 0))
    return out


_SIEVE_CASES = {}


def sieve_case(width):
    if width not in _SIEVE_CASES:
        rng = random.Random(width)
        rows = directed_rows(width, rng)
        vals = [h for h, _ in rows] + [(1 << (32 * width)) - 1, sum(0x80000000 << (32 * j) for j in range(width))]
        vals += [rng.getrandbits(32 * width) for _ in range(ROWS - len(vals))]
        want = [int(mm.safe_sieve_hit(h)) for h in vals]
        assert want[: len(rows)] == [flag for _, flag in rows]
        _SIEVE_CASES[width] = (vals, want)
    return _SIEVE_CASES[width]


def test_model_sieve_is_the_two_residue_definition():
    vals, want = sieve_case(3)
    plist = sieve_list()
    assert want == [int(any(hits(h, plist))) for h in vals]
    assert 0 < sum(want) < len(want)


@pytest.mark.parametrize("width", WIDTHS)
def test_joint_sieve_against_the_model(eng, width):
    vals, want = sieve_case(width)
    for rows in BATCHES:
        got = flags_of(eng.safe_sieve_t(rows_of(eng, vals[:rows], width), sieve_list()))
        assert got == want[:rows], (width, rows)


@pytest.mark.parametrize("width", WIDTHS)
def test_joint_sieve_is_the_two_plain_sieves(eng, width):
    rng = random.Random(1000 + width)
    halves = [rng.getrandbits(32 * width - 1) for _ in range(ROWS)]          # 2h + 1 fits the width
    halves[:2] = [(1 << (32 * width - 1)) - 1, sum(0x80000000 << (32 * j) for j in range(width - 1))]
    joint = flags_of(eng.safe_sieve_t(rows_of(eng, halves, width), sieve_list()))
    low = flags_of(eng.sieve_t(rows_of(eng, halves, width), sieve_list()))
    high = flags_of(eng.sieve_t(rows_of(eng, [2 * h + 1 for h in halves], width), sieve_list()))
    assert joint == [a | b for a, b in zip(low, high)]


def test_joint_sieve_with_a_prime_next_to_2_31(eng):
    """[3, 2^31 - 1] at 64 words: a fold after every limb (chunk = 1) and the bound of 2x + 1 at its extreme."""
    rng = random.Random(31)
    plist, width, l = [3, MERSENNE31], 64, MERSENNE31
    vals = []
    for _ in range(12):
        k = rng.getrandbits(32 * width - 33)
        vals += [k * l, k * l + (l - 1) // 2]
    vals += [(1 << (32 * width)) - 1, sum(0x80000000 << (32 * j) for j in range(width)), l, (l - 1) // 2, l - 1, 0, 1]
    vals += [rng.getrandbits(32 * width) for _ in range(ROWS - len(vals))]
    want = [int(any(hits(h, plist))) for h in vals]
    assert all(want[:24]) and 0 < sum(want) < len(want)
    for rows in (9, ROWS):
        assert flags_of(eng.safe_sieve_t(rows_of(eng, vals[:rows], width), plist)) == want[:rows]
    only = [int(any(hits(h, [l]))) for h in vals]          # the large prime alone, and in a list of one block
    assert flags_of(eng.safe_sieve_t(rows_of(eng, vals, width), [l])) == only


# ------------------------------------------------------------------ doubling
@pytest.mark.parametrize("width", (1, 2, 3, 16, 64))
def test_doubling(eng, width):
    top = 32 * width - 1
    rng = random.Random(width)
    vals = [sum(0x80000000 << (32 * j) for j in range(width - 1)),          # a carry out of every word below the top one
            (1 << top) - 1, 1, 0, 1 << (top - 1), (1 << (top - 1)) | 1]
    vals += [1 << k for k in range(0, top, 31)] + [rng.getrandbits(top) for _ in range(40)]
    assert any(h.bit_length() == top for h in vals)                          # exactly 32 * limbs - 1 bits: accepted
    assert ints_of(eng, eng.safe_double_t(rows_of(eng, vals, width))) == [2 * h + 1 for h in vals]
    with Launches(eng) as seen:
        with pytest.raises(ValueError):
            eng.safe_double_t(rows_of(eng, [5, 1 << top, 7], width))
    assert seen.count == 0
    assert eng.safe_double_t(rows_of(eng, [], width)).shape == (0, width)


# ------------------------------------------------------------------ safe_prime_t
_PSEUDOPRIME = []


def prime_cases(bits):
    """Halves of every kind that passes the joint sieve, a composite that passes the base 2 as well, and random halves."""
    if not _PSEUDOPRIME:
        _PSEUDOPRIME.append(mm.pseudoprime_half())
    if bits >= 512:
        gold = json.loads((ROOT / "tests" / "golden" / "safe_prime_cases.json").read_text())["bits"][str(bits)]
        kinds = {k: [int(h, 16) for h in v] for k, v in gold.items()}
    else:
        kinds = mm.safe_cases(bits)
    for kind, vals in kinds.items():
        for h in vals:
            assert h.bit_length() == bits - 1 and not mm.safe_sieve_hit(h)
            assert (mm.round_passes(h, 2), mm.round_passes(2 * h + 1, 2)) == (kind in ("safe", "half"), kind in ("safe", "full"))
    rng = random.Random(bits)
    psp = _PSEUDOPRIME[0]          # a composite h the base-2 stage keeps: it falls at the base 2 on 2h + 1 or at the random bases
    assert mm.base2(psp) and psp.bit_length() <= 63 and not mm.safe_sieve_hit(psp)
    vals = [h for kind in mm.SAFE_KINDS for h in kinds[kind]] + [psp]
    vals += [mm.force_half_bits(rng.getrandbits(bits - 1), bits) for _ in range(24)]
    rng.shuffle(vals)
    return vals


@pytest.mark.parametrize("bits", (64, 65, 96, 512, 1024))
def test_safe_prime_stages_against_the_model(eng, bits):
    from protocols.distributed_keygen_amd import DeviceRng, limbs

    vals = prime_cases(bits)
    key, rounds = bytes([bits % 251]) * 32, 3
    want = mm.safe_prime_stages(vals, bits, rounds, mm.chacha_draws(key, 5))
    assert len(want[3]) >= 2 and len(want[0]) > len(want[1]) > len(want[2]) >= len(want[3])
    stages = []
    rng = DeviceRng(key, first_call=5)
    got = flags_of(eng.safe_prime_t(rows_of(eng, vals, limbs.limbs_for_bits(bits)), bits, rounds, rng, _stages=stages))
    assert [[int(i) for i in s.cpu()] for s in stages] == want
    assert got == [int(i in want[3]) for i in range(len(vals))]
    assert rng.next_call == 6


# ------------------------------------------------------------------ seeded searches
# (bits, batch, rounds, key whose first batch holds COUNT safe primes, key whose first batch does not): found by
# find_search_keys() below, asserted again by the model in the test
COUNT = 6
SEARCHES = [(64, 4096, 4, 1, 0), (256, 65536, 4, 1, 0)]


def search_key(seed):
    return bytes([seed]) * 32


def find_search_keys(bits, batch, rounds):      # pragma: no cover - how SEARCHES was made
    enough = short = None
    for seed in range(256):
        _, verdicts = mm.safe_prime_search(COUNT, bits, mm.chacha_draws(search_key(seed)), rounds, batch)
        if len(verdicts) == 1 and enough is None:
            enough = seed
        if len(verdicts) == 2 and short is None:
            short = seed
        if enough is not None and short is not None:
            return enough, short


@pytest.mark.parametrize("bits,batch,rounds,seed,batches", [(b, n, r, seed, k) for b, n, r, e, s in SEARCHES for seed, k in ((e, 1), (s, 2))])
def test_search_against_the_model(eng, bits, batch, rounds, seed, batches):
    from protocols.distributed_keygen_amd import DeviceRng

    key = search_key(seed)
    want, verdicts = mm.safe_prime_search(COUNT, bits, mm.chacha_draws(key), rounds, batch)
    assert len(verdicts) == batches                        # the second key takes the redraw path, once
    # the whole first batch, verdict by verdict: no safe prime missed, nothing else kept
    halves = [mm.force_half_bits(r, bits) for r in mm.chacha_draws(key)(batch, bits - 1, (bits + 31) // 32)]
    rng = DeviceRng(key, first_call=1)
    got = flags_of(eng.safe_prime_t(rows_of(eng, halves, (bits + 31) // 32), bits, rounds, rng))
    assert got == [int(v) for v in verdicts[0]]
    # the search itself: the first COUNT safe primes in draw order, exactly `bits` bits, top two bits set, 3 mod 4
    rng = DeviceRng(key)
    found = ints_of(eng, eng.safe_prime_search_t(COUNT, bits, rng, rounds=rounds, batch=batch))
    assert found == want and len(found) == COUNT
    assert all(p >> (bits - 2) == 3 and p % 4 == 3 for p in found)
    assert rng.next_call == sum(1 + int(any(v)) for v in verdicts)


def test_forced_bits_give_the_width():
    for bits in (16, 64, 65, 256):
        for row in (0, (1 << (bits - 1)) - 1):
            p = 2 * mm.force_half_bits(row, bits) + 1
            assert p.bit_length() == bits and p >> (bits - 2) == 3 and p % 4 == 3


# ------------------------------------------------------------------ keys
def host_safe(p):
    from protocols.distributed_keygen_amd import synthetic

    return p % 4 == 3 and synthetic.is_probable_prime(p, random.Random(1)) and synthetic.is_probable_prime((p - 1) // 2, random.Random(2))


def test_generated_safe_prime_keys_work(eng):
    from protocols.distributed_keygen_amd import PaillierPrivateKey, primes

    key = PaillierPrivateKey.generate(512, engine=eng, safe=True)
    (wide,) = primes.random_safe_primes(1, 1024, engine=eng)
    assert key.n.bit_length() == 512 and key.p != key.q
    for p, bits in ((key.p, 256), (key.q, 256), (wide, 1024)):
        assert p.bit_length() == bits and p >> (bits - 2) == 3 and host_safe(p)
    assert key.check_primes(safe=True) is True and key.check_primes() is True
    assert primes.is_safe_prime_batch([wide, wide + 4, key.p, 23, 13], rounds=8, engine=eng) == [True, False, True, True, False]
    rng = random.Random(3)
    msgs = [0, 1, key.n - 1, rng.randrange(key.n)]
    assert key.decrypt_batch(key.encrypt_batch(msgs)) == msgs
    # the golden keys' primes are ordinary ones: (p - 1) / 2 is composite for every one of them
    gold = json.loads((ROOT / "tests" / "golden" / "private_key_primes.json").read_text())["keys"]
    p, q = (int(gold["2048"][x], 16) for x in "pq")
    assert not host_safe(p) and not host_safe(q)
    plain = PaillierPrivateKey(p, q, engine=eng)
    assert plain.check_primes(rounds=4) is True and plain.check_primes(rounds=4, safe=True) is False
    assert PaillierPrivateKey(key.p, q, engine=eng).check_primes(rounds=4, safe=True) is False


def test_plain_generation_is_unchanged(eng):
    """generate(512) from a fixed key: the primes the model of the ordinary search finds, as before."""
    from protocols.distributed_keygen_amd import DeviceRng, PaillierPrivateKey, primes

    seed = bytes(range(32))
    key = PaillierPrivateKey.generate(512, rng=DeviceRng(seed), rounds=6, engine=eng)
    want, _ = mm.prime_search(2, 256, mm.chacha_draws(seed), 6, primes.default_batch(2, 256))
    assert [key.p, key.q] == want
    assert not host_safe(key.p) or not host_safe(key.q)


# ------------------------------------------------------------------ argument checks
def test_argument_checks_launch_nothing(eng):
    from protocols.distributed_keygen_amd import DeviceRng

    rng = DeviceRng(bytes(32))
    big = 2**61 - 1
    good = rows_of(eng, [big, 2**62 + 1], 3)
    with Launches(eng) as seen:
        for bad in ([big, 2**64], [1, big], [big, 0], [big, 8191]):          # even, below the sieve bound
            with pytest.raises(ValueError):
                eng.safe_prime_t(rows_of(eng, bad, 3), 96, 4, rng)
        for call in (lambda: eng.safe_prime_t(good, 63, 4, rng),               # halves of more than bits - 1 bits
                     lambda: eng.safe_prime_t(good, 97, 4, rng),               # p wider than the rows
                     lambda: eng.safe_prime_t(good, 2, 4, rng),
                     lambda: eng.safe_prime_t(good, 96, 0, rng),
                     lambda: eng.safe_prime_t(good.cpu().numpy(), 96, 4, rng),
                     lambda: eng.safe_sieve_t(good, []),
                     lambda: eng.safe_sieve_t(good, [3, 4]),
                     lambda: eng.safe_sieve_t(good, [3, 1]),
                     lambda: eng.safe_sieve_t(good, [3, 2**31 + 11]),
                     lambda: eng.safe_sieve_t(good[:, :2], [3]),               # not contiguous
                     lambda: eng.safe_double_t(rows_of(eng, [2**95], 3)),
                     lambda: eng.safe_prime_search_t(1, 8, rng),
                     lambda: eng.safe_prime_search_t(-1, 64, rng),
                     lambda: eng.safe_prime_search_t(1, 64, rng, rounds=0),
                     lambda: eng.safe_prime_search_t(1, 64, rng, batch=0)):
            with pytest.raises(ValueError):
                call()
        assert eng.safe_prime_search_t(0, 128, rng).shape == (0, 4)
        assert flags_of(eng.safe_prime_t(rows_of(eng, [], 3), 96, 4, rng)) == []
        assert flags_of(eng.safe_sieve_t(rows_of(eng, [], 3), [3, 5])) == []
    assert seen.count == 0 and rng.next_call == 0
    # the C entry points refuse the same, and more, by themselves
    lib, fake, three = eng.lib, 1 << 20, (__import__("ctypes").c_uint32 * 2)(3, 4)
    assert lib.mx_safe_sieve(fake, fake, three, 2, 3, 8, fake, 1 << 30, None) == -1          # an even "prime"
    assert lib.mx_safe_sieve(fake, fake, three, 1, 3, -1, fake, 1 << 30, None) == -1
    assert lib.mx_safe_sieve(fake, fake, three, 1, 0, 8, fake, 1 << 30, None) == -1
    assert lib.mx_safe_sieve(None, fake, three, 1, 3, 8, fake, 1 << 30, None) == -1
    assert lib.mx_safe_sieve(fake, fake, three, 1, 3, 8, fake, 8, None) == -4
    assert lib.mx_safe_sieve(fake, fake, three, 1, 3, 0, fake, 1 << 30, None) == 0             # nothing to do
    assert lib.mx_safe_sieve_workspace_bytes(3, 1899) == lib.mx_sieve_workspace_bytes(3, 1899) > 0
    assert lib.mx_safe_sieve_workspace_bytes(0, 5) == -1
    assert lib.mx_safe_double(fake, fake + 64, 0, 1, None) == -1 and lib.mx_safe_double(fake, fake, 3, 1, None) == -1
    assert lib.mx_safe_double(fake, None, 3, 1, None) == -1 and lib.mx_safe_double(fake, fake + 64, 3, -1, None) == -1
    assert lib.mx_safe_double(fake, fake + 64, 3, 0, None) == 0
