"""The strong-pseudoprime kernels (csrc/mx_mr.hpp) and the prime search over them on the GPU — Engine.mr_split_t /
miller_rabin_t / miller_rabin_base2_t / probable_prime_t / prime_search_t, primes.py, PaillierPrivateKey.generate /
check_primes — every verdict bit for bit against tools/mr_model.py.

Candidates: per width one list of 151 rows — a prime and a composite k 2^s + 1 for every shift s that crosses a limb or
a word boundary (found by the model; those of 512 bits and more are kept in tests/golden/mr_proth.json, finding them
takes a minute), semiprimes (2k+1)(4k+1) with bases the model finds to be strong liars next to witnesses, 561, 2047 and
3215031751, random odd numbers behind them.  Batches are prefixes of that list, bases the first G columns of one matrix
per width, so a reference is computed once per (row, column).  At most 151 rows per launch."""

from __future__ import annotations

import json
import random
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import hostpow  # noqa: E402
import mr_model as mm  # noqa: E402

BATCHES = (1, 2, 63, 64, 65, 151)
ROWS = 151
COLUMNS = 64
PSP = 3215031751
WIDTHS = (67, 512, 1024, 2048)          # lane groups of 1, 2, 4 and 8


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


_PROTH = {}


def proth(bits):
    """{s: (prime or 0, composite)} of exactly `bits` bits."""
    if bits not in _PROTH:
        if bits >= 512:
            gold = json.loads((ROOT / "tests" / "golden" / "mr_proth.json").read_text())["bits"][str(bits)]
            _PROTH[bits] = {int(s): tuple(int(v, 16) for v in pair) for s, pair in gold.items()}
        else:
            _PROTH[bits] = mm.proth_cases(bits)
        for s, (prime, composite) in _PROTH[bits].items():
            for n in (prime, composite):
                assert n == 0 or (n.bit_length() == bits and mm.split(n)[1] == s)
    return _PROTH[bits]


def round_passes(n, b):
    """mr_model.round_passes with the modexp through libgmp where the box has it (hostpow checks it against pow)."""
    d, s = mm.split(n)
    return mm.tail(n, hostpow.powmod(b, d, n), b, s)


def semiprimes(rng, count):
    """(2k+1)(4k+1) of about 64 bits with both factors prime: a quarter of the bases are strong liars."""
    out = []
    while len(out) < count:
        k = rng.getrandbits(30) | (1 << 29)
        p, q = 2 * k + 1, 4 * k + 1
        if all(mm.round_passes(p, b) and mm.round_passes(q, b) for b in (2, 3, 5, 7, 11, 13)):
            out.append(p * q)
    return out


def pick_base(rng, n, want):
    """A base in [2, n - 2] whose round the model classifies as `want`."""
    d, s = mm.split(n)
    for _ in range(4000):
        b = rng.randrange(2, n - 1)
        x0 = pow(b, d, n)
        passes = mm.tail(n, x0, b, s)
        kinds = {"one": x0 == 1, "minus": x0 == n - 1, "last": s > 1 and pow(x0, 1 << (s - 1), n) == n - 1, "liar": passes,
                 "fermat": not passes and pow(x0, 1 << s, n) == 1, "witness": not passes and pow(x0, 1 << s, n) != 1}
        if kinds[want]:
            return b
    return None


class Case:
    """The candidates of one width, their base matrix and the model's verdicts, computed on demand."""

    def __init__(self, bits):
        from protocols.distributed_keygen_amd import limbs

        self.bits = bits
        self.limbs = limbs.limbs_for_bits(bits)
        rng = random.Random(bits)
        cands = []
        for s, (prime, composite) in sorted(proth(bits).items()):
            cands += [n for n in (prime, composite) if n]
        if bits == 67:
            for width in (64, 65, 66):
                cands += [n for pair in mm.proth_cases(width).values() for n in pair if n][:8]
        semis = semiprimes(rng, 4)
        cands += semis + [561, 2047, PSP]
        cands += [rng.getrandbits(bits) | (1 << (bits - 1)) | 1 for _ in range(ROWS - len(cands))]
        cands = cands[:ROWS]
        assert len(cands) == ROWS and all(n % 2 and 3 <= n < 1 << bits for n in cands)
        self.cands = cands
        # the base matrix: random columns, then the directed entries
        self.bases = [[rng.randrange(0, n) for _ in range(COLUMNS)] for n in cands]
        self.kinds = set()
        for row, n in enumerate(cands):
            self.bases[row][0] = 2 % n
            self.bases[row][1] = (0, 1, n - 1)[row % 3]
        for n in semis:                                   # a liar next to witnesses, for the same composite
            row = cands.index(n)
            for col, want in ((0, "liar"), (1, "witness"), (2, "fermat"), (3, "liar")):
                b = pick_base(rng, n, want)
                if b is not None:
                    self.bases[row][col] = b
                    self.kinds.add(want)
        small = sorted(proth(bits).items())[:2]           # primes with s = 1 and s = 2: every way to pass
        for s, (prime, _) in small:
            row = cands.index(prime)
            for col, want in ((0, "minus"), (2, "last" if s > 1 else "minus"), (1, "one")):
                b = pick_base(rng, prime, want)
                if b is not None:
                    self.bases[row][col] = b
                    self.kinds.add(want)
        row = cands.index(561)
        self.bases[row][0], self.bases[row][2] = 2, 50     # 2^280 = 1 only: fails; 50^35 = 560: passes
        row = cands.index(PSP)
        self.bases[row][:5] = [2, 3, 5, 7, 11]
        self._verdict = {}
        self._base2 = {}

    def verdicts(self, rows, cols):
        out = []
        for r in range(rows):
            for c in range(cols):
                if (r, c) not in self._verdict:
                    self._verdict[r, c] = int(round_passes(self.cands[r], self.bases[r][c]))
                out.append(self._verdict[r, c])
        return out

    def base2(self, rows):
        for r in range(rows):
            if r not in self._base2:
                # the kernel's walk where Python walks it in a millisecond; wider, the round to the base 2 through pow —
                # tests/test_primes_host.py holds the two equal
                n = self.cands[r]
                self._base2[r] = int(mm.base2(n, self.bits) if self.bits <= 512 else round_passes(n, 2))
        return [self._base2[r] for r in range(rows)]


_CASES = {}


def case(bits):
    if bits not in _CASES:
        _CASES[bits] = Case(bits)
    return _CASES[bits]


def test_directed_rounds_are_what_they_claim():
    c = case(67)
    assert {"liar", "witness", "fermat", "minus", "last", "one"} <= c.kinds
    r = c.cands.index(561)
    assert c.verdicts(r + 1, 3)[-3:] == [0, c.verdicts(r + 1, 3)[-2], 1]
    r = c.cands.index(PSP)
    assert c.verdicts(r + 1, 5)[-5:] == [1, 1, 1, 1, 0]
    assert c.verdicts(c.cands.index(2047) + 1, 1)[-1] == 1


# ------------------------------------------------------------------ mr_split_t
def test_split_across_limb_and_word_boundaries(eng):
    rng = random.Random(7)
    mixed = []
    for bits in (96, 128, 512, 1024, 2048):
        from protocols.distributed_keygen_amd import limbs

        cands = []
        for s in (*[v for v in mm.S_VALUES if v < bits - 1], bits - 1):
            for _ in range(2):
                width = bits - s
                k = rng.getrandbits(width) | (1 << (width - 1)) | 1
                cands.append((k << s) + 1)
        cands += [3, 5, (1 << bits) - 1, (1 << (bits - 1)) + 1][: ROWS - len(cands)]
        mixed += cands[::3]
        d_t, s_t = eng.mr_split_t(rows_of(eng, cands, limbs.limbs_for_bits(bits)))
        want = [mm.split(n) for n in cands]
        assert ints_of(eng, d_t) == [d for d, _ in want]
        assert flags_of(s_t) == [s for _, s in want]
        d_t, s_t = eng.mr_split_t(rows_of(eng, cands, limbs.limbs_for_bits(bits)), bits)
        assert ints_of(eng, d_t) == [d for d, _ in want] and flags_of(s_t) == [s for _, s in want]
    mixed = mixed[:ROWS]                                   # rows of every width in one launch
    d_t, s_t = eng.mr_split_t(rows_of(eng, mixed, 64))
    assert ints_of(eng, d_t) == [mm.split(n)[0] for n in mixed] and flags_of(s_t) == [mm.split(n)[1] for n in mixed]


def test_argument_checks_launch_nothing(eng):
    from protocols.distributed_keygen_amd import DeviceRng

    rng = DeviceRng(bytes(32))
    good = rows_of(eng, [2**61 - 1, 2**64 - 59], 3)
    for bad in ([2**61 - 1, 2**64], [1, 5], [2**61 - 1, 0]):
        rows_t = rows_of(eng, bad, 3)
        for call in (lambda: eng.mr_split_t(rows_t), lambda: eng.miller_rabin_base2_t(rows_t, 96),
                     lambda: eng.miller_rabin_t(rows_t, good, 1), lambda: eng.probable_prime_t(rows_t, 96, 4, rng)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        eng.miller_rabin_base2_t(good, 61)                 # wider than the launch is sized for
    with pytest.raises(ValueError):
        eng.miller_rabin_t(good, good, 2)                  # rows of another shape
    with pytest.raises(ValueError):
        eng.miller_rabin_t(good, good, 0)
    with pytest.raises(ValueError):
        eng.probable_prime_t(good, 96, 0, rng)
    with pytest.raises(ValueError):
        eng.probable_prime_t(rows_of(eng, [8191, 2**61 - 1], 3), 96, 4, rng)      # below the sieve bound
    with pytest.raises(ValueError):
        eng.prime_search_t(1, 8, rng)
    with pytest.raises(ValueError):
        eng.prime_search_t(1, 128, rng, rounds=0)
    assert rng.next_call == 0
    assert eng.prime_search_t(0, 128, rng).shape == (0, 4)


# ------------------------------------------------------------------ miller_rabin_t / miller_rabin_base2_t
@pytest.mark.parametrize("bits", WIDTHS)
def test_rounds_against_the_model(eng, bits):
    c = case(bits)
    for g in (1, 3, 64):
        # the reference is one Python modexp per (row, column): all 151 x 64 of them where they are cheap, fewer rows
        # under many columns where a modexp takes milliseconds
        batches = BATCHES if bits < 512 or g == 1 else (1, 2) if g == 64 else BATCHES[:5] if bits > 512 else BATCHES
        for rows in batches:
            cands_t = rows_of(eng, c.cands[:rows], c.limbs)
            bases_t = rows_of(eng, [b for r in range(rows) for b in c.bases[r][:g]], c.limbs)
            got = flags_of(eng.miller_rabin_t(cands_t, bases_t, g, bits=bits))
            assert got == c.verdicts(rows, g), (bits, g, rows)
    cands_t = rows_of(eng, c.cands[:65], c.limbs)          # the launch sized by the rows' width alone
    bases_t = rows_of(eng, [b for r in range(65) for b in c.bases[r][:3]], c.limbs)
    assert flags_of(eng.miller_rabin_t(cands_t, bases_t, 3)) == c.verdicts(65, 3)


@pytest.mark.parametrize("bits", WIDTHS)
def test_base2_against_the_model_and_the_general_route(eng, bits):
    c = case(bits)
    for rows in BATCHES:
        cands_t = rows_of(eng, c.cands[:rows], c.limbs)
        got = flags_of(eng.miller_rabin_base2_t(cands_t, bits))
        assert got == c.base2(rows), (bits, rows)
        twos_t = rows_of(eng, [2] * rows, c.limbs)
        assert flags_of(eng.miller_rabin_t(cands_t, twos_t, 1, bits=bits)) == got
    wide = min(32 * c.limbs, bits + 29)                    # a launch sized for wider candidates than it holds
    assert flags_of(eng.miller_rabin_base2_t(rows_of(eng, c.cands[:65], c.limbs), wide)) == c.base2(65)


# ------------------------------------------------------------------ probable_prime_t / prime_search_t
# (bits, batch, rounds, key whose first batch holds COUNT primes, key whose first batch does not): found by
# find_search_keys() below, asserted again by the model in the test
COUNT = 2
SEARCHES = [(128, 128, 5, 1, 0), (512, 384, 5, 0, 3)]


def search_key(seed):
    return bytes([seed]) * 32


def find_search_keys(bits, batch, rounds):      # pragma: no cover - how SEARCHES was made
    enough = short = None
    for seed in range(256):
        _, verdicts = mm.prime_search(COUNT, bits, mm.chacha_draws(search_key(seed)), rounds, batch)
        if len(verdicts) == 1 and enough is None:
            enough = seed
        if len(verdicts) == 2 and short is None:
            short = seed
        if enough is not None and short is not None:
            return enough, short


@pytest.mark.parametrize("bits,batch,rounds,enough,short", SEARCHES)
def test_search_against_the_model(eng, bits, batch, rounds, enough, short):
    from protocols.distributed_keygen_amd import DeviceRng

    for seed, batches in ((enough, 1), (short, 2)):
        key = search_key(seed)
        want, verdicts = mm.prime_search(COUNT, bits, mm.chacha_draws(key), rounds, batch)
        assert len(verdicts) == batches                    # the second key takes the redraw path, once
        # the whole first batch, verdict by verdict: no prime missed, no composite kept
        draw = mm.chacha_draws(key)
        cands = [mm.force_bits(r, bits) for r in draw(batch, bits, 0)]
        rng = DeviceRng(key, first_call=1)
        got = flags_of(eng.probable_prime_t(rows_of(eng, cands, (bits + 31) // 32), bits, rounds, rng))
        assert got == [int(v) for v in verdicts[0]]
        assert got == [int(v) for v in mm.probable_prime(cands, bits, rounds, draw)]
        # the search itself: the first COUNT primes in draw order, top two bits and bit 0 set
        rng = DeviceRng(key)
        found = ints_of(eng, eng.prime_search_t(COUNT, bits, rng, rounds=rounds, batch=batch))
        assert found == want and len(found) == COUNT
        assert all(p >> (bits - 2) == 3 and p & 1 for p in found)
        assert rng.next_call == sum(1 + int(any(v)) for v in verdicts)


# ------------------------------------------------------------------ keys
def test_generated_keys_work(eng):
    from protocols.distributed_keygen_amd import PaillierPrivateKey, synthetic

    keys = [PaillierPrivateKey.generate(1024, engine=eng)] + PaillierPrivateKey.generate_batch(3, 256, engine=eng)
    assert [k.n.bit_length() for k in keys] == [1024, 256, 256, 256]
    assert len({x for k in keys for x in (k.p, k.q)}) == 8
    rng = random.Random(3)
    for k in keys:
        assert k.p.bit_length() == k.q.bit_length() == k.n.bit_length() // 2
        assert synthetic.is_probable_prime(k.p, rng) and synthetic.is_probable_prime(k.q, rng)
        msgs = [0, 1, k.n - 1, rng.randrange(k.n)]
        assert k.decrypt_batch(k.encrypt_batch(msgs)) == msgs


def test_check_primes_on_the_golden_keys(eng):
    from protocols.distributed_keygen_amd import PaillierPrivateKey, primes

    gold = json.loads((ROOT / "tests" / "golden" / "private_key_primes.json").read_text())["keys"]
    p, q = (int(gold["2048"][x], 16) for x in "pq")
    assert PaillierPrivateKey(p, q, engine=eng).check_primes() is True
    fake = int(gold["1024"]["p"], 16) * int(gold["1024"]["q"], 16)      # 1024 bits, two 512-bit prime factors
    assert PaillierPrivateKey(p, fake, engine=eng).check_primes() is False
    assert PaillierPrivateKey(fake, q, engine=eng).check_primes(rounds=2) is False
    vals = [p, fake, q, 2, 561, 2**61 - 1, -5, PSP, PSP * (2**31 - 1)]
    assert primes.is_probable_prime_batch(vals, rounds=8, engine=eng) == [True, False, True, True, False, True, False, False, False]
