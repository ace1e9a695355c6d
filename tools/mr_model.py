#!/usr/bin/env python3
"""Python-int model of the strong-pseudoprime test of csrc/mx_mr.hpp and of the prime search around it
(``Engine.mr_split_t`` / ``miller_rabin_t`` / ``miller_rabin_base2_t`` / ``probable_prime_t`` / ``prime_search_t``) —
developer tool and the ORACLE of the tests: the GPU tests compare the kernels and the shipped compositions with it, and
so do the host tests, whose doubles (tests/mr_engine.py, tests/safe_engine.py) take only the primitives from here
(split, round_passes, base2) and run the shipped pipeline of key_flows.PrivateKeyFlows over them.

    split(n)              (d, s) with n - 1 = 2^s d, d odd
    tail(n, x0, b, s)     the verdict of one round from x0 = b^d mod n: b = 0 modulo n (vacuous), x0 = 1, x0 = n - 1, or
                          x0^(2^i) = n - 1 for an i in [1, s)
    round_passes(n, b)    split, pow, tail
    base2(n, bits)        the round to the base 2 the way mr_base2_kernel walks it: left to right over `bits` bit positions
                          of n - 1, one squaring per bit and a doubling where the bit is set; the comparisons of the last
                          s steps are the witness loop

The pipeline takes its random rows from a ``draw(count, bits, row_words)`` callable that returns ints — with
``chacha_draws(key, first_call)`` the rows of ``DeviceRng(key, first_call)``, call by call, so a seeded search is
reproducible on the CPU:

    probable_prime(cands, bits, rounds, draw)      sieve, base 2 on the survivors, `rounds` random bases on what is left
    prime_search(count, bits, draw, rounds, batch) draw, force the two top bits and bit 0, test, keep, draw again

Safe primes p = 2h + 1 (csrc/mx_sieve.hpp, csrc/mx_safe.hpp; ``Engine.safe_sieve_t`` / ``safe_prime_t`` / ``safe_prime_search_t``), `bits`
the width of p, the candidates the halves h of bits - 1 bits:

    safe_sieve_hit(h)                              some sieve prime divides h or 2h + 1, as one gcd with the primes' product
    safe_prime_stages(halves, bits, rounds, draw)  the survivors after the joint sieve, the base 2 on h, the base 2 on p
                                                   (Pocklington: with h prime that proves p) and `rounds` random bases on h
    safe_prime(halves, bits, rounds, draw)         the verdict per half
    safe_prime_search(count, bits, draw, rounds, batch)  draw halves, force bits bits - 2, bits - 3 and 0, test, keep p
"""
from __future__ import annotations

from typing import Callable, List, Sequence, Tuple

Draw = Callable[[int, int, int], List[int]]

SIEVE_BOUND = 1 << 14          # protocols/distributed_keygen_amd/primes.py: SIEVE_BOUND


def odd_primes_below(bound: int) -> List[int]:
    flags = bytearray([1]) * bound
    flags[0:2] = b"\0\0"
    for i in range(2, int(bound ** 0.5) + 1):
        if flags[i]:
            flags[i * i :: i] = bytearray(len(range(i * i, bound, i)))
    return [i for i in range(3, bound) if flags[i]]


def split(n: int) -> Tuple[int, int]:
    if n < 3 or n % 2 == 0:
        raise ValueError("an odd candidate >= 3 expected")
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    return d, s


def tail(n: int, x0: int, b: int, s: int) -> bool:
    if b % n == 0 or x0 == 1 or x0 == n - 1:
        return True
    x = x0
    for _ in range(1, s):
        x = x * x % n
        if x == n - 1:
            return True
    return False


def round_passes(n: int, b: int) -> bool:
    d, s = split(n)
    return tail(n, pow(b, d, n), b, s)


def base2(n: int, bits: int = 0) -> bool:
    """The kernel's walk: x starts as 1, steps i = bits - 1 .. 1 square it and double it where bit i of n - 1 is set; after
    step i it is 2^((n - 1) >> i).  Step s is compared with 1 and n - 1, the steps below it with n - 1."""
    _, s = split(n)
    bits = bits or n.bit_length()
    if n.bit_length() > bits:
        raise ValueError("candidate wider than the launch")
    x, verdict = 1, False
    for i in range(bits - 1, 0, -1):
        x = x * x % n
        if ((n - 1) >> i) & 1:
            x = 2 * x % n
        if i <= s and (x == n - 1 or (i == s and x == 1)):
            verdict = True
    return verdict


def chacha_draws(key: bytes, first_call: int = 0) -> Draw:
    """draw(count, bits, row_words) of ``DeviceRng(key, first_call)``: every call takes the next call number."""
    import chacha_model

    state = {"call": first_call}

    def draw(count: int, bits: int, row_words: int = 0) -> List[int]:
        call = state["call"]
        state["call"] = call + 1
        return chacha_model.row_ints(key, call, count, bits, row_words)

    return draw


_SIEVE: List[int] = []


def sieve_hit(n: int) -> bool:
    """What Engine.sieve_t reports for the odd primes below SIEVE_BOUND: some prime divides n (a small prime itself too)."""
    if not _SIEVE:
        _SIEVE.extend(odd_primes_below(SIEVE_BOUND))
    return any(n % p == 0 for p in _SIEVE)


def probable_prime(cands: Sequence[int], bits: int, rounds: int, draw: Draw) -> List[bool]:
    """Engine.probable_prime_t: the verdict per candidate.  One draw of survivors * rounds rows of bits + 64 bits — row
    c * rounds + k reduced modulo survivor c is the base of its round k — if anything survives the base 2."""
    out = [False] * len(cands)
    left = [i for i, n in enumerate(cands) if not sieve_hit(n)]
    left = [i for i in left if base2(cands[i], bits)]
    if left:
        draws = draw(len(left) * rounds, bits + 64, (bits + 64 + 31) // 32)
        for j, i in enumerate(left):
            out[i] = all(round_passes(cands[i], draws[j * rounds + k] % cands[i]) for k in range(rounds))
    return out


def force_bits(row: int, bits: int) -> int:
    return row | (3 << (bits - 2)) | 1


def prime_search(count: int, bits: int, draw: Draw, rounds: int, batch: int) -> Tuple[List[int], List[List[bool]]]:
    """Engine.prime_search_t: (the first `count` primes in draw order, the verdict vector of every batch drawn)."""
    found: List[int] = []
    verdicts: List[List[bool]] = []
    while len(found) < count:
        cands = [force_bits(r, bits) for r in draw(batch, bits, (bits + 31) // 32)]
        verdict = probable_prime(cands, bits, rounds, draw)
        verdicts.append(verdict)
        found.extend(n for n, ok in zip(cands, verdict) if ok)
    return found[:count], verdicts


_SIEVE_PRODUCTS: List[int] = []


def safe_sieve_hit(h: int) -> bool:
    """What Engine.safe_sieve_t reports for the odd primes below SIEVE_BOUND: some prime l has h = 0 or h = (l - 1) / 2
    modulo l, that is, divides h (2h + 1) — exact, as gcds with the product of the primes below 2^8 (which settles 97 % of
    random candidates) and with the product of the rest."""
    import math

    if not _SIEVE_PRODUCTS:
        odd = odd_primes_below(SIEVE_BOUND)
        _SIEVE_PRODUCTS.extend([math.prod(l for l in odd if l < 256), math.prod(l for l in odd if l >= 256)])
    v = h * (2 * h + 1)
    return math.gcd(v, _SIEVE_PRODUCTS[0]) != 1 or math.gcd(v, _SIEVE_PRODUCTS[1]) != 1


def safe_prime_stages(halves: Sequence[int], bits: int, rounds: int, draw: Draw) -> List[List[int]]:
    """Engine.safe_prime_t stage by stage: the indices left by the joint sieve, by the base 2 on h (bits - 1 bits), by the
    base 2 on p = 2h + 1 (`bits` bits) and by `rounds` random bases on h — ONE draw of survivors * rounds rows of bits - 1
    + 64 bits, row c * rounds + k reduced modulo survivor c, if anything is left for it."""
    sieved = [i for i, h in enumerate(halves) if not safe_sieve_hit(h)]
    half2 = [i for i in sieved if base2(halves[i], bits - 1)]
    full2 = [i for i in half2 if base2(2 * halves[i] + 1, bits)]
    final: List[int] = []
    if full2:
        draws = draw(len(full2) * rounds, bits - 1 + 64, (bits - 1 + 64 + 31) // 32)
        final = [i for j, i in enumerate(full2)
                 if all(round_passes(halves[i], draws[j * rounds + k] % halves[i]) for k in range(rounds))]
    return [sieved, half2, full2, final]


def safe_prime(halves: Sequence[int], bits: int, rounds: int, draw: Draw) -> List[bool]:
    final = set(safe_prime_stages(halves, bits, rounds, draw)[-1])
    return [i in final for i in range(len(halves))]


def force_half_bits(row: int, bits: int) -> int:
    """The half of a p of exactly `bits` bits with its two top bits set and p = 3 mod 4."""
    return row | (3 << (bits - 3)) | 1


def safe_prime_search(count: int, bits: int, draw: Draw, rounds: int, batch: int) -> Tuple[List[int], List[List[bool]]]:
    """Engine.safe_prime_search_t: (the first `count` safe primes p in draw order, the verdict vector of every batch)."""
    found: List[int] = []
    verdicts: List[List[bool]] = []
    while len(found) < count:
        halves = [force_half_bits(r, bits) for r in draw(batch, bits - 1, (bits + 31) // 32)]
        verdict = safe_prime(halves, bits, rounds, draw)
        verdicts.append(verdict)
        found.extend(2 * h + 1 for h, ok in zip(halves, verdict) if ok)
    return found[:count], verdicts


_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
SAFE_KINDS = ("safe", "half", "full", "neither")


def safe_cases(bits: int, seed: int = 1, per_kind: int = 2) -> dict:
    """{kind: [h, ...]} — `per_kind` halves h of exactly bits - 1 bits (bits bits - 2, bits - 3 and 0 set) that PASS the
    joint sieve, per kind: "safe" (h and p = 2h + 1 prime), "half" (h prime, p composite), "full" (p prime, h composite),
    "neither" (both composite).  From a generator seeded by (seed, bits); the candidates of the GPU tests."""
    import random

    rng = random.Random(seed * 100003 + bits)
    out: dict = {kind: [] for kind in SAFE_KINDS}
    while any(len(v) < per_kind for v in out.values()):
        h = force_half_bits(rng.getrandbits(bits - 1), bits)
        if safe_sieve_hit(h):
            continue
        half = all(round_passes(h, b) for b in _BASES)
        if not half and all(len(out[k]) >= per_kind for k in ("full", "neither")):
            continue                                  # only safe primes are still missing: skip the test of p
        full = all(round_passes(2 * h + 1, b) for b in _BASES)
        kind = SAFE_KINDS[(0 if half else 2) + (0 if full else 1)]
        if len(out[kind]) < per_kind:
            out[kind].append(h)
    return out


def pseudoprime_half(start: int = 1 << 15, tries: int = 1 << 20) -> int:
    """A composite h = f (3f - 2), both factors prime and above SIEVE_BOUND, that is a strong pseudoprime to the base 2 and
    passes the joint sieve together with 2h + 1: the base-2 stage on h keeps it, as it keeps a prime.  (f = 2 mod 3 makes
    h = 2 mod 3, so that 3 does not divide 2h + 1 — a Carmichael number (6k + 1)(12k + 1)(18k + 1) is 1 mod 3 and never
    passes; f - 1 divides 3f - 3, which is what makes liars frequent.)"""
    for f in range(start + (2 - start) % 3, start + tries, 3):
        h = f * (3 * f - 2)
        if f % 2 and not safe_sieve_hit(h) and all(round_passes(x, b) for x in (f, 3 * f - 2) for b in _BASES[:6]) and base2(h):
            return h
    raise ValueError("no such pseudoprime in the range")


S_VALUES = (1, 2, 28, 29, 30, 31, 32, 33, 57, 58, 59, 64, 65)      # shifts across the 29-bit limb and the 32-bit word


def proth_pair(bits: int, s: int, seed: int = 1, tries: int = 20000) -> Tuple[int, int]:
    """(a prime, a composite) of exactly `bits` bits of the form k 2^s + 1 with k odd, from a generator seeded by (seed,
    bits, s); 0 in place of the prime where none turns up (s = bits - 1 leaves k = 1 only)."""
    import random

    rng = random.Random((seed * 100003 + bits) * 100003 + s)
    width = bits - s
    if width < 1:
        raise ValueError("s must be below bits")
    prime = composite = 0
    for _ in range(min(tries, 8 << max(0, width - 2))):      # there are 2^(width - 2) such k
        k = rng.getrandbits(width) | (1 << (width - 1)) | 1
        n = (k << s) + 1
        if all(round_passes(n, b) for b in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)):
            prime = prime or n
        else:
            composite = composite or n
        if prime and composite:
            break
    return prime, composite


def proth_shifts(bits: int) -> List[int]:
    return [*[v for v in S_VALUES if v < bits - 1], bits - 1]


def proth_cases(bits: int, seed: int = 1) -> dict:
    """{s: (prime, composite)} for S_VALUES below bits and for s = bits - 1: the candidates of the GPU tests."""
    return {s: proth_pair(bits, s, seed) for s in proth_shifts(bits)}


if __name__ == "__main__":
    import json
    import sys

    if len(sys.argv) > 2 and sys.argv[1] == "safe":      # mr_model.py safe 512 1024 > tests/golden/safe_prime_cases.json: a minute
        print(json.dumps({"form": "halves h of bits - 1 bits past the joint sieve, hex, by kind: safe = h and 2h + 1 prime, "
                                  "half = h prime only, full = 2h + 1 prime only, neither",
                          "bits": {b: {k: [hex(h) for h in v] for k, v in safe_cases(int(b)).items()} for b in sys.argv[2:]}}, indent=1))
    elif len(sys.argv) > 1:      # mr_model.py 512 1024 2048 > tests/golden/mr_proth.json: the wide cases take a minute to find
        from multiprocessing import Pool

        jobs = [(int(b), s) for b in sys.argv[1:] for s in proth_shifts(int(b))]
        with Pool() as pool:
            pairs = pool.starmap(proth_pair, jobs)
        print(json.dumps({"form": "k * 2^s + 1, k odd; [prime, composite] per s, hex; 0 = none",
                          "bits": {b: {str(s): [hex(v) for v in pair] for (jb, s), pair in zip(jobs, pairs) if jb == int(b)}
                                   for b in sys.argv[1:]}}, indent=1))
    else:
        for n, b in ((561, 2), (2047, 2), (3215031751, 7), (3215031751, 11)):
            print(n, b, round_passes(n, b), base2(n) if b == 2 else "")
