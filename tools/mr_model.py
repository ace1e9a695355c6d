#!/usr/bin/env python3
"""Python-int model of the strong-pseudoprime test of csrc/mx_mr.hpp and of the prime search around it
(``Engine.mr_split_t`` / ``miller_rabin_t`` / ``miller_rabin_base2_t`` / ``probable_prime_t`` / ``prime_search_t``) —
developer tool and test vehicle.

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

    if len(sys.argv) > 1:      # mr_model.py 512 1024 2048 > tests/golden/mr_proth.json: the wide cases take a minute to find
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
