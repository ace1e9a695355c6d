"""Probable primes on the GPU: a batched Miller-Rabin test and the search for random primes around it — what makes or
vets the primes of an ordinary private key (``private_key.PaillierPrivateKey.generate`` / ``check_primes``).

The test of a batch runs in three stages, each on what the one before left (``Engine.probable_prime_t``): trial division
by the odd primes below ``SIEVE_BOUND`` (``Engine.sieve_t``), the strong-pseudoprime test to the base 2
(``Engine.miller_rabin_base2_t``), and ``rounds`` rounds to random bases (``Engine.miller_rabin_t``: the generic modexp
b^d mod n, then the witness loop).  A composite passes a round to a random base with probability at most 1/4, so
``rounds = 64`` bounds the error for ANY input — a number chosen by somebody else to fool the test included — by 4^-64,
without leaning on the average-case tables that hold only for random candidates.  The random rounds run only on the few
candidates that survive the base 2, so the bound is cheap; a caller who tests candidates it drew itself at random may
lower ``rounds`` (for random 1024-bit candidates a handful of rounds already gives 2^-80, Damgard-Landrock-Pomerance
1993).

Side channels.  The base-2 stage (csrc/mx_mr.hpp: mr_base2_kernel) works from the candidate alone, without a window table
or a tape: one squaring and one selected doubling per bit, a sequence of operations that depends on the bit length of
the widest candidate of the launch only (the comparisons at its end run for as many steps as the largest number of
trailing zero bits of n - 1 in a wavefront).  A candidate that becomes p or q leaks neither through a schedule nor
through table addresses there.  The random-base rounds go through ``Engine.powmod_multi_t``, the generic kernel's
fixed-window ladder: its sequence of operations depends on the bit lengths only, the table rows it reads are chosen by the
digits of d = (n - 1) / 2^s — the class private_key.py documents for the key's own modexps.  The sieve and the
compaction between the stages show which candidates were dropped where; those are not the key.

Safe primes, p = 2h + 1 with h prime as well (``random_safe_primes`` / ``is_safe_prime_batch``;
``Engine.safe_prime_t``).  The candidates are the halves h.  One joint sieve (``Engine.safe_sieve_t``, csrc/mx_sieve.hpp)
drops every h with h = 0 or h = (l - 1) / 2 modulo a prime l below ``SIEVE_BOUND`` — l divides h or 2h + 1 — from one
pass over limbs and tables; then the base 2 on h, the base 2 on p, and the `rounds` random bases on h ONLY.  Pocklington:
with h an odd prime, p = 2h + 1, 3 not dividing p (the sieve saw to it) and 2^(p-1) = 1 mod p, p is prime — the proven
factor F = h of p - 1 exceeds sqrt(p), and gcd(2^((p-1)/h) - 1, p) = gcd(3, p) = 1.  The round to the base 2 on p has
s = 1 and d = h and checks 2^h = 1 or -1, which is that condition.  The error bound for ANY input stays 4^-rounds: a
composite h passes the rounds with at most that probability, and a prime h makes the verdict on p exact.

Side channels of the safe-prime search.  All modexps are those above, on h and on p = 2h + 1: the base 2 from the
candidate alone, the random rounds on h through the fixed-window ladder, table rows chosen by the digits of
(h - 1) / 2^s.  The joint sieve and the compaction between the four stages show which candidates fell where and how
many batches a search drew; those are not the key.
"""

from __future__ import annotations

import math
from typing import Any, List, Optional, Sequence

SIEVE_BOUND = 1 << 14          # the sieve divides by the 1899 odd primes below it; about 12 % of odd candidates survive

_ODD_PRIMES: List[int] = []


def sieve_primes() -> List[int]:
    """The odd primes below SIEVE_BOUND."""
    if not _ODD_PRIMES:
        flags = bytearray([1]) * SIEVE_BOUND
        for i in range(3, math.isqrt(SIEVE_BOUND) + 1, 2):
            if flags[i]:
                flags[i * i :: 2 * i] = bytearray(len(range(i * i, SIEVE_BOUND, 2 * i)))
        _ODD_PRIMES.extend(i for i in range(3, SIEVE_BOUND, 2) if flags[i])
    return _ODD_PRIMES


def prime_density(bits: int) -> float:
    """A lower bound of the share of primes among the odd numbers of `bits` bits: 2 / (bits ln 2)."""
    return 2.0 / (bits * math.log(2.0))


def poisson_shortfall(count: int, mean: float) -> float:
    """P[X < count] for X Poisson with the given mean."""
    term = total = math.exp(-mean)
    for k in range(1, count):
        term *= mean / k
        total += term
    return total if count > 0 else 0.0


SHORTFALL = 0.02


def default_batch(count: int, bits: int) -> int:
    """The rows ``Engine.prime_search_t`` draws per batch when the caller names none: the smallest multiple of 64 whose
    expected number of primes, batch * 2 / (bits ln 2), leaves a Poisson probability of at most 2 % that the batch
    holds fewer than `count` — one batch is nearly always enough, and a second one is drawn when it is not."""
    count, bits = int(count), int(bits)
    if count < 1 or bits < 2:
        raise ValueError("count >= 1 and bits >= 2 expected")
    mean = float(count)
    while poisson_shortfall(count, mean) > SHORTFALL:      # grows by at most a few standard deviations
        mean += max(1.0, 0.25 * math.sqrt(mean))
    return 64 * math.ceil(mean / prime_density(bits) / 64)


HARDY_LITTLEWOOD_C2 = 0.6601618158      # the twin-prime constant: prod over odd primes l of 1 - 1 / (l - 1)^2


def safe_prime_density(bits: int) -> float:
    """The share of the odd h of `bits` - 1 bits for which h and p = 2h + 1 are both prime (p a safe prime of `bits`
    bits), by the Hardy-Littlewood conjecture for Sophie Germain pairs: 4 C2 / ((bits - 1) ln 2)^2 — one in about
    190 000 at 1024 bits.  Counted against random draws at 64, 128 and 256 bits: 276, 142 and 24 found where the
    formula predicts 277, 136 and 25."""
    bits = int(bits)
    if bits < 3:
        raise ValueError("bits >= 3 expected")
    return 4.0 * HARDY_LITTLEWOOD_C2 / ((bits - 1) * math.log(2.0)) ** 2


# What ``default_safe_batch`` lets one draw of the safe-prime search hold at most, in bytes of candidate rows (4 bytes per
# word of a row of `bits` bits).  It bounds two things: the device memory of a draw — the rows, and the index and flag
# tensors of the stages, a few bytes per row more — and the work a search does past its last hit, which is at most one
# batch because the search stops at the first batch that completes `count`.  At 1024 bits it is 131 072 rows, about 0.7
# expected safe primes.
SAFE_BATCH_BYTES = 16 << 20


def default_safe_batch(count: int, bits: int) -> int:
    """The rows ``Engine.safe_prime_search_t`` draws per batch when the caller names none: ``default_batch``'s Poisson
    rule from ``safe_prime_density`` — the smallest multiple of 64 whose expected number of safe primes leaves at most
    2 % that it holds fewer than `count` — capped at ``SAFE_BATCH_BYTES`` of rows (a multiple of 64 again, at least
    64).  Where the cap binds, as it does from a few hundred bits on, a search takes several batches and stops at the
    first that completes `count`: sizing a batch to hold a rare hit with 98 % probability would be 3-7 times the
    expected work."""
    count, bits = int(count), int(bits)
    if count < 1 or bits < 3:
        raise ValueError("count >= 1 and bits >= 3 expected")
    mean = float(count)
    while poisson_shortfall(count, mean) > SHORTFALL:
        mean += max(1.0, 0.25 * math.sqrt(mean))
    cap = max(64, SAFE_BATCH_BYTES // (4 * ((bits + 31) // 32)) // 64 * 64)
    return min(cap, 64 * math.ceil(mean / safe_prime_density(bits) / 64))


def _trial_division(n: int) -> bool:
    """Exact for 2 <= n < SIEVE_BOUND^2."""
    if n % 2 == 0:
        return n == 2
    for p in sieve_primes():
        if p * p > n:
            break
        if n % p == 0:
            return False
    return True


def _engine(engine: Any) -> Any:
    if engine is not None:
        return engine
    from .engine import default_engine

    return default_engine()


def _rng(rng: Any) -> Any:
    if rng is not None:
        return rng
    from .device_rng import DeviceRng

    return DeviceRng()


def is_probable_prime_batch(values: Sequence[int], rounds: int = 64, rng: Any = None, engine: Any = None) -> List[bool]:
    """[is n a (probable) prime for n in values] as one GPU batch.  Negative numbers, 0, 1 and even numbers are decided on
    the host, and so is everything below SIEVE_BOUND^2, by exact trial division (the device sieve flags a small prime
    itself as divisible); the rest goes through ``Engine.probable_prime_t``: wrong with probability at most 4^-rounds
    for a composite, never for a prime.  ``rng``: a ``device_rng.DeviceRng`` for the random bases (default: a fresh
    one)."""
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError("rounds must be at least 1")
    vals = [int(v) for v in values]
    out = [False] * len(vals)
    device: List[int] = []
    for i, n in enumerate(vals):
        if n < 2 or (n % 2 == 0 and n != 2):
            continue
        if n < SIEVE_BOUND * SIEVE_BOUND:
            out[i] = _trial_division(n)
        else:
            device.append(i)
    if device:
        from . import limbs

        eng = _engine(engine)
        cands = [vals[i] for i in device]
        bits = limbs.max_bits(cands)
        rows_t = eng.to_device(limbs.pack(cands, limbs.limbs_for_bits(bits)))
        verdict = eng.probable_prime_t(rows_t, bits, rounds, _rng(rng))
        verdict = verdict.cpu().numpy() if hasattr(verdict, "cpu") else verdict
        for i, ok in zip(device, verdict):
            out[i] = bool(ok)
    return out


def random_primes(count: int, bits: int, rng: Any = None, rounds: int = 64, engine: Any = None, batch: Optional[int] = None) -> List[int]:
    """`count` random probable primes of exactly `bits` bits with the two top bits set (the product of two of them has
    exactly 2 * bits bits), drawn and tested on the device: ``Engine.prime_search_t`` fetched as ints.  ``rng``: a
    ``device_rng.DeviceRng`` (default: a fresh one, keyed from the operating system)."""
    count = int(count)
    if count < 0:
        raise ValueError("count must not be negative")
    if count == 0:
        return []
    from . import limbs

    eng = _engine(engine)
    return limbs.unpack(eng.to_host(eng.prime_search_t(count, int(bits), _rng(rng), rounds=rounds, batch=batch)))


def is_safe_prime_batch(values: Sequence[int], rounds: int = 64, rng: Any = None, engine: Any = None) -> List[bool]:
    """[is p a safe prime — p and (p - 1) / 2 both (probable) primes — for p in values] as one GPU batch.  Decided on the
    host: negative numbers, 0, 1 and even numbers (2 is no safe prime), every p below SIEVE_BOUND^2 (exact trial
    division of p and (p - 1) / 2; 5 and 7 are safe primes), and p = 1 mod 4, whose half is even.  The rest goes through
    ``Engine.safe_prime_t`` as the halves (p - 1) / 2: wrong with probability at most 4^-rounds for anything that is no
    safe prime, never for a safe prime (the module docstring has the argument)."""
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError("rounds must be at least 1")
    vals = [int(v) for v in values]
    out = [False] * len(vals)
    device: List[int] = []
    for i, p in enumerate(vals):
        if p < 5 or p % 2 == 0:
            continue
        if p < SIEVE_BOUND * SIEVE_BOUND:
            out[i] = _trial_division(p) and _trial_division((p - 1) // 2)
        elif p % 4 == 3:
            device.append(i)
    if device:
        from . import limbs

        eng = _engine(engine)
        halves = [(vals[i] - 1) // 2 for i in device]
        bits = limbs.max_bits([vals[i] for i in device])
        rows_t = eng.to_device(limbs.pack(halves, limbs.limbs_for_bits(bits)))
        verdict = eng.safe_prime_t(rows_t, bits, rounds, _rng(rng))
        verdict = verdict.cpu().numpy() if hasattr(verdict, "cpu") else verdict
        for i, ok in zip(device, verdict):
            out[i] = bool(ok)
    return out


def random_safe_primes(count: int, bits: int, rng: Any = None, rounds: int = 64, engine: Any = None, batch: Optional[int] = None) -> List[int]:
    """`count` random safe primes p = 2h + 1 of exactly `bits` bits with the two top bits set (the product of two of them
    has exactly 2 * bits bits; p = 3 mod 4), drawn and tested on the device: ``Engine.safe_prime_search_t`` fetched as
    ints.  ``rng``: a ``device_rng.DeviceRng`` (default: a fresh one, keyed from the operating system)."""
    count = int(count)
    if count < 0:
        raise ValueError("count must not be negative")
    if count == 0:
        return []
    from . import limbs

    eng = _engine(engine)
    return limbs.unpack(eng.to_host(eng.safe_prime_search_t(count, int(bits), _rng(rng), rounds=rounds, batch=batch)))
