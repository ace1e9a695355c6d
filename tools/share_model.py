#!/usr/bin/env python3
"""Model of the candidate and sharing kernels (csrc/mx_share.hpp) and of the layers above them — developer tool and
test vehicle.  Pure Python: random rows come from tools/chacha_model.py, reductions are ``%`` and polynomials are
evaluated by Horner's rule on Python ints.

The definitions (what the kernels, ``Engine.prime_candidates_t`` / ``shamir_share_t`` and ``shamir.generate_pq_*`` must
reproduce bit for bit):

    candidate(r, L, first)      2^(L-1) + (r << 2) + (3 if first else 0)        r: L - 3 random bits   (DK:874-875)
    coefficient k of element e  a_k[e] = D[k][e] mod P                           D: bits(P) + 64 random bits
    share of element e at x     s[e] + sum_{k=1..degree} a_k[e] * x^k  mod P     canonical residue

    rows of a device draw       ``rng.rows_t(engine, degree * batch, bits(P) + 64, cw)``, cw = ceil((bits(P) + 64) / 32):
                                row (k - 1) * batch + e is D[k][e]

    generate_pq, first call c   c: p candidates, c + 1: q candidates, c + 2: p coefficients (degree t),
                                c + 3: q coefficients (degree t), c + 4: zero coefficients (degree 2t)
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import chacha_model


def coefficient_bits(prime: int) -> int:
    return prime.bit_length() + 64


def coefficient_words(prime: int) -> int:
    return -(-coefficient_bits(prime) // 32)


def row_int(words: Sequence[int]) -> int:
    return sum(int(v) << (32 * j) for j, v in enumerate(words))


def int_row(value: int, words: int) -> List[int]:
    if value < 0 or value >> (32 * words):
        raise ValueError("the value does not fit the row")
    return [(value >> (32 * j)) & 0xFFFFFFFF for j in range(words)]


def candidate(r: int, prime_length: int, first_party: bool) -> int:
    if prime_length < 8:
        raise ValueError("prime_length must be at least 8")
    if not 0 <= r < 1 << (prime_length - 3):
        raise ValueError("r must have at most prime_length - 3 bits")
    return (1 << (prime_length - 1)) + (r << 2) + (3 if first_party else 0)


def candidates(random_rows: Sequence[Sequence[int]], prime_length: int, first_party: bool) -> List[int]:
    """The candidates of rows of L - 3 random bits (little-endian 32-bit words)."""
    return [candidate(row_int(row), prime_length, first_party) for row in random_rows]


def share(secret: int, draws: Sequence[int], prime: int, points: Sequence[int]) -> List[int]:
    """The shares of one secret at `points`; draws[k - 1] is the draw of coefficient k."""
    coeffs = [d % prime for d in draws]
    out = []
    for x in points:
        acc = 0
        for a in reversed(coeffs):
            acc = (acc + a) * x % prime
        out.append((acc + secret) % prime)
    return out


def shamir_share(secrets: Optional[Sequence[int]], draws: Sequence[Sequence[int]], prime: int, points: Sequence[int]) -> List[List[int]]:
    """out[j][e] for draws[k - 1][e] = D[k][e]; ``secrets=None`` shares zero."""
    degree = len(draws)
    batch = len(draws[0])
    if secrets is None:
        secrets = [0] * batch
    per_elem = [share(secrets[e], [draws[k][e] for k in range(degree)], prime, points) for e in range(batch)]
    return [[per_elem[e][j] for e in range(batch)] for j in range(len(points))]


def device_draws(key: bytes, call: int, degree: int, batch: int, prime: int) -> List[List[int]]:
    """draws[k - 1][e] of the one rows call a device-drawn sharing makes (call number `call` of `key`)."""
    rows = chacha_model.row_ints(key, call, degree * batch, coefficient_bits(prime), coefficient_words(prime)) if degree * batch else []
    return [rows[k * batch : (k + 1) * batch] for k in range(degree)]


def device_candidates(key: bytes, call: int, count: int, prime_length: int, first_party: bool) -> List[int]:
    rows = chacha_model.rows(key, call, count, prime_length - 3) if count else []
    return candidates(rows, prime_length, first_party)


def generate_pq(key: bytes, first_call: int, index: int, prime_length: int, prime: int, n_parties: int, t: int,
                batch: int) -> Tuple[List[int], List[int], Dict[str, Dict[int, List[int]]]]:
    """``shamir.generate_pq_batch`` for ``DeviceRng(key, first_call)``: (p_additive, q_additive, shares)."""
    points = list(range(1, n_parties + 1))
    p = device_candidates(key, first_call, batch, prime_length, index == 1)
    q = device_candidates(key, first_call + 1, batch, prime_length, index == 1)
    cols = {
        "p": shamir_share(p, device_draws(key, first_call + 2, t, batch, prime), prime, points),
        "q": shamir_share(q, device_draws(key, first_call + 3, t, batch, prime), prime, points),
        "zero": shamir_share(None, device_draws(key, first_call + 4, 2 * t, batch, prime), prime, points),
    }
    return p, q, {name: {x: col[j] for j, x in enumerate(points)} for name, col in cols.items()}


if __name__ == "__main__":
    P = (1 << 127) - 1
    print(generate_pq(bytes(range(32)), 0, 1, 32, P, 3, 1, 2))
