"""Inputs of the share-recombination tests (tests/test_combine_constants.py), built with CPython integers only.

A case is a synthetic key (``synthetic.make_key``), a number of partials np and BATCH plaintexts.  A threshold
decryption of m multiplies partial decryptions whose product is x = 1 + (m theta) N modulo N^2; here np - 1 of them are
``pow(g, e, N^2)`` for random residues g and random 32-bit exponents e, and the last one is x times the inverse of their
product (``pow(product, -1, N^2)``), so that the rows have the product of a real decryption for any np, without the
key-sized exponentiations of one.

The bad rows are fixed rows of the same shape whose product is NOT 1 modulo N, or is 0: what the kernel writes for them
(zeros and status 1) is recorded from the library as it was before the recombination took its constants from the
host, tests/golden/combine_bad_rows.json.
"""

from __future__ import annotations

import functools
import random
from typing import Dict, List, Tuple

BATCH = 64
KEY_LENGTHS = (512, 2048)
NPS = (2, 3, 5)
NP_GENERAL = 9           # more partials than the plan holds a constant for (MX_COMBINE_NP_MAX = 8): the general route


@functools.lru_cache(maxsize=None)
def make_key(key_length: int):
    from protocols.distributed_keygen_amd import synthetic

    return synthetic.make_key(key_length, 3, 1)


@functools.lru_cache(maxsize=None)
def messages(key_length: int) -> List[int]:
    key = make_key(key_length)
    rng = random.Random(key_length * 17 + 5)
    return [0, 1, key.n - 1] + [rng.randrange(key.n) for _ in range(BATCH - 3)]


@functools.lru_cache(maxsize=None)
def good_case(key_length: int, np_: int) -> Tuple[List[List[int]], List[int]]:
    """(partials[e][i], expected plaintexts) of the BATCH plaintexts of the key for np_ partials."""
    key, msgs = make_key(key_length), messages(key_length)
    n, n2 = key.n, key.n_square
    rng = random.Random(key_length * 131 + np_)
    rows, want = [], []
    for m in msgs:
        row, prod = [], 1
        for _ in range(np_ - 1):
            row.append(pow(rng.randrange(2, n2), rng.getrandbits(32) | 1, n2))
            prod = prod * row[-1] % n2
        row.append((1 + m * key.theta % n * n) * pow(prod, -1, n2) % n2)
        x = 1
        for p in row:
            x = x * p % n2
        assert (x - 1) % n == 0
        rows.append(row)
        want.append((x - 1) // n * key.theta_inv % n)
    assert want == msgs
    return rows, want


def bad_rows(key_length: int, np_: int) -> List[List[int]]:
    """Rows that the recombination must refuse: the good rows 0 .. 3 with one partial changed so that the product is no
    longer 1 modulo N (+1, doubled, replaced by N^2 - 1, replaced by N), then rows whose product is 0 modulo N^2: a
    partial that is 0, and the pair N * N."""
    key = make_key(key_length)
    n, n2 = key.n, key.n_square
    rows = [list(r) for r in good_case(key_length, np_)[0][:6]]
    rows[0][0] = (rows[0][0] + 1) % n2
    rows[1][-1] = rows[1][-1] * 2 % n2
    rows[2][np_ // 2] = n2 - 1
    rows[3][0] = n
    rows[4][np_ - 1] = 0
    rows[5][0], rows[5][1] = n, n
    for r in rows[:4]:
        x = 1
        for p in r:
            x = x * p % n2
        assert (x - 1) % n != 0
    return rows


def golden_name(key_length: int, np_: int) -> str:
    return f"k{key_length}_np{np_}"


def bad_cases() -> Dict[str, Tuple[int, int]]:
    return {golden_name(kl, np_): (kl, np_) for kl in KEY_LENGTHS for np_ in NPS + (NP_GENERAL,)}
