"""The cases the sparse-matrix-product tests share (tests/test_spmm_host.py, tests/test_gpu_spmm.py): the parity matrix
of 9 rows over 40 inputs, its inputs for a modulus, and the expected values by CPython's ``pow``."""

from __future__ import annotations

import math
import random

N_IN, N_ROWS = 40, 9
TOP = (1 << 63) - 1


def expected(cts, crow, col, val, n, bias=None):
    """[(1 + (bias_r % n) * n) * prod(pow(x, v, n * n)) % (n * n)]; pow with a negative v gives the inverse."""
    n2 = n * n
    out = []
    for r in range(len(crow) - 1):
        acc = 1 if bias is None else (1 + (bias[r] % n) * n) % n2
        for t in range(crow[r], crow[r + 1]):
            acc = acc * pow(cts[col[t]], val[t], n2) % n2
        out.append(acc)
    return out


def unit(rng, n):
    """A residue modulo n^2 with an inverse."""
    while True:
        x = rng.randrange(2, n * n)
        if math.gcd(x, n) == 1:
            return x


def parity_inputs(n, seed=1):
    """40 inputs with inverses: 1, N^2 - 1, a value >= N^2 (reduced on upload) and duplicates among them."""
    rng = random.Random(seed)
    cts = [unit(rng, n) for _ in range(N_IN)]
    cts[0] = 1
    cts[1] = n * n - 1
    cts[2] = n * n + unit(rng, n)
    cts[5] = cts[4]
    cts[17] = cts[3]
    return cts


def parity_matrix(seed=2):
    """(crow, col, val, bias) as lists: an empty row, a single weight 1, a single weight -1, a row over all 40 columns
    with signed weights, a row with a duplicate (row, column), a row with a stored 0, a row with 2^63 - 1 and
    -(2^63 - 1), two random rows with signed 16-bit weights.  The bias has a negative value and one above any N used
    here."""
    rng = random.Random(seed)
    rows = [
        [],
        [(7, 1)],
        [(3, -1)],
        [(c, rng.choice((-1, 1)) * rng.randrange(1, 1 << 12)) for c in range(N_IN)],
        [(4, 5), (9, -3), (4, 11), (9, -2), (12, 1)],
        [(6, 0), (8, 9), (30, -4), (31, 0)],
        [(10, TOP), (11, -TOP), (0, 2), (1, 3)],
        [(c, rng.randrange(-(1 << 15), 1 << 15)) for c in sorted(rng.sample(range(N_IN), 12))],
        [(c, rng.randrange(-(1 << 15), 1 << 15)) for c in rng.sample(range(N_IN), 17)],
    ]
    assert len(rows) == N_ROWS
    crow, col, val = [0], [], []
    for row in rows:
        col += [c for c, _ in row]
        val += [v for _, v in row]
        crow.append(len(col))
    bias = [3, -5, 0, (1 << 4100) + 12345, 7, -1, 1, 2, 99]
    return crow, col, val, bias


def dict_rows(crow, col, val):
    """The rows as ``{column: weight}`` for linear_map: duplicate entries added up (x^a x^b = x^(a + b))."""
    rows = []
    for r in range(len(crow) - 1):
        row = {}
        for t in range(crow[r], crow[r + 1]):
            row[col[t]] = row.get(col[t], 0) + val[t]
        rows.append(row)
    return rows
