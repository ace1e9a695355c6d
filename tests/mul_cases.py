"""Keys, statements and the directed rows of the response modulo M the multiplication-proof tests share
(test_multiplication_host.py, test_gpu_multiplication.py): the golden safe-prime keys as N and the model
(tools/mul_model.py) as the oracle."""

from __future__ import annotations

import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "tools"))
sys.path.insert(0, str(HERE))

import mul_model as mulm  # noqa: E402
from range_cases import KEY, modulus, primes  # noqa: E402,F401

LABEL = b"party 2 / product 2026-10-21"
E_MAX = (1 << 128) - 1
DIRECTED_K = (1, 0xFFFFFFFF, 1 << 32, 1 << 64, E_MAX)


def decrypt(key_length, c):
    """The plaintext of c under the golden key, by the textbook formula."""
    p, q = primes(key_length)
    n = p * q
    lam = (p - 1) * (q - 1)
    return (pow(c, lam, n * n) - 1) // n * pow(lam, -1, n) % n


def statements(n, count, seed=5):
    """(a, r_a, gamma, b, c_a, c_b): a = 0, N - 1, 1 first, then random; b random, N - 1, 0, 1 first."""
    rnd = random.Random(seed)
    a = ([0, n - 1, 1] + [rnd.randrange(n) for _ in range(max(0, count - 3))])[:count]
    b = ([rnd.randrange(n), n - 1, 0, 1] + [rnd.randrange(n) for _ in range(max(0, count - 4))])[:count]
    ra, gamma, rb = ([rnd.randrange(1, n) for _ in a] for _ in range(3))
    return a, ra, gamma, b, [mulm.encrypt(n, m, r) for m, r in zip(a, ra)], [mulm.encrypt(n, m, r) for m, r in zip(b, rb)]


def model_proofs(n, label, a, ra, gamma, ca, cb, call):
    """(d, (A, B, w, z, y) as five columns): the model's for the draws of DeviceRng(KEY, first_call=call)."""
    xs, us, vs = mulm.device_draws(KEY, call, len(a), n)
    rows = [mulm.prove(n, label, ca[r], cb[r], a[r], ra[r], gamma[r], xs[r], us[r], vs[r]) for r in range(len(a))]
    return [mulm.product(n, cb[r], a[r], gamma[r]) for r in range(len(a))], tuple([row[j] for row in rows] for j in range(5))


# ---- the rows of Engine.response_mod_rows_t ------------------------------------------------------------------------------
def moduli(wn, seed=3):
    """(name, M of exactly wn words): top word 1, top word all ones, 2^(32 (wn - 1)) + 1, all words all ones, an even
    one, and a random odd one."""
    rnd = random.Random(seed * 1000 + wn)
    low = 32 * (wn - 1)
    return [
        ("top word 1", (1 << low) | rnd.getrandbits(low) | 1),
        ("top word all ones", (0xFFFFFFFF << low) | rnd.getrandbits(low) | 1),
        ("2^(32 (wn - 1)) + 1", (1 << low) + 1),
        ("all words all ones", (1 << (32 * wn)) - 1),
        ("even", ((rnd.getrandbits(31) | (1 << 30)) << low | rnd.getrandbits(low)) & ~1),
        ("random odd", (rnd.getrandbits(32) | (1 << 17)) << low | rnd.getrandbits(low) | 1),
    ]


def directed_rows(mod, wn, ew=4):
    """(rho, e, x) rows with rho, x below M that put s = rho + e x on and beside multiples of M: s = 0; s = k M - 1, k M,
    k M + 1 for k in {1, 2^32 - 1, 2^32, 2^64, 2^128 - 1} — e and x chosen, rho = (-e x) mod M or that value -+ 1 when it
    stays in [0, M) —; and the largest row rho = x = M - 1, e = 2^(32 ew) - 1."""
    e_max = (1 << (32 * ew)) - 1
    rows = [(0, 0, 0), (0, e_max, 0), (0, 0, mod - 1), (mod - 1, e_max, mod - 1)]
    for k in DIRECTED_K:
        # e x in (k M - x, k M], so that rho = (-e x) mod M makes s = k M exactly; a k no row below M reaches is left out
        for x in (mod - 1, mod // 2 + 1, (mod >> 31) | 1):
            e = k * mod // x
            if not 1 <= e <= e_max or not 0 < x < mod:
                continue
            base = (-e * x) % mod
            assert base + e * x == k * mod
            for delta in (-1, 0, 1):
                rho = base + delta
                if 0 <= rho < mod:
                    rows.append((rho, e, x))
    return rows


def response_rows(mod, wn, count, ew=4, seed=9):
    """`count` rows (rho, e, x): the directed ones, then random ones below M; the LAST FOUR have rho or x at or above M
    where the row's width leaves room (their status may rise; w must be the residue all the same)."""
    rnd = random.Random(seed * 100 + wn)
    rows = directed_rows(mod, wn, ew)[:count]
    while len(rows) < count:
        rows.append((rnd.randrange(mod), rnd.getrandbits(32 * ew), rnd.randrange(mod)))
    full = (1 << (32 * wn)) - 1
    if count >= 8 and mod < full:
        e_max = (1 << (32 * ew)) - 1
        rows[-4:] = [(full, e_max, full), (mod, 0, 0), (mod - 1, e_max, full), (full, rnd.getrandbits(32 * ew), rnd.randrange(mod))]
    return rows


def expected(rows, mod, ew=4):
    """(w, t, status) columns of Python divmod."""
    out = [divmod(rho + e * x, mod) for rho, e, x in rows]
    return [r for _, r in out], [q & ((1 << (32 * ew)) - 1) for q, _ in out], [int(q >> (32 * ew) != 0) for q, _ in out]
