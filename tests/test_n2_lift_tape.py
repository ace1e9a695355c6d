"""The lifted tape of the N^2 modexp (include/mxpaillier.h: mx_nsquare_plan), checked without a GPU.

For a = b (mod N), a^N = b^N (mod N^2); with e = e1 N + e0 the planner therefore computes c^e1 with first-digit
operations only — modulo N — and raises that to N, times c^e0, with pair operations.  The tapes come from the host-only
export mx_nsquare_tape and run here in an interpreter over plain integers, on the residues the pairs represent:

  * a pair operation acts modulo N^2;
  * a first-digit operation computes its product modulo N and then ADDS A RANDOM MULTIPLE OF N: the kernel leaves the
    second digit stale there, so nothing downstream may depend on it;
  * N2_CLR1 reduces modulo N.

Slots as the kernel's prologue fills them, in represented values (rho = R^-1 mod N^2): K1 = R, K2 = 2^k R, E = rho,
ONE = 1, x_lo and x_hi times rho; the epilogue reads the accumulator's plain N-adic value, acc * R."""

from __future__ import annotations

import ctypes
import random

import numpy as np
import pytest

SQR, MUL, ADD, LOAD, STORE, MULC, SQR0, MUL0, CLR1 = range(9)
SLOT_K1, SLOT_K2, SLOT_E, SLOT_ONE, SLOT_LO, SLOT_HI, SLOT_TMP, SLOT_SQ, SLOT_TABLE = range(9)
FIXED_WINDOW = 1
MAX_WORDS = 16384

# two known primes per composite modulus (Mersenne and other well-known primes keep the file free of big literals)
P25, Q25 = 33554393, 33554383                        # the two largest primes below 2^25
P521, Q508 = (1 << 521) - 1, (1 << 508) - 0x1BD      # 2^521 - 1 is prime; the second factor only has to be odd


def _modulus(bits: int, rng: random.Random):
    """(N, a known factor or None): 50 and 1029 bits as products, 131 and 2051 bits random odd numbers of that length."""
    if bits == 50:
        n = P25 * Q25
        assert n.bit_length() == 50
        return n, P25
    if bits == 1029:
        n = P521 * Q508
        assert n.bit_length() == 1029, n.bit_length()
        return n, P521
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1, None


def _tape(n: int, e: int, flags: int, lifted: int):
    from protocols.distributed_keygen_amd import _lib, limbs as Lm

    lib = _lib.lib()
    limbs_n, elimbs = Lm.limbs_for(n), Lm.limbs_for(e)
    h_n, h_e = Lm.pack_one(n, limbs_n), Lm.pack_one(e, elimbs)
    words = np.zeros(MAX_WORDS, dtype=np.uint32)
    plan = _lib.NsquarePlan()
    got = lib.mx_nsquare_tape(h_n.ctypes.data, h_e.ctypes.data, limbs_n, elimbs, flags, lifted, words.ctypes.data, MAX_WORDS,
                              ctypes.byref(plan))
    assert got >= 0, got
    return [(int(w) >> 28, int(w) & 0x0FFFFFFF) for w in words[:got]], plan


def _run(tape, n: int, bases, rng: random.Random):
    """The tape over the residues the pairs represent, every base at once; the results as the epilogue would emit them."""
    n2 = n * n
    k = n.bit_length() - 1
    r = 1 << (n.bit_length() + 4)
    rho = pow(r, -1, n2)
    out = []
    for x in bases:
        slots = {SLOT_K1: r % n2, SLOT_K2: (r << k) % n2, SLOT_E: rho, SLOT_ONE: 1,
                 SLOT_LO: rho * (x & ((1 << k) - 1)) % n2, SLOT_HI: rho * (x >> k) % n2}
        acc = 0
        noise = lambda: rng.randrange(n) * n                      # what a stale second digit amounts to
        for op, arg in tape:
            if op == SQR:
                for _ in range(arg):
                    acc = acc * acc % n2
            elif op == SQR0:
                for _ in range(arg):
                    acc = (acc * acc % n + noise()) % n2
            elif op in (MUL, MULC):
                acc = acc * slots[arg] % n2
            elif op == MUL0:
                acc = (acc * (slots[arg] % n) % n + noise()) % n2   # the slot's second digit is never read
            elif op == ADD:
                acc = (acc + slots[arg]) % n2
            elif op == LOAD:
                acc = slots[arg]
            elif op == STORE:
                slots[arg] = acc
            elif op == CLR1:
                acc %= n
            else:
                raise AssertionError(f"unknown tape operation {op}")
        out.append(acc * r % n2)
    return out


def _counts(tape):
    c = {"sqr": 0, "mul": 0, "sqr0": 0, "mul0": 0, "top": SLOT_TABLE}
    for op, arg in tape:
        if op == SQR:
            c["sqr"] += arg
        elif op == SQR0:
            c["sqr0"] += arg
        elif op in (MUL, MULC):
            c["mul"] += 1
        elif op == MUL0:
            c["mul0"] += 1
        if op not in (SQR, SQR0, CLR1):
            c["top"] = max(c["top"], arg)
    return c


def _exponents(n: int, bits: int, rng: random.Random):
    es = {
        "0": 0, "1": 1, "N-1": n - 1, "N": n, "N+1": n + 1, "2N": 2 * n,
        "kN": rng.getrandbits(bits) * n,                                            # e0 = 0
        "N+2^j": n + (1 << (bits // 3)),
        "short e0": (rng.getrandbits(bits + 40) | (1 << (bits + 39))) * n + rng.getrandbits(bits - 41),      # e0 with 40 leading zero bits
        "2.05x": rng.getrandbits(int(2.05 * bits)) | (1 << (int(2.05 * bits) - 1)),
    }
    if bits == 2051:
        es["headline"] = rng.getrandbits(4197) | (1 << 4196)
    return es


@pytest.mark.parametrize("bits", [50, 131, 1029, 2051])
def test_tapes_compute_the_power_and_counts_match(bits):
    rng = random.Random(bits)
    n, factor = _modulus(bits, rng)
    n2 = n * n
    bases = [0, 1, n, n + 1, n2 - 1, (factor or 3) * rng.randrange(1, n) % n2, rng.randrange(n2)]
    lifted_seen = preferred_seen = 0
    for name, e in _exponents(n, bits, rng).items():
        want = [pow(b, e, n2) for b in bases]
        classic, plan = _tape(n, e, 0, 0)
        assert _run(classic, n, bases, rng) == want, (bits, name, "classic")
        cc = _counts(classic)
        assert (cc["sqr0"], cc["mul0"]) == (0, 0)
        assert plan.ntape == len(classic)
        lifted, plan_l = _tape(n, e, 0, 1)
        assert bytes(plan) == bytes(plan_l)                                          # one descriptor whichever tape is fetched
        assert plan.ntape_lift == len(lifted) and bool(plan.lift & 1) == bool(lifted)
        top = cc["top"]
        if lifted:
            lifted_seen += 1
            assert e > n, name                                                       # e <= N: nothing to lift
            assert _run(lifted, n, bases, rng) == want, (bits, name, "lifted")
            lc = _counts(lifted)
            assert (lc["sqr0"] > 0 or e < 2 * n) and lc["sqr"] + lc["sqr0"] == plan.lift_positions      # e1 = 1: a load, no squaring
            assert 0 < plan.lift_pos1 < plan.lift_positions and 0 < plan.lift_share1 < 65536
            assert (plan.n_sqr_classic, plan.n_mul_classic) == (cc["sqr"], cc["mul"])
            top = max(top, lc["top"])
        else:
            assert plan.lift == 0 and e <= n, name
        # the counts of the descriptor are those of the tape a one-wavefront launch runs by default
        d = _counts(lifted) if plan.lift & 2 else cc
        preferred_seen += 1 if plan.lift & 2 else 0
        assert (plan.n_sqr, plan.n_mul, plan.n_sqr_first, plan.n_mul_first) == (d["sqr"], d["mul"], d["sqr0"], d["mul0"]), name
        assert SLOT_TABLE + plan.table_rows > top, name                              # the table region covers every slot touched
        if e <= n:
            assert not (plan.lift & 2) and plan.n_sqr_first == 0 and plan.n_mul_first == 0, name
        # fixed-window plans stay classic
        fixed, plan_f = _tape(n, e, FIXED_WINDOW, 0)
        fc = _counts(fixed)
        assert (fc["sqr0"], fc["mul0"]) == (0, 0) and plan_f.lift == 0 and plan_f.ntape_lift == 0 and plan_f.n_sqr_first == 0, name
        assert _tape(n, e, FIXED_WINDOW, 1)[0] == []
        if name in ("1", "2.05x"):
            assert _run(fixed, n, bases[3:], rng) == want[3:], (bits, name, "fixed")
    assert lifted_seen >= 6
    assert preferred_seen >= 1                                                       # 2.05 x bits(N) pays at every size


def test_headline_plan_prefers_the_lifted_tape_and_saves_what_the_model_says():
    """key_length 2048, a 4197-bit exponent: ~2145 first-digit and ~2050 pair squarings, two tables within the region a
    fixed-window plan has today, and ~0.81 of the classic tape's cost in the planner's units."""
    rng = random.Random(4197)
    n = rng.getrandbits(2051) | (1 << 2050) | 1
    e = rng.getrandbits(4197) | (1 << 4196)
    lifted, plan = _tape(n, e, 0, 1)
    assert plan.lift == 3
    assert 2040 <= plan.n_sqr <= 2060 and 2135 <= plan.n_sqr_first <= 2155
    assert 4188 <= plan.n_sqr_classic <= 4197 and plan.table_rows <= 128      # (the first window is loaded, not squared up to)
    cost = lambda sq, mu, sq0, mu0: 5718 * sq + 7746 * mu + 2615 * sq0 + 3367 * mu0          # csrc/mx_host.hpp: N2_COST_*
    ratio = cost(plan.n_sqr, plan.n_mul, plan.n_sqr_first, plan.n_mul_first) / cost(plan.n_sqr_classic, plan.n_mul_classic, 0, 0)
    assert 0.78 < ratio < 0.84, ratio
    # cost-based segment cuts: phase 1 holds about half of the positions but well under half of the cost
    assert plan.lift_pos1 / plan.lift_positions > 0.5 and plan.lift_share1 / 65536 < 0.4


def test_export_refuses_what_prepare_refuses():
    from protocols.distributed_keygen_amd import _lib, limbs as Lm

    lib = _lib.lib()
    h_n, h_e = Lm.pack_one(15, 1), Lm.pack_one(77, 1)
    words = np.zeros(64, dtype=np.uint32)
    plan = _lib.NsquarePlan()
    call = lambda hn, fl, lf, mx: lib.mx_nsquare_tape(hn.ctypes.data, h_e.ctypes.data, 1, 1, fl, lf, words.ctypes.data, mx, ctypes.byref(plan))
    assert call(h_n, 0, 0, 64) > 0
    assert call(h_n, 0, 0, 2) == -4 and call(h_n, 2, 0, 64) == -1 and call(h_n, 0, 2, 64) == -1
    assert call(Lm.pack_one(14, 1), 0, 0, 64) == -3 and call(Lm.pack_one(1, 1), 0, 0, 64) == -3
