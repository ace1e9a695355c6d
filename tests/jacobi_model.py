"""Host models of the Jacobi kernels (csrc/mx_jacobi.hpp) and the operands of their directed tests.

posdivsteps_jacobi_model   the algorithm alone (batched all-positive divsteps), as validated against sympy
divstep_wave_model         jacobi_kernel<NL> for one wavefront: the lanes in lock-step with the kernel's g == 1 exit, the
                           launcher's max_batches and the `live` / JC / JREFRESH bookkeeping that the lanes share
fallback_model             jacobi_fallback_kernel<NL>'s pass loop for one symbol
launch_model               a whole mx_jacobi_dev launch: symbols packed 64 to a wavefront across the groups, the last one padded
                           with its last row, unfinished symbols handed to the fallback from their original operands

The models are CASE SELECTORS: they say which paths operands reach.  What is right is decided by oracle.jacobi_symbol.
"""

from __future__ import annotations

import random

JC, JREFRESH, JSTEPS = 8, 4, 30
INSTANCES = (3, 5, 9, 17, 33, 65, 129, 257)
M64 = (1 << 64) - 1
WORD = 0xFFFFFFFF

DIVSTEP_EVENTS = (
    "finish_f_one",            # f == 1 after a batch
    "finish_g_one",            # g == 1 after a batch (the kernel's second exit)
    "finish_f_eq_g",           # f == g > 1: common factor, symbol 0
    "batch_is_one_shift",      # the low 30 bits of g are zero: the whole batch is one shift
    "mask_capped_by_i",        # eta + 1 >= i: the steps left in the batch cap the bits cancelled at once
    "top_carry_nonzero",       # a non-zero final carry goes into the top limb of the last live chunk
    "live_chunk_crossed",      # the operands' top limb drops below a JC chunk boundary between two refreshes (NL > JC)
    "unfinished_at_max_batches",
)
FALLBACK_EVENTS = (
    "word_shift",              # a[0] == 0: a whole word of trailing zeros
    "swap_sign_flip",          # a < n and both = 3 (mod 4)
    "swap_no_flip",
    "no_swap",
    "odd_z_n_3_mod_8",         # an odd number of trailing zeros removed with n = 3 (mod 8): sign flips
    "odd_z_n_5_mod_8",
)


def instance_for(limbs: int) -> int:
    return next(nl for nl in INSTANCES if limbs <= nl)


def max_batches_for(limbs: int, knob: int = 0) -> int:
    """mx_jacobi_dev_range: the batch bound of the divstep kernel; the developer knob v > 0 allows v - 1 batches"""
    return knob - 1 if knob > 0 else (32 * limbs * 9 // 2) // JSTEPS + 8


def _batch_matrix(f: int, g: int, eta: int, jac: int, steps: int, ev=None):
    """`steps` divsteps decided on the low 64 bits: (u, v, q, r, eta, jac)"""
    u, v, q, r = 1, 0, 0, 1
    fl, gl, i = f & M64, g & M64, steps
    first = True
    while True:
        t = (gl | (M64 << i)) & M64
        zeros = (t & -t).bit_length() - 1
        if ev is not None and first and zeros == steps:
            ev.add("batch_is_one_shift")
        first = False
        gl >>= zeros
        u <<= zeros
        v <<= zeros
        eta -= zeros
        i -= zeros
        jac ^= zeros & ((fl >> 1) ^ (fl >> 2)) & 1
        if i == 0:
            break
        if eta < 0:
            eta = -eta
            fl, gl, u, q, v, r = gl, fl, q, u, r, v
            jac ^= ((fl & gl) >> 1) & 1
            mask = (M64 >> (64 - min(eta + 1, i))) & 63
            w = (fl * gl * (fl * fl - 2)) & mask
        else:
            mask = (M64 >> (64 - min(eta + 1, i))) & 15
            w = (-(fl + (((fl + 1) & 4) << 1)) * gl) & mask
        if ev is not None and eta + 1 >= i:
            ev.add("mask_capped_by_i")
        gl = (gl + fl * w) & M64
        q += u * w
        r += v * w
    assert max(u, v, q, r) <= 1 << steps
    return u, v, q, r, eta, jac


def posdivsteps_jacobi_model(x: int, n: int, steps: int = 30) -> int:
    """Python model of csrc/mx_jacobi.hpp: batches of `steps` all-positive divsteps decided from the
    low 64 bits, a 2x2 matrix per batch applied to the full operands, sign tracked on the low bits."""
    if n == 1:
        return 1
    if x == 0 or n % 2 == 0:
        return 0
    f, g, eta, jac = n, x, -1, 0
    for _ in range((n.bit_length() + 31) // 32 * 32 * 4 // steps + 8):
        u, v, q, r, eta, jac = _batch_matrix(f, g, eta, jac, steps)
        f, g = (u * f + v * g) >> steps, (q * f + r * g) >> steps
        assert f <= n and g <= n
        if f == 1:
            return 1 - 2 * (jac & 1)
        if f == g:
            return 0
    raise AssertionError("no convergence")


def _limbs_of(x: int) -> int:
    return (x.bit_length() + 31) // 32


def divstep_wave_model(pairs, nl: int, max_batches: int):
    """jacobi_kernel<NL> on one wavefront.  pairs: up to 64 (value, modulus).  Returns ([symbol, or None where the kernel
    writes JACOBI_UNFINISHED], batches run, events)."""
    assert 0 < len(pairs) <= 64
    nch = (nl + JC - 1) // JC
    ev: set = set()
    lanes = []
    for x, n in pairs:
        f_is_one = n == 1
        done = f_is_one or x == 0 or not n & 1
        lanes.append({"f": n, "g": x, "eta": -1, "jac": 0, "done": done, "result": 1 if f_is_one else 0})
    live, batch = nch, 0
    for batch in range(max_batches):
        if all(s["done"] for s in lanes):
            break
        top = max((0 if s["done"] else _limbs_of(s["f"] | s["g"])) for s in lanes)
        if batch % JREFRESH == 0:
            live = (top + JC - 1) // JC
        elif (top + JC - 1) // JC < live:
            ev.add("live_chunk_crossed")
        room = 32 * min(live * JC, nl)                   # the limbs the kernel reads and writes this batch
        for s in lanes:
            if s["done"]:
                continue
            u, v, q, r, s["eta"], s["jac"] = _batch_matrix(s["f"], s["g"], s["eta"], s["jac"], JSTEPS, ev)
            f, g = s["f"], s["g"]
            assert f >> room == 0 and g >> room == 0     # (`live` covers every lane: what lies above is zero)
            sf, sg = u * f + v * g, q * f + r * g
            if sf >> room or sg >> room:
                ev.add("top_carry_nonzero")
            # the top limb of the last live chunk takes 32 bits of (carry, low word) >> 30: what does not fit is lost
            s["f"], s["g"] = (sf >> JSTEPS) & ((1 << room) - 1), (sg >> JSTEPS) & ((1 << room) - 1)
            if s["f"] == 1 or s["g"] == 1:
                ev.add("finish_f_one" if s["f"] == 1 else "finish_g_one")
                s["done"], s["result"] = True, 1 - 2 * (s["jac"] & 1)
            elif s["f"] == s["g"]:
                ev.add("finish_f_eq_g")
                s["done"], s["result"] = True, 0
    else:
        batch = max_batches
    if not all(s["done"] for s in lanes):
        ev.add("unfinished_at_max_batches")
    return [s["result"] if s["done"] else None for s in lanes], batch, ev


def fallback_model(x: int, n: int, nl: int):
    """jacobi_fallback_kernel<NL>'s pass loop from the original operands: (symbol, passes, events)"""
    ev: set = set()
    a, t, passes = x, 1, 0
    for passes in range(64 * nl + 2):
        if a == 0:
            break
        while a & WORD == 0:
            ev.add("word_shift")
            a >>= 32
        low = a & WORD
        z = (low & -low).bit_length() - 1
        if z:
            a >>= z
            if z & 1 and n & 7 in (3, 5):
                ev.add("odd_z_n_3_mod_8" if n & 7 == 3 else "odd_z_n_5_mod_8")
                t = -t
        if a < n:
            if a & 3 == 3 and n & 3 == 3:
                ev.add("swap_sign_flip")
                t = -t
            else:
                ev.add("swap_no_flip")
            a, n = n - a, a
        else:
            ev.add("no_swap")
            a -= n
    return (t if a == 0 and n == 1 else 0), passes, ev


def launch_model(rows, mods, knob: int = 0):
    """Engine.jacobi_batch(rows, mods) as the device computes it (equal-sized groups): ([[symbol]], divstep events,
    fallback events, most batches of a wavefront)"""
    gsize = len(rows[0])
    assert all(len(r) == gsize for r in rows)
    limbs = max(1, max(_limbs_of(m) for m in mods))
    nl = instance_for(limbs)
    flat = [(x, m) for r, m in zip(rows, mods) for x in r]
    out, dev, fev, most = [], set(), set(), 0
    for w in range(0, len(flat), 64):
        pairs = flat[w : w + 64]
        lanes = pairs + [pairs[-1]] * (64 - len(pairs))              # invalid lanes compute the launch's last row again
        res, batches, ev = divstep_wave_model(lanes, nl, max_batches_for(limbs, knob))
        dev |= ev
        most = max(most, batches)
        for (x, n), s in zip(pairs, res):
            if s is None:
                s, _, ev = fallback_model(x, n, nl)
                fev |= ev
            out.append(s)
    return [out[g * gsize : (g + 1) * gsize] for g in range(len(mods))], dev, fev, most


# ---------------------------------------------------------------------------------------------- operands of the directed tests
GROUP = 32          # symbols per modulus: two groups to a wavefront, so that moduli of one width share their `live`


def directed_moduli(nl: int):
    """moduli of instance NL, in pairs of one width (a pair fills a wavefront): two pairs that exactly fill the NL limbs, and
    pairs one bit over a chunk boundary (8 c limbs + 1 bit: the top chunk holds a single bit, which the first batches remove
    between two refreshes of `live`).  The 257-word instance gets one pair of each kind."""
    rng = random.Random(nl)
    full = 32 * nl
    mods = [(1 << full) - 1, (1 << full) - 3]
    if nl < 257:
        mods += [rng.getrandbits(full) | (1 << (full - 1)) | 1, (1 << full) - (1 << (full // 2)) - 1]
    chunks = sorted({c for c in (1, (nl - 1) // JC // 2, (nl - 1) // JC) if c >= 1 and JC * c + 1 <= nl and (nl < 257 or c == 32)})
    for c in chunks:
        bits = 32 * JC * c + 1
        mods += [(1 << (bits - 1)) + 1 + 2 * (rng.getrandbits(bits - 2)), (1 << (bits - 1)) + 3]
    return mods


def directed_values(n: int, count: int = GROUP):
    """`count` numerators below n: multiples of 2^32 and 2^64 (whole-word shifts), tiny ones, n - 2^k, halves, common factors"""
    k = n.bit_length()
    rng = random.Random(n & WORD)
    cand = [0, 1, 2, 3, 5, 7, 1 << 32, 1 << 64, 3 << 32, 7 << 64, 1 << 30, 1 << 60, 1 << 62, n - 1, n - 2, n - 4, n - (1 << 32),
            n - (1 << 64), n - (1 << (k // 2)), n - (1 << (k - 2)), (n + 1) // 2, n >> 1, n // 3, 3 * (n // 3) % n,
            (1 << (k - 1)) - 1, 1 << (k - 2), (1 << (k // 2)) - 1, ((n >> 96) << 96) + (3 << 64), rng.getrandbits(20) | 1,
            rng.getrandbits(k // 3) << 32, 15 * rng.getrandbits(40)]
    out = []
    for v in cand:
        v %= n
        if v not in out:
            out.append(v)
    while len(out) < count:
        out.append(rng.randrange(n))
    return out[:count]


def directed_groups(nl: int):
    """(rows, moduli) of the directed test of instance NL"""
    mods = directed_moduli(nl)
    return [directed_values(m, GROUP if nl < 257 else GROUP // 2) for m in mods], mods


# ---------------------------------------------------------------------------------------------- how many batches operands need
def batches_needed(x: int, n: int) -> int:
    """divstep batches until (x / n) is decided, with no bound"""
    res, batch, _ = divstep_wave_model([(x, n)], instance_for(max(1, _limbs_of(n))), 1 << 30)
    assert res[0] is not None
    return batch


def worst_batches(bits: int):
    """(batches, modulus name, value name) of the operand pair of the structured families that needs the most batches"""
    rng = random.Random(bits)
    k, h = bits, bits // 2
    mods = {"2^k-1": (1 << k) - 1, "2^k-3": (1 << k) - 3, "2^(k-1)+1": (1 << (k - 1)) + 1, "2^(k-1)+3": (1 << (k - 1)) + 3,
            "2^k-2^(k/2)-1": (1 << k) - (1 << h) - 1, "2^(k-1)+2^(k/2)+1": (1 << (k - 1)) + (1 << h) + 1,
            "random": rng.getrandbits(k) | (1 << (k - 1)) | 1}
    worst = (0, "", "")
    for mname, n in mods.items():
        vals = {"1": 1, "2": 2, "3": 3, "5": 5, "7": 7, "n-1": n - 1, "n-2": n - 2, "n-3": n - 3, "n-4": n - 4, "(n+1)/2": (n + 1) // 2,
                "n>>1": n >> 1, "n//3": n // 3, "2^32": 1 << 32, "2^64": 1 << 64, "n-2^32": n - (1 << 32), "2^(k/2)": 1 << h,
                "2^(k/2)-1": (1 << h) - 1, "2^(k/2)+1": (1 << h) + 1, "n-2^(k/2)": n - (1 << h), "2^(k-2)": 1 << (k - 2),
                "2^(k-2)-1": (1 << (k - 2)) - 1, "2^(k-2)+1": (1 << (k - 2)) + 1, "3*2^(k-3)": 3 << (k - 3), "random": rng.randrange(n)}
        for vname, v in vals.items():
            if 0 < v < n:
                worst = max(worst, (batches_needed(v, n), mname, vname))
    return worst


if __name__ == "__main__":
    for bits in (96, 160, 1028, 2053, 4100, 8197):
        b, mname, vname = worst_batches(bits)
        bound = max_batches_for((bits + 31) // 32)
        print(f"{bits} bits: {b} batches ({b / bits:.3f} per bit) for ({vname} / {mname}); the launcher's bound is {bound}", flush=True)
