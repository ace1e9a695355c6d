"""Operands for the directed tests of the wave-wide inverse (csrc/mx_modinv.hpp), chosen with tests/modinv_model.py.

Random operands of 2000 bits and more reach none of the kernel's carry-propagate, zero-word and in-lane ripple paths (each
has probability about 2^-32 per lane and step).  The structured families below reach them.  For every instance (LPL = 1, 2, 3,
5, 9) and two sizes — "large": the widest modulus the instance takes, "small": about three lanes — the candidates
moduli x values are run through the model and a small set that covers every reachable event is kept.

The families are enumerated here, deterministically; which candidates were kept is recorded in
tests/golden/modinv_directed_cases.json as indices into that enumeration, with the events each one reaches, because running the
model over every large candidate takes half an hour.  `python tests/modinv_cases.py` rewrites that file;
tests/test_modinv_model_host.py re-runs the model on the kept cases and fails if the record no longer matches.
"""

from __future__ import annotations

import json
import random
from pathlib import Path

import modinv_model as model

STORE = Path(__file__).resolve().parent / "golden" / "modinv_directed_cases.json"
MAX_CASES = 24                       # per (instance, size): also the most rows of one launch in the GPU tests
SIZES = ("large", "small")


def size_bits(lpl: int, size: str) -> int:
    """bit length of the moduli of (instance, size)"""
    if size == "large":
        # 64 * LPL words >= bits + 34 bits; the LPL = 9 instance stops earlier, at the library's widest modulus
        return min(2048 * lpl - 34, model.MAX_MOD_BITS)
    bits = 96 * lpl - 3                                  # three lanes ...
    while model.dispatch(bits, (bits + 31) // 32) != lpl:      # ... or the smallest size the dispatch gives to this instance
        bits += 1
    return bits


def _in_instance(m: int, lpl: int) -> bool:
    return m >= 3 and m & 1 == 1 and model.dispatch(m.bit_length(), (m.bit_length() + 31) // 32) == lpl


def moduli(lpl: int, size: str):
    """[(name, modulus)]: 2^k +- 1, 2^k - 3, 2^k +- 2^(k/2) +- 1 with k at and just under the size, word and lane multiples, a
    random modulus, moduli with all-ones words inside lanes, and multiples of 3 (so that non-invertible values exist)"""
    nb, B = size_bits(lpl, size), 32 * lpl
    ks = {nb, nb - 1, nb // 32 * 32, nb // 32 * 32 - 1, nb // B * B, nb // B * B - 1, nb // B * B + 1}
    out = []
    for k in sorted(ks, reverse=True):
        h = k // 2
        for name, m in ((f"2^{k}-1", (1 << k) - 1), (f"2^{k}+1", (1 << k) + 1), (f"2^{k}-3", (1 << k) - 3),
                        (f"2^{k}-2^{h}-1", (1 << k) - (1 << h) - 1), (f"2^{k}-2^{h}+1", (1 << k) - (1 << h) + 1),
                        (f"2^{k}+2^{h}+1", (1 << k) + (1 << h) + 1), (f"2^{k}+2^{h}-1", (1 << k) + (1 << h) - 1)):
            if _in_instance(m, lpl):
                out.append((name, m))
    rng = random.Random(1000 * lpl + len(size))
    out.append(("random", rng.getrandbits(nb) | (1 << (nb - 1)) | 1))
    # all-ones and all-zero words inside lanes: every third lane random, the others 0xFFFFFFFF / 0 word by word
    m = 0
    for l in range((nb + B - 1) // B):
        for j in range(lpl):
            word = rng.getrandbits(32) if l % 3 == 0 and j == 0 else (model.WORD if (l + j) % 2 == 0 else 0)
            m |= word << (B * l + 32 * j)
    m = (m & ((1 << nb) - 1)) | (1 << (nb - 1)) | 1
    out.append(("ones_words", m))
    out.append(("3*random", 3 * (rng.getrandbits(nb - 2) | (1 << (nb - 3)) | 1)))
    return [(name, m) for name, m in out if _in_instance(m, lpl) and m.bit_length() <= nb]


def values(lpl: int, m: int):
    """[(name, value)], 0 <= value < m"""
    B, k = 32 * lpl, m.bit_length()
    h = k // 2
    rng = random.Random(m & 0xFFFFFFFF)
    ones_lanes = sum((model.WORD if (l + j) % 3 else rng.getrandbits(32)) << (B * l + 32 * j) for l in range(64) for j in range(lpl))
    cand = [("0", 0), ("1", 1), ("2", 2), ("3", 3), ("m-1", m - 1), ("m-2", m - 2), ("m-3", m - 3), ("(m+1)/2", (m + 1) // 2),
            ("m>>1", m >> 1), ("2^h", 1 << h), ("2^h-1", (1 << h) - 1), ("2^h+1", (1 << h) + 1), ("2^32", 1 << 32), ("2^64", 1 << 64),
            ("2^64-1", (1 << 64) - 1), ("2^B", 1 << B), ("2^B-1", (1 << B) - 1), ("2^B+1", (1 << B) + 1), ("2^(2B)-1", (1 << 2 * B) - 1),
            ("2^(5B)+1", (1 << 5 * B) + 1), ("2^(7B)-1", (1 << 7 * B) - 1), ("2^(5B)", 1 << 5 * B), ("3*2^(2B)", 3 << 2 * B),
            ("m-2^64", m - (1 << 64)), ("m-2^B", m - (1 << B)), ("m-2^(3B)", m - (1 << 3 * B)), ("m-2^h", m - (1 << h)),
            ("m-2^(2B)+1", m - (1 << 2 * B) + 1), ("(m>>B)<<B", (m >> B) << B), ("m>>(k-2B)", m >> max(k - 2 * B, 1)),
            ("(2^(3B)-1)<<(2B)", ((1 << 3 * B) - 1) << 2 * B), ("2^(h+B)-2^h", (1 << (h + B)) - (1 << h)),
            ("m//3", m // 3), ("2(m//3)", 2 * (m // 3)), ("m//3+2^(2B)", m // 3 + (1 << 2 * B)), ("m-m//3-2^B", m - m // 3 - (1 << B)),
            ("ones_lanes", ones_lanes), ("random", rng.getrandbits(k)), ("random_h", rng.getrandbits(h)),
            ("random<<3B", rng.getrandbits(max(h - 3 * B, 8)) << 3 * B)]
    seen, out = set(), []
    for name, v in cand:
        v %= m
        if v not in seen and v >= 0:
            seen.add(v)
            out.append((name, v))
    return out


def candidates(lpl: int, size: str):
    """[(modulus index, value index, modulus name, value name, modulus, value)] of (instance, size), in a fixed order"""
    out = []
    for mi, (mname, m) in enumerate(moduli(lpl, size)):
        for vi, (vname, v) in enumerate(values(lpl, m)):
            out.append((mi, vi, mname, vname, m, v))
    return out


def select(lpl: int, size: str):
    """greedy cover, twice over: the candidate that reaches the most events which fewer than two kept cases reach so far,
    until none adds any or MAX_CASES are kept.  Among equals an invertible candidate goes first (a non-invertible one needs a
    launch of its own)."""
    scored = []
    for mi, vi, _, _, m, v in candidates(lpl, size):
        inv, _, ev = model.modinv(v, m)
        scored.append((mi, vi, inv is not None, frozenset(ev)))
    kept, times = [], dict.fromkeys(model.EVENTS, 0)
    while len(kept) < MAX_CASES:
        rest = [c for c in scored if c not in kept]
        best = max(rest, key=lambda c: (sum(times[e] == 0 for e in c[3]), sum(times[e] == 1 for e in c[3]), c[2]))
        if all(times[e] >= 2 for e in best[3]):
            break
        kept.append(best)
        for e in best[3]:
            times[e] += 1
    return [[mi, vi, sorted(ev)] for mi, vi, _, ev in kept]


def load():
    """{(lpl, size): [(modulus, value, recorded events)]} of the kept cases"""
    record = json.loads(STORE.read_text())
    out = {}
    for lpl in model.LPLS:
        for size in SIZES:
            mods = moduli(lpl, size)
            vals = {}
            cases = []
            for mi, vi, ev in record[f"{lpl}/{size}"]:
                m = mods[mi][1]
                if mi not in vals:
                    vals[mi] = values(lpl, m)
                cases.append((m, vals[mi][vi][1], frozenset(ev)))
            out[(lpl, size)] = cases
    return out


def dispatch_boundary_moduli():
    """[(need, limbs, modulus, instance or None)]: both sides of every boundary of the dispatch.  need = 64 ... 321 is set by the
    modulus' bits (the smallest and the largest bit length of that `need`); 576 and 577 by the row width, the modulus itself
    held at the library's widest (a longer one is refused before the dispatch)."""
    out = []
    for need in (64, 65, 128, 129, 192, 193, 320, 321):
        for bits in (32 * need - 65, 32 * need - 34):
            m = (1 << bits) - (1 << (bits // 2)) - 1                 # inter-lane borrows and zero words (the families above)
            limbs = (bits + 31) // 32
            assert max(limbs, (bits + 65) // 32) == need
            out.append((need, limbs, m, model.dispatch(bits, limbs)))
    m = (1 << model.MAX_MOD_BITS) - (1 << (model.MAX_MOD_BITS // 2)) - 1
    out.append((576, 576, m, model.dispatch(m.bit_length(), 576)))
    out.append((577, 577, m, model.dispatch(m.bit_length(), 577)))
    return out


if __name__ == "__main__":
    from multiprocessing import Pool

    keys = [(lpl, size) for lpl in reversed(model.LPLS) for size in SIZES]
    with Pool(len(keys)) as pool:
        record = {f"{lpl}/{size}": sel for (lpl, size), sel in zip(keys, pool.starmap(select, keys))}
    for lpl in model.LPLS:
        for size in SIZES:
            reached = set().union(*(set(c[2]) for c in record[f"{lpl}/{size}"]))
            print(lpl, size, size_bits(lpl, size), "bits:", len(record[f"{lpl}/{size}"]), "cases; not reached:",
                  sorted(set(model.EVENTS) - reached), flush=True)
    STORE.write_text(json.dumps(record, separators=(",", ":")) + "\n")
