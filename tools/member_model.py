#!/usr/bin/env python3
"""Model of the one-of-k membership proofs for Paillier ciphertexts (protocols/distributed_keygen_amd/membership.py) in
Python ints and hashlib — developer tool and the oracle of tests/test_membership_host.py and tests/test_gpu_membership.py.

The proof is the Cramer-Damgard-Schoenmakers OR-composition of the Sigma-protocol for N-th residues (Damgard-Jurik 2001
§5; Baudron-Fouque-Pointcheval-Poupard-Stern 2001): the sender proves that c encrypts one of the public values
S = (s_0 .. s_(k-1)), exactly, without saying which.

    public      odd N; S with 2 <= k <= 16, the s_j distinct and 0 <= s_j < N; a label.  E = 128 (challenge width).
    statement   c = (1 + N)^(s_i) r^N mod N^2 for some i the prover knows, together with r.
                u_j = c (1 + (N - s_j) N) mod N^2  [= c (1 + N)^(-s_j)],   ub_j = c^-1 (1 + s_j N) mod N^2  [= u_j^-1]
    prove       zt_j of bits(N) + 64 bits for all j (slot i's serves as omega);  et_j of 128 bits for all j, then et_i = 0
                a_j = zt_j^N ub_j^(et_j) mod N^2 for all j                                   (slot i: omega^N)
                e = first 16 bytes of SHA-256(ctx | BE(c) | BE(A)) as a big-endian integer
                e_i = e - sum_(j != i) et_j mod 2^128,  e_j = et_j otherwise
                z_i = (omega mod N) r^(e_i) mod N,      z_j = zt_j mod N otherwise
                the proof is (a_j, e_j, z_j) for j < k
    verify      c < N^2;  0 < a_j < N^2 and 0 < z_j < N for all j;  sum_j e_j = e (mod 2^128) with e recomputed;
                z_j^N = a_j u_j^(e_j) (mod N^2) for all j

ZERO IS REFUSED: a_j = z_j = 0 satisfies 0^N = 0 u_j^(e_j) for ANY c and any e_j, so without the check anybody forges a
proof for any ciphertext (all slots zero, or one zero slot beside k - 1 simulated ones with the challenge re-split).
Special soundness needs z_j a unit modulo N; with every prime factor of N above 2^128 a nonzero non-unit would factor N,
so zero is the only non-unit that needs a check — and z_j != 0 forces z_j^N != 0 (mod N^2), hence a_j != 0, which is
checked all the same.  An honest z_j is zero with probability 2^-bits(N).

BE(c) is c as a big-endian integer of 4 limbs(N^2) bytes.  A is ONE row of k limbs(N^2) little-endian words, a_j in words
j limbs(N^2) .. (j + 1) limbs(N^2) - 1 — the integer sum_j a_j 2^(32 limbs(N^2) j) — and BE(A) is that row as a big-endian
integer of 4 k limbs(N^2) bytes: the bytes of a_(k-1) come first and those of a_0 last.  Any k is one row set of the hash.
ctx, 32 bytes, binds a proof to the key, the list S IN ITS ORDER and the caller's label:

    ctx = SHA-256(LP(TAG) | LP(N) | LP(k) | LP(s_0) | .. | LP(s_(k-1)) | LP(label))
    LP(bytes) = 4-byte big-endian length | bytes;  an integer is its minimal big-endian bytes (one zero byte for 0)

Draw order on a device generator (device_rng.DeviceRng: one call number per draw): call c the zt — count k rows of
bits(N) + 64 bits at the width limbs(N^2), row r k + j for slot j of ciphertext r —, call c + 1 the et — count k rows of
128 bits.  Both are drawn for EVERY slot, the real one included: what is drawn does not depend on i.
"""
from __future__ import annotations

import hashlib
from typing import List, Sequence, Tuple

E_BITS = 128                     # challenge width
MIN_K, MAX_K = 2, 16
TAG = b"mxpaillier/membership/v1"
M128 = (1 << E_BITS) - 1


def limbs_for(value: int) -> int:
    return max(1, (int(value).bit_length() + 31) // 32)


def be_row(value: int, limbs: int) -> bytes:
    return int(value).to_bytes(4 * limbs, "big")


def _lp(data: bytes) -> bytes:
    return len(data).to_bytes(4, "big") + data


def _int_bytes(x: int) -> bytes:
    return int(x).to_bytes(max(1, (int(x).bit_length() + 7) // 8), "big")


def check_values(n: int, values: Sequence[int]) -> None:
    k = len(values)
    if n < 3 or n % 2 == 0:
        raise ValueError("N must be odd")
    if not MIN_K <= k <= MAX_K:
        raise ValueError("2 <= k <= 16 expected")
    if len(set(values)) != k or any(not 0 <= s < n for s in values):
        raise ValueError("distinct values in [0, N) expected")


def context(n: int, values: Sequence[int], label: bytes) -> bytes:
    fields = [_int_bytes(n), _int_bytes(len(values))] + [_int_bytes(s) for s in values] + [bytes(label)]
    return hashlib.sha256(_lp(TAG) + b"".join(_lp(f) for f in fields)).digest()


def shape(n: int, k: int) -> dict:
    """Bit lengths and row widths of everything a proof holds."""
    if not MIN_K <= k <= MAX_K:
        raise ValueError("2 <= k <= 16 expected")
    return dict(k=k, draw_bits=n.bit_length() + 64, e_bits=E_BITS, e_words=E_BITS // 32, limbs_n=limbs_for(n), limbs2=limbs_for(n * n))


def challenge(ctx: bytes, c: int, a: Sequence[int], limbs2: int) -> int:
    row = sum(int(v) << (32 * limbs2 * j) for j, v in enumerate(a))
    h = hashlib.sha256(ctx + be_row(c, limbs2) + be_row(row, limbs2 * len(a))).digest()
    return int.from_bytes(h[:16], "big")


def encrypt(n: int, message: int, r: int) -> int:
    n2 = n * n
    return (1 + message * n) % n2 * pow(r, n, n2) % n2


def branches(n: int, values: Sequence[int], c: int) -> List[int]:
    """u_j = c (1 + (N - s_j) N) mod N^2: what is an N-th residue exactly for the value c holds."""
    n2 = n * n
    return [c * (1 + (n - s) * n) % n2 for s in values]


def prove(n: int, values: Sequence[int], label: bytes, i: int, r: int, z_draws: Sequence[int], e_draws: Sequence[int],
          c: int = None) -> Tuple[List[int], List[int], List[int]]:
    """(a, e, z), k entries each, for c = encrypt(n, values[i], r) and the two draws of k entries each."""
    check_values(n, values)
    k = len(values)
    sh = shape(n, k)
    if not 0 <= i < k or len(z_draws) != k or len(e_draws) != k:
        raise ValueError("a slot in [0, k) and k draws of each kind expected")
    if any(v < 0 or v >> sh["draw_bits"] for v in z_draws) or any(v < 0 or v >> E_BITS for v in e_draws):
        raise ValueError("a draw is out of range")
    n2 = n * n
    if c is None:
        c = encrypt(n, values[i], r)
    cinv = pow(c, -1, n2)
    sim = [0 if j == i else e_draws[j] for j in range(k)]
    a = [pow(z_draws[j], n, n2) * pow(cinv * (1 + values[j] * n) % n2, sim[j], n2) % n2 for j in range(k)]
    e = challenge(context(n, values, label), c, a, sh["limbs2"])
    es = list(sim)
    es[i] = (e - sum(sim)) & M128
    zs = [zd % n for zd in z_draws]
    zs[i] = zs[i] * pow(r % n, es[i], n) % n
    return a, es, zs


def in_range(n: int, k: int, c: int, proof: Sequence[Sequence[int]]) -> bool:
    """The range checks of verify, which come before any arithmetic on the row."""
    a, es, zs = proof
    n2 = n * n
    if len(a) != k or len(es) != k or len(zs) != k or not 0 <= c < n2:
        return False
    return all(0 < v < n2 for v in a) and all(0 < v < n for v in zs) and all(0 <= v <= M128 for v in es)


def verify(n: int, values: Sequence[int], label: bytes, c: int, proof: Sequence[Sequence[int]]) -> bool:
    check_values(n, values)
    k = len(values)
    if not in_range(n, k, c, proof):
        return False
    a, es, zs = proof
    n2 = n * n
    if sum(es) & M128 != challenge(context(n, values, label), c, a, shape(n, k)["limbs2"]):
        return False
    return all(pow(z, n, n2) == aj * pow(u, e, n2) % n2 for z, aj, u, e in zip(zs, a, branches(n, values, c), es))


# ---- the challenge arithmetic of csrc/mx_member.hpp, on lists of ints ------------------------------------------------------
def challenges(mode: int, e: Sequence[int], sim: Sequence[Sequence[int]], index: Sequence[int]):
    """mode 0 (mask): rows of sim with slot index[r] zeroed; 1 (split): that slot = e[r] - the sum of the others mod
    2^128; 2 (sum): [1 if the sum of row r mod 2^128 differs from e[r] else 0]."""
    if mode == 2:
        return [int(sum(row) & M128 != ev) for row, ev in zip(sim, e)]
    out = []
    for r, row in enumerate(sim):
        row = [0 if j == index[r] else v for j, v in enumerate(row)]
        if mode == 1 and 0 <= index[r] < len(row):
            row[index[r]] = (e[r] - sum(row)) & M128
        out.append(row)
    return out


def device_draws(key: bytes, call: int, count: int, n: int, k: int) -> Tuple[List[List[int]], List[List[int]]]:
    """(zt, et), `count` lists of k, as DeviceRng(key, first_call=call) gives them to Engine.member_prove_t."""
    import chacha_model

    sh = shape(n, k)
    zt = chacha_model.row_ints(key, call, count * k, sh["draw_bits"], sh["limbs2"])
    et = chacha_model.row_ints(key, call + 1, count * k, E_BITS)
    return [zt[r * k : (r + 1) * k] for r in range(count)], [et[r * k : (r + 1) * k] for r in range(count)]


if __name__ == "__main__":
    import random

    rnd = random.Random(1)
    p, q = 0xF5B0124F8C69215B, 0xE2FCE1351448C67B          # tests/golden/threshold_keys.json, key length 128
    n_, vals = p * q, [0, 1, 1 << 16]
    for i_ in range(3):
        r_ = rnd.randrange(1, n_)
        pf = prove(n_, vals, b"demo", i_, r_, [rnd.getrandbits(192) for _ in vals], [rnd.getrandbits(128) for _ in vals])
        c_ = encrypt(n_, vals[i_], r_)
        print(i_, verify(n_, vals, b"demo", c_, pf), verify(n_, vals, b"demo", c_ * (1 + n_) % (n_ * n_), pf))
