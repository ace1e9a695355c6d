#!/usr/bin/env python3
"""Model of the range proofs for Paillier ciphertexts (protocols/distributed_keygen_amd/range_proof.py) in Python ints
and hashlib — developer tool and the oracle of tests/test_range_proof_host.py and tests/test_gpu_range_proofs.py.

The proof is the Paillier range proof with a Pedersen commitment over an auxiliary RSA modulus (Fujisaki-Okamoto 1997,
MacKenzie-Reiter 2001; Pi^enc of Canetti-Gennaro-Goldfeder-Makriyannis-Peled 2021, Fig. 14) with unsigned values.

    parameters  Nh = ph qh, ph = 2ph' + 1 and qh = 2qh' + 1 safe primes; t = tau^2 mod Nh for a random unit tau;
                s = t^lambda mod Nh for a random lambda < ph' qh'.  The prover knows (Nh, s, t) only.
                Bh = bits(Nh), E = 128 (challenge), K = 128 (hiding margin), l = the claimed bit length.
    statement   c = (1 + N)^m r^N mod N^2 with 0 <= m < 2^l; the prover knows m and r.  l + E + K + 2 <= bits(N) - 1.
    prove       alpha < 2^(l + E + K),  mu < 2^(Bh + K),  gamma < 2^(Bh + E + 2K),  rho = rho' mod N for a draw rho' of
                bits(N) + 64 bits (the way encrypt_fresh_batch draws its r)
                S = s^m t^mu mod Nh,   A = (1 + N)^alpha rho^N mod N^2,   C = s^alpha t^gamma mod Nh
                e = first 16 bytes of SHA-256(ctx | BE(c) | BE(S) | BE(A) | BE(C)) as a big-endian integer
                z1 = alpha + e m,   z2 = rho r^e mod N,   z3 = gamma + e mu          (z1, z3 over the integers)
                the proof is (S, A, C, z1, z2, z3)
    verify      S, C < Nh;  A, c < N^2;  z2 < N;  z1 < 2^(l + E + K + 1);  z3 < 2^(Bh + E + 2K + 1)
                (1 + N)^z1 z2^N = A c^e (mod N^2);   s^z1 t^z3 = C S^e (mod Nh)        (e recomputed)

BE(x) is x as a big-endian integer of 4 * limbs bytes at the value's OWN row width: limbs(N^2) for c and A, limbs(Nh)
for S and C.  ctx, 32 bytes, binds a proof to the key, the parameters, the claimed length and the caller's label:

    ctx = SHA-256(LP(TAG) | LP(N) | LP(Nh) | LP(s) | LP(t) | LP(l) | LP(label))
    LP(bytes) = 4-byte big-endian length | bytes;  an integer is its minimal big-endian bytes (one zero byte for 0)

Draw order on a device generator (device_rng.DeviceRng: one call number per draw): call c alpha, c + 1 mu, c + 2 gamma,
c + 3 rho' — rows of ceil(bits / 32) words, rho' in rows of limbs(N^2) words.

The parameter proof (s in <t>): 128 rounds with binary challenges.  r_i < ph' qh', a_i = t^(r_i); the challenge bits are
the first 128 bits of SHA-256(LP(PTAG) | LP(Nh) | LP(s) | LP(t) | LP(a_0) | .. | LP(a_127)); z_i = r_i + e_i lambda mod
ph' qh'; check t^(z_i) = a_i s^(e_i).
"""
from __future__ import annotations

import hashlib
import math
from typing import List, Sequence, Tuple

E_BITS = 128                     # challenge width
K_BITS = 128                     # statistical hiding margin
ROUNDS = 128                     # rounds of the parameter proof
TAG = b"mxpaillier/range-proof/v1"
PTAG = b"mxpaillier/range-parameters/v1"


def limbs_for(value: int) -> int:
    return max(1, (int(value).bit_length() + 31) // 32)


def be_row(value: int, limbs: int) -> bytes:
    return int(value).to_bytes(4 * limbs, "big")


def _lp(data: bytes) -> bytes:
    return len(data).to_bytes(4, "big") + data


def _int_bytes(x: int) -> bytes:
    return int(x).to_bytes(max(1, (int(x).bit_length() + 7) // 8), "big")


class Parameters:
    """The public part (Nh, s, t)."""

    def __init__(self, nh: int, s: int, t: int) -> None:
        self.nh, self.s, self.t = int(nh), int(s), int(t)
        self.bits = self.nh.bit_length()
        self.limbs = limbs_for(self.nh)


def make_parameters(ph: int, qh: int, lam: int, tau: int) -> Parameters:
    nh = ph * qh
    t = tau * tau % nh
    return Parameters(nh, pow(t, lam, nh), t)


def context(n: int, par: Parameters, bits: int, label: bytes) -> bytes:
    fields = [_int_bytes(x) for x in (n, par.nh, par.s, par.t, bits)] + [bytes(label)]
    return hashlib.sha256(_lp(TAG) + b"".join(_lp(f) for f in fields)).digest()


def shape(n: int, par: Parameters, bits: int) -> dict:
    """Bit lengths and row widths of everything a proof holds."""
    if bits < 1 or bits + E_BITS + K_BITS + 2 > n.bit_length() - 1:
        raise ValueError("l + E + K + 2 <= bits(N) - 1 expected")
    out = dict(alpha_bits=bits + E_BITS + K_BITS, mu_bits=par.bits + K_BITS, gamma_bits=par.bits + E_BITS + 2 * K_BITS,
               rho_bits=n.bit_length() + 64)
    out.update(z1_bits=out["alpha_bits"] + 1, z3_bits=out["gamma_bits"] + 1)
    out.update(z1_words=-(-out["z1_bits"] // 32), z3_words=-(-out["z3_bits"] // 32), limbs_n=limbs_for(n), limbs2=limbs_for(n * n),
               limbs_h=par.limbs)
    return out


def challenge(ctx: bytes, c: int, s_: int, a: int, c_: int, limbs2: int, limbs_h: int) -> int:
    h = hashlib.sha256(ctx + be_row(c, limbs2) + be_row(s_, limbs_h) + be_row(a, limbs2) + be_row(c_, limbs_h)).digest()
    return int.from_bytes(h[:16], "big")


def encrypt(n: int, message: int, r: int) -> int:
    n2 = n * n
    return (1 + message * n) % n2 * pow(r, n, n2) % n2


def prove(n: int, par: Parameters, bits: int, label: bytes, m: int, r: int, alpha: int, mu: int, gamma: int, rho_draw: int,
          c: int = None) -> Tuple[int, int, int, int, int, int]:
    """(S, A, C, z1, z2, z3) for c = encrypt(n, m, r) and the four draws.  The honest algorithm for ANY m >= 0: a
    message of 2^l or more still gives a proof, which verifies while z1 stays below its bound (the slack)."""
    sh = shape(n, par, bits)
    for v, b in ((alpha, sh["alpha_bits"]), (mu, sh["mu_bits"]), (gamma, sh["gamma_bits"]), (rho_draw, sh["rho_bits"])):
        if v < 0 or v >> b:
            raise ValueError("a draw is out of range")
    if m < 0:
        raise ValueError("m >= 0 expected (a signed value v is proven as v + 2^(l - 1))")
    n2, nh = n * n, par.nh
    rho = rho_draw % n
    if c is None:
        c = encrypt(n, m, r)
    s_ = pow(par.s, m, nh) * pow(par.t, mu, nh) % nh
    a = (1 + alpha * n) % n2 * pow(rho, n, n2) % n2
    c_ = pow(par.s, alpha, nh) * pow(par.t, gamma, nh) % nh
    e = challenge(context(n, par, bits, label), c, s_, a, c_, sh["limbs2"], sh["limbs_h"])
    return s_, a, c_, alpha + e * m, rho * pow(r % n, e, n) % n, gamma + e * mu


def in_range(n: int, par: Parameters, bits: int, c: int, proof: Sequence[int]) -> bool:
    """The range checks of verify, which come before any arithmetic on the row."""
    sh = shape(n, par, bits)
    s_, a, c_, z1, z2, z3 = proof
    n2, nh = n * n, par.nh
    if not (0 <= s_ < nh and 0 <= c_ < nh and 0 <= a < n2 and 0 <= c < n2 and 0 <= z2 < n):
        return False
    return 0 <= z1 < 1 << sh["z1_bits"] and 0 <= z3 < 1 << sh["z3_bits"]


def verify(n: int, par: Parameters, bits: int, label: bytes, c: int, proof: Sequence[int]) -> bool:
    sh = shape(n, par, bits)
    s_, a, c_, z1, z2, z3 = proof
    n2, nh = n * n, par.nh
    if not in_range(n, par, bits, c, proof):
        return False
    e = challenge(context(n, par, bits, label), c, s_, a, c_, sh["limbs2"], sh["limbs_h"])
    if (1 + z1 * n) % n2 * pow(z2, n, n2) % n2 != a * pow(c, e, n2) % n2:
        return False
    return pow(par.s, z1, nh) * pow(par.t, z3, nh) % nh == c_ * pow(s_, e, nh) % nh


def device_draws(key: bytes, call: int, count: int, n: int, par: Parameters, bits: int) -> Tuple[List[int], ...]:
    """(alpha, mu, gamma, rho') of `count` rows as DeviceRng(key, first_call=call) gives them to Engine.range_prove_t."""
    import chacha_model

    sh = shape(n, par, bits)
    return (chacha_model.row_ints(key, call, count, sh["alpha_bits"]), chacha_model.row_ints(key, call + 1, count, sh["mu_bits"]),
            chacha_model.row_ints(key, call + 2, count, sh["gamma_bits"]),
            chacha_model.row_ints(key, call + 3, count, sh["rho_bits"], sh["limbs2"]))


# ---- the parameter proof ------------------------------------------------------------------------------------------------
def parameter_challenge(par: Parameters, commitments: Sequence[int]) -> List[int]:
    msg = _lp(PTAG) + b"".join(_lp(_int_bytes(x)) for x in (par.nh, par.s, par.t, *commitments))
    bits = int.from_bytes(hashlib.sha256(msg).digest()[: ROUNDS // 8], "big")
    return [(bits >> (ROUNDS - 1 - i)) & 1 for i in range(ROUNDS)]


def prove_parameters(par: Parameters, ph: int, qh: int, lam: int, rand) -> Tuple[List[int], List[int]]:
    """(a_0 .. a_127, z_0 .. z_127); `rand` has randrange; draw order r_0 .. r_127."""
    order = ((ph - 1) // 2) * ((qh - 1) // 2)
    rs = [rand.randrange(order) for _ in range(ROUNDS)]
    commitments = [pow(par.t, r, par.nh) for r in rs]
    es = parameter_challenge(par, commitments)
    return commitments, [(r + e * lam) % order for r, e in zip(rs, es)]


def verify_parameters(par: Parameters, proof: Tuple[Sequence[int], Sequence[int]]) -> bool:
    commitments, zs = proof
    nh = par.nh
    if nh < 3 or nh % 2 == 0 or len(commitments) != ROUNDS or len(zs) != ROUNDS:
        return False
    if not (0 < par.s < nh and 0 < par.t < nh and math.gcd(par.s, nh) == 1 and math.gcd(par.t, nh) == 1):
        return False
    if any(not 0 < a < nh for a in commitments) or any(not 0 <= z < nh for z in zs):
        return False
    es = parameter_challenge(par, commitments)
    return all(pow(par.t, z, nh) == a * (par.s if e else 1) % nh for a, z, e in zip(commitments, zs, es))


# ---- the parameters of tests/golden/range_params.json -----------------------------------------------------------------------
def golden_parameters(seed: int) -> dict:
    """A pair of 64-bit safe primes (other than those of tests/golden/threshold_keys.json at key length 128), lambda
    and tau from a seeded search: find_safe_prime of tools/proof_model.py over random.Random(seed)."""
    import random

    import proof_model

    rand = random.Random(seed)
    taken = {0xF5B0124F8C69215B, 0xE2FCE1351448C67B}
    primes: List[int] = []
    while len(primes) < 2:
        p = proof_model.find_safe_prime(64, rand)
        if p not in taken and p not in primes:
            primes.append(p)
    ph, qh = primes
    nh = ph * qh
    assert nh.bit_length() == 128
    lam = rand.randrange(((ph - 1) // 2) * ((qh - 1) // 2))
    while True:
        tau = rand.randrange(2, nh)
        if math.gcd(tau, nh) == 1:
            break
    return {"seed": seed, "provenance": "tools/range_model.py: golden_parameters(seed) over random.Random(seed) — a seeded search, "
            "nothing secret", "p": format(ph, "x"), "q": format(qh, "x"), "lambda": format(lam, "x"), "tau": format(tau, "x")}


if __name__ == "__main__":
    import json
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    print(json.dumps(golden_parameters(int(sys.argv[1]) if len(sys.argv) > 1 else 20261020), indent=1))
