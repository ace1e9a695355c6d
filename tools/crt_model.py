"""Python model of the two kernels of the private-key CRT decryption (csrc/mx_crt.hpp) at the level of their Montgomery
products and plan constants: which radix, which cut, which operand bounds.  Every product asserts the bound the kernel
relies on, so running the model over unequal prime lengths checks the analysis, not only the results.

    Paillier 1999, section 7, for N = p q and a ciphertext c:
        x_p = (c mod p^2)^(p-1) mod p^2      m_p = L_p(x_p) h_p mod p       L_p(x) = (x - 1) / p
        x_q = (c mod q^2)^(q-1) mod q^2      m_q = L_q(x_q) h_q mod q
        m   = m_p + p ((m_q - m_p) p^-1 mod q)                              (Garner)
        h_p = L_p((N + 1)^(p-1) mod p^2)^-1 mod p,  h_q likewise

Lane geometry (csrc/mx_host.hpp: choose_geometry): limbs of W = 29 bits, L = 9 per lane, a Montgomery radix
R = 2^(W L b) with b blocks, R >= 16 * modulus.  ONE radix serves both primes in each kernel — it is chosen from the
longer prime — so a q^2 that is wider than p^2 can never exceed "the R of p^2":

  split      Rs = 2^rs with rs >= max(bits(p^2), bits(q^2), 16 limbs2) + 4.  A row c of limbs2 words (ANY value below
             2^(32 limbs2)) is cut at s = 16 limbs2 into lo, hi < 2^s <= Rs / 16.  Per prime square P:
                 h = mont(hi, 2^s Rs mod P)     = hi 2^s,  < 2 P      (a < Rs, b < P  =>  a b / Rs + P < 2 P)
                 t = lo + h                     < Rs / 16 + Rs / 8 < Rs
                 u = mont(t, Rs^2 mod P)        = c Rs,    < 2 P
                 c mod P = mont(u, 1), one conditional subtraction behind it
  recombine  R1 = 2^r1 with r1 >= max(bits(p), bits(q)) + 4, in lane groups that hold a number of the half width.
             Per prime r (x < r^2 as the modexp left it):
                 y = x - 1;  (rem, Q) = REDC_r(y) with y + Q r = rem R1;  r | y  <=>  rem in {0, r}  (rem < y / R1 + r)
                 u = (R1 - Q) mod R1 = y / r  (0 for rem = 0)
                 m_r = mont(u, h_r R1 mod r), < 2 r            (canonical for p: it is a summand of the result)
             Garner modulo q — m_p < p may exceed q, and even R1 / 16 > q, which is why R1 comes from the longer prime:
                 a = mont(m_p, R1 mod q)        = m_p mod q, < 2 q    (m_p < p <= R1 / 16  =>  m_p q / R1 + q < 2 q)
                 d = m_q + 2 q - a              in (0, 4 q)
                 t = mont(d, p^-1 R1 mod q)     = (m_q - m_p) p^-1, < 2 q, made canonical
             m = m_p + p t: a plain product and an add, canonical in [0, N) because m_p < p and t <= q - 1.

Private-key ENCRYPTION (csrc/mx_crt_enc.hpp).  Z*_{p^2} = C_{p-1} x C_p and x -> x^p mod p^2 depends on
x mod p only, multiplicatively, so the reference's randomiser r^N mod N^2 is, modulo p^2,
        rho_p = ((r mod p)^(q mod (p-1)) mod p)^p mod p^2,   rho_q likewise
— one modexp modulo p and one modulo p^2 with the exponent p — and a key holder's own randomness needs the second only:
rho_p = (D mod p^2)^p.  Around these modexps stand (CrtEncPlan):

  prime split  the split above with the primes in place of their squares and the radix of ITS launch: Rp = 2^rp with
             rp >= max(bits(p), bits(q), 16 limbs_r) + 4 for randomness rows of limbs_r words (any value of that width).
  lift       R = 2^r2 with r2 >= 2 max(bits(p), bits(q)) + 4, lane groups that hold a half.  Per prime square P, with the
             factor v in front of the noise (a message row m < N, a ciphertext half v < P, or nothing):
                 a = mont(m, N R^2 mod P) + (R mod P)   = (1 + m N) R,  < 3 P < R      (m < N <= R / 16)
                 a = mont(v, R^2 mod P)                 = v R,          < 2 P
                 c_P = mont(a, rho_P)                   = v rho_P,      < 2 P          (rho_P < P; a < R)
             c_p is made canonical (a summand of the result), c_q stays lazy.  Garner modulo Q = q^2 as above:
                 a' = mont(c_p, R mod Q), < 2 Q;   d = c_q + 2 Q - a' in (0, 4 Q);   t = mont(d, (p^2)^-1 R mod Q), canonical
             c = c_p + p^2 t by a plain product, canonical in [0, N^2).  status bit 0: rho_p = 0, bit 1: rho_q = 0 — p or q
             divides the randomness — and the row is zero then.
"""

from __future__ import annotations

import math
import random
from typing import List, Tuple

W, L = 29, 9
MAX_MOD_BITS = W * L * 64 - 4


def limbs_for(v: int) -> int:
    return max(1, (v.bit_length() + 31) // 32)


def geometry(bits: int) -> Tuple[int, int]:
    """(lanes per element, blocks) of choose_geometry(bits) at 9 limbs per lane."""
    if bits < 2 or bits > MAX_MOD_BITS:
        raise ValueError("no lane geometry for this width")
    nblk = -(-(bits + 4) // (W * L))
    k = 1
    while k < nblk:
        k <<= 1
    return k, nblk


def h_constant(p: int, n: int) -> int:
    """h_p = L_p((N + 1)^(p-1) mod p^2)^-1 mod p (ValueError where it does not exist)."""
    return pow((pow(n + 1, p - 1, p * p) - 1) // p, -1, p)


def mont(a: int, b: int, mod: int, rbits: int) -> Tuple[int, int]:
    """(a b + Q mod) / R with the quotient Q = -a b mod^-1 mod R the word-serial product records."""
    r = 1 << rbits
    q = (-a * b * pow(mod, -1, r)) % r
    t = a * b + q * mod
    assert t % r == 0
    return t >> rbits, q


class CrtPlan:
    """What mx_crt_prepare derives from (p, q, h_p, h_q, p^-1 mod q) and the width of the ciphertext rows."""

    def __init__(self, p: int, q: int, limbs2: int = 0) -> None:
        if p % 2 == 0 or q % 2 == 0 or p < 3 or q < 3 or p == q:
            raise ValueError("two different odd primes are needed")
        self.p, self.q, self.n = p, q, p * q
        self.limbs_n = limbs_for(self.n)
        self.limbs2 = limbs2 or limbs_for(self.n * self.n)
        if self.limbs2 < limbs_for(self.n * self.n):
            raise ValueError("rows narrower than N^2")
        self.limbs_half = max(limbs_for(p * p), limbs_for(q * q))
        prime_bits = max(p.bit_length(), q.bit_length())
        self.half_bits = 2 * prime_bits
        self.hp, self.hq = h_constant(p, self.n), h_constant(q, self.n)
        self.pinv = pow(p, -1, q)
        # split
        self.split_bit = 16 * self.limbs2
        self.ks, nblk_s = geometry(max(self.half_bits, self.split_bit))
        self.rs = W * L * nblk_s
        assert self.limbs2 <= 2 * self.ks * L + 6, "the row must fit the group's staging area"
        self.split_rows = [(sq, pow(2, self.split_bit + self.rs, sq), pow(2, 2 * self.rs, sq)) for sq in (p * p, q * q)]
        # recombine
        self.kr, _ = geometry(self.half_bits)
        self.nblk1 = -(-(prime_bits + 4) // (W * L))
        self.r1 = W * L * self.nblk1
        assert self.nblk1 <= self.kr and self.limbs_half <= 2 * self.kr * L + 6
        self.hp_r = self.hp * (1 << self.r1) % p
        self.hq_r = self.hq * (1 << self.r1) % q
        self.one_q = (1 << self.r1) % q
        self.pinv_r = self.pinv * (1 << self.r1) % q

    # ---- crt_split_kernel
    def split(self, c: int) -> Tuple[int, int]:
        assert 0 <= c < 1 << (32 * self.limbs2)
        rs_val = 1 << self.rs
        lo, hi = c & ((1 << self.split_bit) - 1), c >> self.split_bit
        assert lo < rs_val >> 4 and hi < rs_val >> 4
        out = []
        for sq, k_cut, k_r2 in self.split_rows:
            assert rs_val >= 16 * sq and k_cut < sq and k_r2 < sq
            h, _ = mont(hi, k_cut, sq, self.rs)
            assert h < 2 * sq
            t = lo + h
            assert t < rs_val
            u, _ = mont(t, k_r2, sq, self.rs)
            assert u < 2 * sq
            v, _ = mont(u, 1, sq, self.rs)
            assert v <= sq
            out.append(v - sq if v >= sq else v)
        return out[0], out[1]

    # ---- crt_recombine_kernel
    def _l_times_h(self, x: int, r: int, h_r: int) -> Tuple[int, bool]:
        """(L_r(x) h_r as the lazy residue below 2 r, r divides x - 1) through the quotient-recording reduction."""
        r1_val = 1 << self.r1
        assert 0 <= x < r * r and r1_val >= 16 * r
        if x == 0:
            return 0, False
        y = x - 1
        rem, quo = mont(y, 1, r, self.r1)
        assert rem < y // r1_val + r + 1
        if rem not in (0, r):
            return 0, False
        u = (r1_val - quo) % r1_val if rem == r else 0
        assert u * r == y and u < r
        m, _ = mont(u, h_r, r, self.r1)
        assert m < 2 * r
        return m, True

    def recombine(self, xp: int, xq: int) -> Tuple[int, int]:
        """(m, status): status bit 0 = x_p is not 1 modulo p, bit 1 = x_q is not 1 modulo q; m = 0 with a status."""
        p, q = self.p, self.q
        mp, ok_p = self._l_times_h(xp, p, self.hp_r)
        mq, ok_q = self._l_times_h(xq, q, self.hq_r)
        status = (0 if ok_p else 1) | (0 if ok_q else 2)
        mp = mp - p if mp >= p else mp                       # canonical: a summand of the result
        assert mp < (1 << self.r1) >> 4
        a, _ = mont(mp, self.one_q, q, self.r1)
        assert a < 2 * q and (a - mp) % q == 0
        d = mq + 2 * q - a
        assert 0 < d < 4 * q
        t, _ = mont(d, self.pinv_r, q, self.r1)
        assert t < 2 * q
        t = t - q if t >= q else t
        m = mp + p * t
        assert 0 <= m < self.n
        return (0, status) if status else (m, 0)

    def decrypt(self, c: int) -> Tuple[int, int]:
        cp, cq = self.split(c)
        return self.recombine(pow(cp, self.p - 1, self.p * self.p), pow(cq, self.q - 1, self.q * self.q))


class CrtEncPlan:
    """What mx_crt_enc_prepare derives from (p, q) and the width of the randomness rows: the constants of the prime split
    and of the lift (module docstring), and the two exponents of the modexps modulo the primes."""

    def __init__(self, p: int, q: int, limbs_r: int = 0) -> None:
        if p % 2 == 0 or q % 2 == 0 or p < 3 or q < 3 or p == q:
            raise ValueError("two different odd primes are needed")
        self.p, self.q, self.n = p, q, p * q
        self.n2 = self.n * self.n
        self.limbs_n, self.limbs2 = limbs_for(self.n), limbs_for(self.n2)
        self.limbs_r = limbs_r or self.limbs_n
        self.limbs_half = max(limbs_for(p * p), limbs_for(q * q))
        prime_bits = max(p.bit_length(), q.bit_length())
        self.e_p, self.e_q = q % (p - 1), p % (q - 1)
        assert self.e_p > 0 and self.e_q > 0            # p - 1 is even and q an odd prime: p - 1 never divides q
        # prime split
        self.split_bit = 16 * self.limbs_r
        self.ks, nblk_s = geometry(max(prime_bits, self.split_bit))
        self.rp = W * L * nblk_s
        assert self.limbs_r <= 2 * self.ks * L + 6 and limbs_for(max(p, q)) <= 2 * self.ks * L + 6
        self.split_rows = [(r, pow(2, self.split_bit + self.rp, r), pow(2, 2 * self.rp, r)) for r in (p, q)]
        # lift
        self.kl, self.nblk = geometry(2 * prime_bits)
        self.r2 = W * L * self.nblk
        assert self.nblk <= self.kl and max(self.limbs_half, self.limbs_n) <= 2 * self.kl * L + 6
        big_r = 1 << self.r2
        self.lift_rows = [(sq, self.n * big_r * big_r % sq, big_r % sq, big_r * big_r % sq) for sq in (p * p, q * q)]
        self.p2inv_r = pow(p * p, -1, q * q) * big_r % (q * q)

    # ---- crt_split_kernel over the primes
    def prime_split(self, row: int) -> Tuple[int, int]:
        assert 0 <= row < 1 << (32 * self.limbs_r)
        rp_val = 1 << self.rp
        lo, hi = row & ((1 << self.split_bit) - 1), row >> self.split_bit
        assert lo < rp_val >> 4 and hi < rp_val >> 4
        out = []
        for r, k_cut, k_r2 in self.split_rows:
            assert rp_val >= 16 * r and k_cut < r and k_r2 < r
            h, _ = mont(hi, k_cut, r, self.rp)
            assert h < 2 * r
            t = lo + h
            assert t < rp_val
            u, _ = mont(t, k_r2, r, self.rp)
            assert u < 2 * r
            v, _ = mont(u, 1, r, self.rp)
            assert v <= r
            out.append(v - r if v >= r else v)
        return out[0], out[1]

    # ---- crt_lift_kernel
    def _times_noise(self, half: int, rho: int, m, v) -> int:
        """v rho modulo the square `half` holds, lazy (< 2 P): v = 1 + m N for a message row, the half v, or 1."""
        sq, k_nr2, k_r, k_r2 = self.lift_rows[half]
        big_r = 1 << self.r2
        assert big_r >= 16 * sq and 0 <= rho < sq
        if m is not None:
            assert 0 <= m < self.n and self.n <= big_r >> 4
            a, _ = mont(m, k_nr2, sq, self.r2)
            assert a < 2 * sq
            a += k_r
            assert a < 3 * sq < big_r
        elif v is not None:
            assert 0 <= v < sq
            a, _ = mont(v, k_r2, sq, self.r2)
            assert a < 2 * sq
        else:
            return rho
        c, _ = mont(a, rho, sq, self.r2)
        assert c < 2 * sq
        return c

    def lift(self, rho_p: int, rho_q: int, m=None, halves=None) -> Tuple[int, int]:
        """(c, status) for the noise (rho_p, rho_q) and at most one of a message m < N and a pair of ciphertext halves."""
        assert m is None or halves is None
        p2, q2 = self.p * self.p, self.q * self.q
        status = (1 if rho_p == 0 else 0) | (2 if rho_q == 0 else 0)
        cp = self._times_noise(0, rho_p, m, None if halves is None else halves[0])
        cq = self._times_noise(1, rho_q, m, None if halves is None else halves[1])
        cp = cp - p2 if cp >= p2 else cp                     # canonical: a summand of the result
        big_r = 1 << self.r2
        assert cp < p2 <= big_r >> 4 and cq < 2 * q2
        a, _ = mont(cp, self.lift_rows[1][2], q2, self.r2)
        assert a < 2 * q2 and (a - cp) % q2 == 0
        d = cq + 2 * q2 - a
        assert 0 < d < 4 * q2 < big_r
        t, _ = mont(d, self.p2inv_r, q2, self.r2)
        assert t < 2 * q2
        t = t - q2 if t >= q2 else t
        c = cp + p2 * t
        assert 0 <= c < self.n2 and c.bit_length() <= W * L * (self.nblk + self.kl)
        return (0, status) if status else (c, 0)

    # ---- the routes
    def noise_of_r(self, r: int) -> Tuple[int, int]:
        """(rho_p, rho_q) of the caller's r: the prime split, a modexp modulo each prime, one modulo each square."""
        p, q = self.p, self.q
        rp, rq = self.prime_split(r)
        return pow(pow(rp, self.e_p, p), p, p * p), pow(pow(rq, self.e_q, q), q, q * q)

    def noise_of_draw(self, draw: int) -> Tuple[int, int]:
        """(rho_p, rho_q) of a fresh draw D: (D mod p^2)^p and (D mod q^2)^q."""
        p, q = self.p, self.q
        return pow(draw % (p * p), p, p * p), pow(draw % (q * q), q, q * q)

    def encrypt(self, m: int, r: int) -> Tuple[int, int]:
        return self.lift(*self.noise_of_r(r), m=m % self.n)


def formula_lift(p: int, q: int, rho_p: int, rho_q: int, m=None, halves=None) -> Tuple[int, int]:
    """The lift on Python ints with `%`: (c, status)."""
    n, p2, q2 = p * q, p * p, q * q
    status = (1 if rho_p == 0 else 0) | (2 if rho_q == 0 else 0)
    if status:
        return 0, status
    vp, vq = (1, 1) if m is None and halves is None else ((1 + m * n) % p2, (1 + m * n) % q2) if halves is None else halves
    cp, cq = vp * rho_p % p2, vq * rho_q % q2
    return cp + p2 * ((cq - cp) * pow(p2, -1, q2) % q2), 0


def edge_randomness(p: int, q: int, limbs_r: int, rng: random.Random) -> List[int]:
    n = p * q
    top = 1 << (32 * limbs_r)
    return [v % top for v in (0, 1, p, q, n - 1, n, top - 1, 7 * p, 5 * q, rng.getrandbits(32 * limbs_r), rng.randrange(1, n))]


def enc_check(p: int, q: int, seed: int = 5, extra_words: int = 0) -> int:
    """The encryption model against `%`, `pow` and the formulas for one key; returns the number of values checked."""
    rng = random.Random(seed)
    n, p2, q2 = p * q, p * p, q * q
    n2 = n * n
    plan = CrtEncPlan(p, q, limbs_for(n) + extra_words)
    count = 0
    for r in edge_randomness(p, q, plan.limbs_r, rng):
        assert plan.prime_split(r) == (r % p, r % q)
        count += 1
    # r^N through the two short chains, bit for bit
    r0 = rng.randrange(2, n)
    for r in (1, 2, n - 1, r0, r0 + 3 * n):
        if r >= 1 << (32 * plan.limbs_r):
            continue
        rho = plan.noise_of_r(r)
        assert plan.lift(*rho) == (pow(r, n, n2), 0)
        for m in (0, 1, n - 1, rng.randrange(n)):
            assert plan.encrypt(m, r) == ((1 + m * n) * pow(r, n, n2) % n2, 0)
        count += 1
    # the lift on directed noise, all three modes
    small, big = (p2, q2) if p2 < q2 else (q2, p2)
    noise = [(1, 1), (p2 - 1, q2 - 1), (rng.randrange(1, p2), rng.randrange(1, q2)), (p2 - 1, 1), (1, q2 - 1),
             (p2 - 1 if p2 > q2 else rng.randrange(1, p2), 1),      # rho_p above q^2 in the swapped order
             (small - 1, 1), (p2 - 2, 2)]                           # rho_q below c_p mod q^2: the negative difference
    for rho_p, rho_q in noise:
        for m in (None, 0, 1, n - 1, rng.randrange(n)):
            assert plan.lift(rho_p, rho_q, m=m) == formula_lift(p, q, rho_p, rho_q, m=m)
        c = rng.randrange(n2)
        halves = (c % p2, c % q2)
        want = c * formula_lift(p, q, rho_p, rho_q)[0] % n2
        assert plan.lift(rho_p, rho_q, halves=halves) == (want, 0) == formula_lift(p, q, rho_p, rho_q, halves=halves)
        count += 1
    for rho_p, rho_q, st in ((0, 1, 1), (1, 0, 2), (0, 0, 3), (0, q2 - 1, 1)):
        for m in (None, 5):
            assert plan.lift(rho_p, rho_q, m=m) == (0, st)
        count += 1
    for r, st in ((0, 3), (7 * p, 1), (5 * q, 2)):
        assert plan.encrypt(3, r) == (0, st)
        count += 1
    # fresh draws: a uniform N-th residue — its lambda-th power is 1, the ciphertext decrypts, and r comes back
    lam = (p - 1) * (q - 1)
    for _ in range(3):
        draw = rng.getrandbits(n.bit_length() + 64)
        rho, st = plan.lift(*plan.noise_of_draw(draw))
        if st:
            continue
        assert pow(rho, lam, n2) == 1
        m = rng.randrange(n)
        c, _ = plan.lift(*plan.noise_of_draw(draw), m=m)
        assert c == (1 + m * n) * rho % n2 and lambda_decrypt(c, p, q) == m
        r = pow(rho, pow(n, -1, lam), n)
        assert pow(r, n, n2) == rho
        count += 1
    return count


def formula_decrypt(c: int, p: int, q: int) -> Tuple[int, int]:
    """The formulas of the docstring on Python ints with `%`: (m, status)."""
    n = p * q
    xp, xq = pow(c % (p * p), p - 1, p * p), pow(c % (q * q), q - 1, q * q)
    status = (0 if xp % p == 1 else 1) | (0 if xq % q == 1 else 2)
    if status:
        return 0, status
    mp = (xp - 1) // p * h_constant(p, n) % p
    mq = (xq - 1) // q * h_constant(q, n) % q
    return mp + p * ((mq - mp) * pow(p, -1, q) % q), 0


def lambda_decrypt(c: int, p: int, q: int) -> int:
    """pow(c, lambda, N^2) and the division, the route without the factors' structure (gcd(c, N) = 1)."""
    n, lam = p * q, (p - 1) * (q - 1)
    return (pow(c, lam, n * n) - 1) // n * pow(lam, -1, n) % n


def _is_prime(v: int, rng: random.Random) -> bool:
    if v < 2 or any(v % s == 0 and v != s for s in (2, 3, 5, 7, 11, 13)):
        return v in (2, 3, 5, 7, 11, 13)
    d, s = v - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(24):
        x = pow(rng.randrange(2, v - 1), d, v)
        if x in (1, v - 1):
            continue
        for _ in range(s - 1):
            x = x * x % v
            if x == v - 1:
                break
        else:
            return False
    return True


def prime_of_bits(bits: int, rng: random.Random) -> int:
    while True:
        v = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if _is_prime(v, rng):
            return v


def key_of_bits(p_bits: int, q_bits: int, seed: int = 1) -> Tuple[int, int]:
    """Two different primes of exactly these lengths with gcd(pq, (p-1)(q-1)) = 1, from a seed."""
    rng = random.Random(seed * 7919 + p_bits * 131 + q_bits)
    while True:
        p, q = prime_of_bits(p_bits, rng), prime_of_bits(q_bits, rng)
        if p != q and math.gcd(p * q, (p - 1) * (q - 1)) == 1:
            return p, q


def edge_ciphertexts(p: int, q: int, limbs2: int, rng: random.Random) -> List[int]:
    n2 = (p * q) ** 2
    return [0, 1, n2 - 1, (1 << (32 * limbs2)) - 1, rng.getrandbits(31), 5 * p * p, 3 * q * q + 1, 7 * p,
            rng.getrandbits(32 * limbs2)] + [rng.randrange(n2) for _ in range(4)]


def check(p: int, q: int, seed: int = 5, extra_words: int = 0) -> int:
    """Model against `%`, the formulas and the lambda route for one key; returns the number of values checked."""
    rng = random.Random(seed)
    n = p * q
    plan = CrtPlan(p, q, limbs_for(n * n) + extra_words)
    count = 0
    for c in edge_ciphertexts(p, q, plan.limbs2, rng):
        assert plan.split(c) == (c % (p * p), c % (q * q))
        assert plan.decrypt(c) == formula_decrypt(c, p, q)
        if math.gcd(c, n) == 1:
            assert plan.decrypt(c) == (lambda_decrypt(c, p, q), 0)
        count += 1
    for m in (0, 1, n - 1, p, q, p - 1, q - 1, n - p, n - q, rng.randrange(n)):
        c = (1 + m * n) * pow(rng.randrange(1, n), n, n * n) % (n * n)
        assert plan.decrypt(c) == (m, 0)
        count += 1
    for xp, xq in ((1, 1), (1 + p * (p - 1), 1), (1, 1 + q * (q - 1)), (0, 1), (1, 0), (2, 1 + q), (p * p - 1, q * q - 1)):
        sp, sq = (0 if xp % p == 1 else 1), (0 if xq % q == 1 else 2)
        want = 0
        if not sp | sq:
            mp, mq = (xp - 1) // p * plan.hp % p, (xq - 1) // q * plan.hq % q
            want = mp + p * ((mq - mp) * plan.pinv % q)
        assert plan.recombine(xp, xq) == (want, sp | sq)
        count += 1
    return count


if __name__ == "__main__":
    for pb, qb in ((64, 67), (67, 64), (66, 66), (30, 101), (101, 30), (512, 515), (515, 512), (1025, 1026), (700, 261), (5, 9)):
        p_, q_ = key_of_bits(pb, qb)
        print(f"primes of {pb} and {qb} bits: {check(p_, q_)} values agree (rows as wide as N^2), "
              f"{check(p_, q_, extra_words=3)} with rows 3 words wider; encryption {enc_check(p_, q_)} and "
              f"{enc_check(p_, q_, extra_words=3)}")
