#!/usr/bin/env python3
"""Model of the multiplication proofs for Paillier ciphertexts (protocols/distributed_keygen_amd/multiplication.py) in
Python ints and hashlib — developer tool and the oracle of tests/test_multiplication_host.py and
tests/test_gpu_multiplication.py.

The proof of correct multiplication of Damgard-Jurik 2001 §4 (Cramer-Damgard-Nielsen 2001): whoever knows a shows that d
holds a b for the a inside c_a and the b inside c_b, without learning b and without showing a.

    public      odd N; ciphertexts c_a, c_b, d below N^2; a label.  E = 128 (challenge width).
    statement   c_a = (1 + N)^a r_a^N,   d = c_b^a gamma^N   (mod N^2);   the prover knows a < N, r_a, gamma
    prove       x < N,  u, v
                A = (1 + x N) u^N,   B = c_b^x v^N   (mod N^2)
                e = first 16 bytes of SHA-256(ctx | BE(c_a) | BE(c_b) | BE(d) | BE(A) | BE(B)) as a big-endian integer
                (w, t) = divmod(x + e a, N)
                z = u r_a^e mod N,   y = v (c_b mod N)^t gamma^e mod N
                the proof is (A, B, w, z, y)
    verify      0 < c_a, c_b, d, A, B < N^2;   w < N;   0 < z, y < N
                (1 + w N) z^N = A c_a^e   (mod N^2)
                c_b^w y^N = B d^e         (mod N^2)

Why t: x + e a = w + t N, and c_b^(tN) = ((c_b mod N)^t)^N (mod N^2) — an N-th power only sees its base modulo N —, so
the quotient moves from the exponent of c_b into the N-th root y.  The exponent lives modulo N EXACTLY: w is uniform
whatever a is, no slack.

ZERO IS REFUSED: A = z = 0 satisfies the first equation and B = y = 0 the second for ANY statement.  With every prime
factor of N above 2^128 any other non-unit would factor N, so zero is the only one that needs a check.

BE(v) is v as a big-endian integer of 4 limbs(N^2) bytes.  ctx, 32 bytes, binds a proof to the key and the label:

    ctx = SHA-256(LP(TAG) | LP(N) | LP(label))
    LP(bytes) = 4-byte big-endian length | bytes;  an integer is its minimal big-endian bytes (one zero byte for 0)

Draw order on a device generator (device_rng.DeviceRng: one call number per draw): call c the x draws — count rows of
bits(N) + 64 bits at the width limbs(N^2), x = draw mod N —, call c + 1 the u and v draws — 2 count rows of bits(N) + 64
bits at the width limbs(N^2), the u of all rows first, then the v; used unreduced as bases of an N-th power and modulo N
in z and y, as ``encrypt_fresh_batch`` draws its r.

``response_mod`` is the one step no other entry point covers (csrc/mx_response_mod.hpp): (w, t) = divmod(rho + e x, M)
with the status "t does not fit ew words".  ``response_mod_steps`` is the kernel step for step — the words of s in one
row, schoolbook division from the top, a digit estimate from the top 64 bits (two words) and a reciprocal, three passes
"window -= f M; is it >= M" — at ANY word width, so the estimate's error bound is checked exhaustively at 4-bit words.
"""
from __future__ import annotations

import hashlib
from typing import List, Optional, Sequence, Tuple

E_BITS = 128                     # challenge width
TAG = b"mxpaillier/multiplication/v1"
MAX_ESTIMATE_ERROR = 2           # what the kernel's two masked corrections cover


def limbs_for(value: int) -> int:
    return max(1, (int(value).bit_length() + 31) // 32)


def be_row(value: int, limbs: int) -> bytes:
    return int(value).to_bytes(4 * limbs, "big")


def _lp(data: bytes) -> bytes:
    return len(data).to_bytes(4, "big") + data


def _int_bytes(x: int) -> bytes:
    return int(x).to_bytes(max(1, (int(x).bit_length() + 7) // 8), "big")


def context(n: int, label: bytes) -> bytes:
    return hashlib.sha256(_lp(TAG) + _lp(_int_bytes(n)) + _lp(bytes(label))).digest()


def shape(n: int) -> dict:
    """Bit lengths and row widths of everything a proof holds."""
    return dict(draw_bits=n.bit_length() + 64, e_bits=E_BITS, e_words=E_BITS // 32, limbs_n=limbs_for(n), limbs2=limbs_for(n * n))


def challenge(ctx: bytes, ca: int, cb: int, d: int, a_: int, b_: int, limbs2: int) -> int:
    h = hashlib.sha256(ctx + b"".join(be_row(v, limbs2) for v in (ca, cb, d, a_, b_))).digest()
    return int.from_bytes(h[:16], "big")


def encrypt(n: int, message: int, r: int) -> int:
    n2 = n * n
    return (1 + message % n * n) % n2 * pow(r, n, n2) % n2


def product(n: int, cb: int, a: int, gamma: int) -> int:
    """d = c_b^a gamma^N mod N^2: what holds a b."""
    n2 = n * n
    return pow(cb, a, n2) * pow(gamma, n, n2) % n2


def prove(n: int, label: bytes, ca: int, cb: int, a: int, ra: int, gamma: int, x_draw: int, u: int, v: int,
          d: Optional[int] = None) -> Tuple[int, int, int, int, int]:
    """(A, B, w, z, y) for c_a = encrypt(n, a, ra), d = product(n, cb, a, gamma) and the three draws."""
    sh = shape(n)
    if not 0 <= a < n:
        raise ValueError("a in [0, N) expected")
    if any(t < 0 or t >> sh["draw_bits"] for t in (x_draw, u, v)):
        raise ValueError("a draw is out of range")
    n2 = n * n
    if d is None:
        d = product(n, cb, a, gamma)
    x = x_draw % n
    a_ = (1 + x * n) % n2 * pow(u, n, n2) % n2
    b_ = pow(cb, x, n2) * pow(v, n, n2) % n2
    e = challenge(context(n, label), ca, cb, d, a_, b_, sh["limbs2"])
    w, t = response_mod(x, e, a, n)
    z = u % n * pow(ra % n, e, n) % n
    y = v % n * pow(cb % n, t, n) % n * pow(gamma % n, e, n) % n
    return a_, b_, w, z, y


def in_range(n: int, ca: int, cb: int, d: int, proof: Sequence[int]) -> bool:
    """The range checks of verify, which come before any arithmetic on the row."""
    if len(proof) != 5:
        return False
    a_, b_, w, z, y = proof
    n2 = n * n
    return all(0 < v < n2 for v in (ca, cb, d, a_, b_)) and 0 <= w < n and 0 < z < n and 0 < y < n


def verify(n: int, label: bytes, ca: int, cb: int, d: int, proof: Sequence[int]) -> bool:
    if n < 3 or n % 2 == 0:
        raise ValueError("N must be odd")
    if not in_range(n, ca, cb, d, proof):
        return False
    a_, b_, w, z, y = proof
    n2 = n * n
    e = challenge(context(n, label), ca, cb, d, a_, b_, shape(n)["limbs2"])
    if (1 + w * n) % n2 * pow(z, n, n2) % n2 != a_ * pow(ca, e, n2) % n2:
        return False
    return pow(cb, w, n2) * pow(y, n, n2) % n2 == b_ * pow(d, e, n2) % n2


# ---- the response modulo M of csrc/mx_response_mod.hpp ---------------------------------------------------------------------
def response_mod(rho: int, e: int, x: int, mod: int) -> Tuple[int, int]:
    """(w, t) = divmod(rho + e x, mod): what the kernel computes."""
    t, w = divmod(rho + e * x, mod)
    return w, t


def response_mod_constants(mod: int, wn: int, wbits: int = 32) -> Tuple[int, int]:
    """(reciprocal, shift) the host derives from M of wn words of wbits bits, top word non-zero: shift = the leading
    zeros of the top word, Md = the top two words of M << shift (a zero word below a one-word M),
    reciprocal = floor(b^3 / (Md + 1)) with b = 2^wbits — in [b, 2 b)."""
    b = 1 << wbits
    top = mod >> (wbits * (wn - 1))
    if mod < 1 or not 0 < top < b:
        raise ValueError("a modulus of wn words whose top word is non-zero expected")
    shift = wbits - top.bit_length()
    md = (mod << shift) >> (wbits * (wn - 2)) if wn >= 2 else (mod << shift) << wbits
    assert b * b // 2 <= md < b * b
    recip = b ** 3 // (md + 1)
    assert b <= recip < 2 * b
    return recip, shift


def response_mod_form(rho: int, e: int, x: int, wn: int, ew: int, wbits: int = 32) -> List[int]:
    """Pass 1 of response_mod_kernel: the wn + ew words of s = rho + e x, by columns."""
    b = 1 << wbits
    mask = b - 1
    if not (0 <= rho < b ** wn and 0 <= x < b ** wn and 0 <= e < b ** ew):
        raise ValueError("operands beyond their rows")
    s = [0] * (wn + ew)
    acc = 0
    for k in range(wn + ew):
        if k < wn:
            acc += (rho >> (wbits * k)) & mask
        for j in range(max(0, k - (wn - 1)), min(k, ew - 1) + 1):
            acc += ((e >> (wbits * j)) & mask) * ((x >> (wbits * (k - j))) & mask)
        s[k] = acc & mask
        acc >>= wbits
    assert acc == 0                                     # s <= b^ew (b^wn - 1): no word above them
    return s


def response_mod_estimate(hi: int, u1: int, u0: int, recip: int, shift: int, wbits: int = 32) -> int:
    """The digit's estimate from the window's top three words (hi the word ABOVE the wn words): the top two words of the
    window shifted, times the reciprocal, the high part.  q - 2 <= estimate <= q for a window below M b."""
    uh = (((hi << wbits) | u1) << shift) | ((u0 << shift) >> wbits)
    assert uh >> (2 * wbits) == 0
    return (uh * recip) >> (2 * wbits)


def response_mod_divide(s: List[int], mod: int, wn: int, ew: int, wbits: int = 32,
                        errors: Optional[List[int]] = None) -> Tuple[int, int, int]:
    """The division of response_mod_kernel on the wn + ew words `s` (changed in place): schoolbook from the top, digit
    i = ew .. 0, three passes "window -= f M; is it >= M" per digit, the digit stored where the window's dead top word
    was.  (w, t, status)."""
    b = 1 << wbits
    mask = b - 1
    recip, shift = response_mod_constants(mod, wn, wbits)
    m = [(mod >> (wbits * j)) & mask for j in range(wn)]

    def mulsub(i: int, f: int, hi: int) -> Tuple[int, int]:
        """window -= f M; (hi, 1 iff the result is >= M)"""
        carry = borrow = below = 0
        for j in range(wn):
            prod = f * m[j] + carry
            carry = prod >> wbits
            d = s[i + j] - (prod & mask) - borrow
            borrow = 1 if d < 0 else 0
            s[i + j] = d & mask
            c = s[i + j] - m[j] - below
            below = 1 if c < 0 else 0
        hi = hi - carry - borrow
        assert 0 <= hi <= 2
        return hi, int(hi >= below)

    top = 0
    for i in range(ew, -1, -1):
        hi = s[i + wn] if i < ew else 0
        q = response_mod_estimate(hi, s[i + wn - 1], s[i + wn - 2] if wn >= 2 else 0, recip, shift, wbits)
        if errors is not None:
            window = hi * b ** wn + sum(s[i + j] << (wbits * j) for j in range(wn))
            assert window < mod * b
            errors.append(window // mod - q)
        hi, ge = mulsub(i, q, hi)
        q += ge
        hi, ge = mulsub(i, ge, hi)
        q += ge
        hi, ge = mulsub(i, ge, hi)
        assert hi == 0 and ge == 0 and q < b             # the two corrections sufficed: what is left is below M
        if i < ew:
            s[i + wn] = q                                # where the digit goes: the word is dead
        else:
            top = q
    w = sum(s[j] << (wbits * j) for j in range(wn))
    t = sum(s[wn + i] << (wbits * i) for i in range(ew))
    return w, t, int(top != 0)


def response_mod_steps(rho: int, e: int, x: int, mod: int, wn: int, ew: int, wbits: int = 32,
                       errors: Optional[List[int]] = None) -> Tuple[int, int, int]:
    """(w, t, status) as response_mod_kernel computes them, step for step, on words of `wbits` bits: rho, x below
    b^wn, e below b^ew, M of wn words with a non-zero top word.  t is the low ew words of the quotient, status 1 iff
    there is more.  ``errors`` receives, per digit, how far the estimate fell short of the digit (0 .. 2)."""
    return response_mod_divide(response_mod_form(rho, e, x, wn, ew, wbits), mod, wn, ew, wbits, errors)


def device_draws(key: bytes, call: int, count: int, n: int) -> Tuple[List[int], List[int], List[int]]:
    """(x draws, u, v), `count` ints each, as DeviceRng(key, first_call=call) gives them to Engine.mul_prove_t."""
    import chacha_model

    sh = shape(n)
    xs = chacha_model.row_ints(key, call, count, sh["draw_bits"], sh["limbs2"])
    uv = chacha_model.row_ints(key, call + 1, 2 * count, sh["draw_bits"], sh["limbs2"])
    return xs, uv[:count], uv[count:]


if __name__ == "__main__":
    import random

    rnd = random.Random(1)
    p, q = 0xF5B0124F8C69215B, 0xE2FCE1351448C67B          # tests/golden/threshold_keys.json, key length 128
    n_ = p * q
    for _ in range(3):
        a_s, b_s = rnd.randrange(n_), rnd.randrange(n_)
        ra_, rb_, g_ = (rnd.randrange(1, n_) for _ in range(3))
        ca_, cb_ = encrypt(n_, a_s, ra_), encrypt(n_, b_s, rb_)
        d_ = product(n_, cb_, a_s, g_)
        pf = prove(n_, b"demo", ca_, cb_, a_s, ra_, g_, *(rnd.getrandbits(192) for _ in range(3)))
        print(verify(n_, b"demo", ca_, cb_, d_, pf), verify(n_, b"demo", ca_, cb_, d_ * (1 + n_) % (n_ * n_), pf))
    worst = []
    for mod_ in range(16, 256):
        for _ in range(200):
            response_mod_steps(rnd.randrange(256), rnd.randrange(16), rnd.randrange(256), mod_, 2, 1, 4, worst)
    print("largest estimate error at 4-bit words (sampled):", max(worst))
