#!/usr/bin/env python3
"""Model of the dealt threshold key with verifiable partial decryptions (protocols/distributed_keygen_amd/threshold.py)
in Python ints and hashlib — developer tool and the oracle of tests/test_threshold_host.py and tests/test_gpu_proofs.py.

The scheme is Damgård–Jurik 2001 §4.1 (Shoup 2000 for the proof) with s = 1.  p = 2p' + 1 and q = 2q' + 1 are safe
primes, N = pq, m = p'q'; `parties` = n players, `threshold` = t is the polynomial's degree: t + 1 partials decrypt.

    deal      d = m (m^-1 mod N)                      d = 0 mod m,  d = 1 mod N
              f(X) = d + a_1 X + .. + a_t X^t  mod N m,   a_j uniform in [0, N m)
              s_i = f(i),  Delta = n!,  x_i = Delta s_i   (the exponent party i holds)
              v = u^2 mod N^2 for a random unit u,  w_i = v^(x_i) mod N^2   (verification keys)
              theta^-1 = (4 Delta^2)^-1 mod N
    partial   c_i = c^(2 x_i) mod N^2
    proof     that log_chat(c_i^2) = log_v(w_i), chat = c^4:
              X = bits(N m Delta), E = 128, K = 128;  rho uniform in [0, 2^(X + E + K))
              a = chat^rho,  b = v^rho
              e = first 16 bytes of SHA-256(ctx | BE(chat) | BE(c_i^2) | BE(a) | BE(b)) as a big-endian integer
              z = rho + e x_i over the integers;  the proof is (a, b, z)
    verify    a, b, c_i < N^2;  z < 2^(X + E + K + 1);  chat^z = a (c_i^2)^e;  v^z = b w_i^e  (e recomputed)
    combine   any S of t + 1 indices:  lambda_i = Delta prod_{j in S, j != i} j / (j - i)   (an integer, signed)
              c' = prod c_i^(2 lambda_i) mod N^2;   M = L(c') theta^-1 mod N,  L(x) = (x - 1) / N

BE(x) is x as a big-endian integer of 4 * limbs(N^2) bytes: the limb row of x with its words in reverse order.

ctx, 32 bytes, binds a proof to the key and the party:

    ctx = SHA-256(LP(TAG) | LP(N) | LP(v) | LP(w_i) | LP(i) | LP(n) | LP(t))
    LP(bytes) = 4-byte big-endian length | bytes;  an integer is its minimal big-endian bytes (one zero byte for 0)

The piece split.  The device multi-exponentiation and the fixed-base tables take exponents of at most 2 bits(N) + 64
bits; rho and z have up to X + 257.  Rows of rho and z are `pieces` pieces of `kw` words each (row width pieces * kw):

    kw_max = (2 bits(N) + 64) div 32,  wz = ceil((X + 257) / 32),  pieces = ceil(wz / kw_max),  kw = ceil(wz / pieces)
    chat^rho = prod_j B_j^(rho_j),   B_j = chat^(2^(32 kw j)),   rho = sum_j rho_j 2^(32 kw j),  rho_j < 2^(32 kw)

and likewise for v with the bases V_j = v^(2^(32 kw j)).  At every real key length pieces = 2.
"""
from __future__ import annotations

import hashlib
import math
from typing import Dict, List, Sequence, Tuple

E_BITS = 128                     # challenge width
K_BITS = 128                     # statistical hiding margin
MAX_PIECES = 8                   # pieces a row of rho or z may have (deal refuses a key that needs more)
TAG = b"mxpaillier/threshold-dleq/v1"


def limbs_for(value: int) -> int:
    return max(1, (int(value).bit_length() + 31) // 32)


def be_row(value: int, limbs: int) -> bytes:
    """BE(value): 4 * limbs bytes, big-endian."""
    return int(value).to_bytes(4 * limbs, "big")


def _lp(data: bytes) -> bytes:
    return len(data).to_bytes(4, "big") + data


def _int_bytes(x: int) -> bytes:
    return int(x).to_bytes(max(1, (int(x).bit_length() + 7) // 8), "big")


def context(n: int, v: int, w_i: int, index: int, parties: int, threshold: int) -> bytes:
    """ctx of party `index` under the key (N, v, w_i, n, t)."""
    msg = _lp(TAG) + b"".join(_lp(_int_bytes(x)) for x in (n, v, w_i, index, parties, threshold))
    return hashlib.sha256(msg).digest()


def split_shape(n_bits: int, z_bits: int) -> Tuple[int, int]:
    """(pieces, kw) of rows that hold z_bits bits under a modulus of n_bits bits."""
    kw_max = (2 * n_bits + 64) // 32
    wz = -(-z_bits // 32)
    pieces = -(-wz // kw_max)
    return pieces, -(-wz // pieces)


def pieces_of(value: int, pieces: int, kw: int) -> List[int]:
    """value = sum_j out[j] 2^(32 kw j) with out[j] < 2^(32 kw); ValueError if it does not fit."""
    if value < 0 or value >> (32 * kw * pieces):
        raise ValueError("the value does not fit the row")
    mask = (1 << (32 * kw)) - 1
    return [(value >> (32 * kw * j)) & mask for j in range(pieces)]


def row_words(value: int, words: int) -> List[int]:
    """The little-endian 32-bit words of a row."""
    return [(value >> (32 * k)) & 0xFFFFFFFF for k in range(words)]


class PublicKey:
    """What everybody holds: N, the players, v and the verification keys, and the sizes derived from them."""

    def __init__(self, n: int, parties: int, threshold: int, v: int, vks: Sequence[int], x_bits: int) -> None:
        self.n, self.parties, self.threshold, self.v, self.vks, self.x_bits = n, parties, threshold, v, list(vks), x_bits
        self.n_square = n * n
        self.limbs2 = limbs_for(self.n_square)
        self.delta = math.factorial(parties)
        self.theta_inv = pow(4 * self.delta * self.delta, -1, n)
        self.rho_bits = x_bits + E_BITS + K_BITS
        self.z_bits = self.rho_bits + 1
        self.pieces, self.kw = split_shape(n.bit_length(), self.z_bits)
        self.z_words = self.pieces * self.kw

    def vk(self, index: int) -> int:
        if not 1 <= index <= self.parties:
            raise ValueError(f"no party {index}")
        return self.vks[index - 1]

    def ctx(self, index: int) -> bytes:
        return context(self.n, self.v, self.vk(index), index, self.parties, self.threshold)


class Share:
    def __init__(self, index: int, x: int) -> None:
        self.index, self.x = index, x


def deal(p: int, q: int, parties: int, threshold: int, rand) -> Tuple[PublicKey, List[Share]]:
    """The dealer.  `rand` has randrange (random.Random for tests, secrets.SystemRandom otherwise).  Draw order: the t
    coefficients a_1 .. a_t, then candidates for u until one is a unit."""
    if parties < 2 or not 0 < threshold < parties:
        raise ValueError("1 <= threshold < parties and parties >= 2 expected")
    n = p * q
    m = ((p - 1) // 2) * ((q - 1) // 2)
    nm = n * m
    d = m * pow(m, -1, n)
    coeffs = [d] + [rand.randrange(nm) for _ in range(threshold)]
    delta = math.factorial(parties)
    xs = [delta * (sum(a * i ** k for k, a in enumerate(coeffs)) % nm) for i in range(1, parties + 1)]
    n2 = n * n
    while True:
        u = rand.randrange(2, n2)
        if math.gcd(u, n) == 1:
            break
    v = u * u % n2
    pub = PublicKey(n, parties, threshold, v, [pow(v, x, n2) for x in xs], (nm * delta).bit_length())
    return pub, [Share(i + 1, x) for i, x in enumerate(xs)]


def partial(pub: PublicKey, share: Share, c: int) -> int:
    return pow(c, 2 * share.x, pub.n_square)


def piece_bases(base: int, pieces: int, kw: int, n2: int) -> List[int]:
    """B_j = base^(2^(32 kw j)) mod n2, j < pieces."""
    out = [base % n2]
    for _ in range(pieces - 1):
        out.append(pow(out[-1], 1 << (32 * kw), n2))
    return out


def pow_by_pieces(bases: Sequence[int], exponent: int, kw: int, n2: int) -> int:
    """prod_j bases[j]^(exponent_j): the device's route to base^exponent."""
    acc = 1
    for b, ej in zip(bases, pieces_of(exponent, len(bases), kw)):
        acc = acc * pow(b, ej, n2) % n2
    return acc


def challenge(ctx: bytes, chat: int, ci2: int, a: int, b: int, limbs2: int) -> int:
    h = hashlib.sha256(ctx + be_row(chat, limbs2) + be_row(ci2, limbs2) + be_row(a, limbs2) + be_row(b, limbs2)).digest()
    return int.from_bytes(h[:16], "big")


def prove(pub: PublicKey, share: Share, c: int, rho: int) -> Tuple[int, int, int, int]:
    """(c_i, a, b, z) for the ciphertext c and the draw rho < 2^rho_bits."""
    if rho < 0 or rho >> pub.rho_bits:
        raise ValueError("rho out of range")
    n2 = pub.n_square
    ci = partial(pub, share, c)
    chat = pow(c, 4, n2)
    a = pow_by_pieces(piece_bases(chat, pub.pieces, pub.kw, n2), rho, pub.kw, n2)
    b = pow_by_pieces(piece_bases(pub.v, pub.pieces, pub.kw, n2), rho, pub.kw, n2)
    assert a == pow(chat, rho, n2) and b == pow(pub.v, rho, n2)
    e = challenge(pub.ctx(share.index), chat, ci * ci % n2, a, b, pub.limbs2)
    return ci, a, b, rho + e * share.x


def verify(pub: PublicKey, index: int, c: int, ci: int, a: int, b: int, z: int) -> bool:
    n2 = pub.n_square
    if not (0 <= a < n2 and 0 <= b < n2 and 0 <= ci < n2 and 0 <= z < 1 << pub.z_bits):
        return False
    chat, ci2 = pow(c, 4, n2), ci * ci % n2
    e = challenge(pub.ctx(index), chat, ci2, a, b, pub.limbs2)
    if pow_by_pieces(piece_bases(chat, pub.pieces, pub.kw, n2), z, pub.kw, n2) != a * pow(ci2, e, n2) % n2:
        return False
    return pow_by_pieces(piece_bases(pub.v, pub.pieces, pub.kw, n2), z, pub.kw, n2) == b * pow(pub.vk(index), e, n2) % n2


def lagrange(delta: int, subset: Sequence[int]) -> Dict[int, int]:
    """lambda_i = delta prod_{j in S, j != i} j / (j - i): integers, some negative."""
    out = {}
    for i in subset:
        num, den = delta, 1
        for j in subset:
            if j != i:
                num *= j
                den *= j - i
        assert num % den == 0
        out[i] = num // den
    return out


def combine(pub: PublicKey, partials: Dict[int, int]) -> int:
    """The plaintext from t + 1 partials {index: c_i}; ValueError if the combination is not 1 modulo N."""
    if len(partials) != pub.threshold + 1:
        raise KeyError("threshold + 1 partials expected")
    n, n2 = pub.n, pub.n_square
    acc = 1
    for i, lam in lagrange(pub.delta, sorted(partials)).items():
        acc = acc * pow(partials[i], 2 * lam, n2) % n2
    if acc % n != 1:
        raise ValueError("Combination of partial decryptions is not 1 modulo N")
    return (acc - 1) // n * pub.theta_inv % n


def encrypt(n: int, message: int, r: int) -> int:
    n2 = n * n
    return (1 + message * n) * pow(r, n, n2) % n2


def sha256_rows(prefix: bytes, row_sets: Sequence[Tuple[Sequence[int], int]]) -> List[int]:
    """digest[r] = SHA-256(prefix | BE(rows_0[r]) | ..) as an integer (big-endian): the contract of mx_sha256_rows.
    row_sets: (values, limbs) pairs; no set at all gives ONE digest of the prefix alone per requested row — the caller
    says how many."""
    count = len(row_sets[0][0]) if row_sets else 1
    return [int.from_bytes(hashlib.sha256(prefix + b"".join(be_row(vals[r], limbs) for vals, limbs in row_sets)).digest(), "big")
            for r in range(count)]


def dleq_response(rho: Sequence[int], e: Sequence[int], x: int, wz: int) -> Tuple[List[int], List[int]]:
    """(z rows truncated to wz words, status): the contract of mx_dleq_response."""
    full = [r + k * x for r, k in zip(rho, e)]
    return [f & ((1 << (32 * wz)) - 1) for f in full], [1 if f >> (32 * wz) else 0 for f in full]


# ---- the safe primes of tests/golden/threshold_keys.json ---------------------------------------------------------------
_SMALL = [l for l in range(3, 20000, 2) if all(l % d for d in range(3, int(l ** 0.5) + 1, 2))]


def _is_prime(x: int, rand, rounds: int = 24) -> bool:
    if x < 2 or x % 2 == 0:
        return x == 2
    d, s = x - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for k in range(rounds):
        a = 2 if k == 0 else rand.randrange(2, x - 1)
        y = pow(a, d, x)
        if y in (1, x - 1):
            continue
        for _ in range(s - 1):
            y = y * y % x
            if y == x - 1:
                break
        else:
            return False
    return True


def find_safe_prime(bits: int, rand) -> int:
    """A safe prime p = 2h + 1 of exactly `bits` bits with its two top bits set (the product of two has 2 * bits bits):
    random starts, a joint sieve of h and 2h + 1 over a window of consecutive odd h, then Miller-Rabin."""
    span = 1 << 16
    while True:
        h0 = rand.getrandbits(bits - 1) | (3 << (bits - 3)) | 1
        alive = bytearray([1]) * span                     # h = h0 + 2 k
        for l in _SMALL:
            if l >= h0:
                break
            inv2 = (l + 1) // 2
            for target in (0, (l - 1) // 2):              # l | h,  l | 2h + 1
                k = (target - h0) * inv2 % l
                alive[k::l] = bytes(len(range(k, span, l)))
        for k in range(span):
            if alive[k]:
                h = h0 + 2 * k
                if (2 * h + 1).bit_length() != bits:
                    break
                if pow(2, h - 1, h) == 1 and pow(2, h, 2 * h + 1) in (1, 2 * h) and _is_prime(h, rand) and _is_prime(2 * h + 1, rand):
                    return 2 * h + 1


def golden_keys(seed: int, key_lengths: Sequence[int]) -> dict:
    import random

    out = {"seed": seed, "generator": "tools/proof_model.py: golden_keys(seed, key_lengths) over random.Random(seed)", "keys": {}}
    rand = random.Random(seed)
    for kl in key_lengths:
        p = find_safe_prime(kl // 2, rand)
        q = p
        while q == p:
            q = find_safe_prime(kl // 2, rand)
        assert (p * q).bit_length() == kl
        out["keys"][str(kl)] = {"p": format(p, "x"), "q": format(q, "x")}
    return out


if __name__ == "__main__":
    import json
    import sys

    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 20261020
    print(json.dumps(golden_keys(seed, (128, 1024, 2048)), indent=1))
