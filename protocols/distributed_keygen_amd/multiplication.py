"""Multiplication proofs for Paillier ciphertexts: whoever knows the a inside c_a = (1 + N)^a r_a^N proves that
d = c_b^a gamma^N holds a b for the b inside ANOTHER party's ciphertext c_b — without learning b and without showing a.
The proof of correct multiplication of Damgard-Jurik 2001 §4 (Cramer-Damgard-Nielsen 2001), on the GPU engine.  It is
what makes "multiply this ciphertext by my private scalar" accountable, the step ``secure_product`` builds the product
of two ENCRYPTED values from, and the building block of MtA-style protocols.

    statement   c_a = (1 + N)^a r_a^N,   d = c_b^a gamma^N   (mod N^2);   the prover knows a < N, r_a, gamma
    prove       x < N,  u, v;   A = (1 + x N) u^N,   B = c_b^x v^N
                e = SHA-256(ctx | c_a | c_b | d | A | B)[:16]
                (w, t) = divmod(x + e a, N);   z = u r_a^e mod N,   y = v (c_b mod N)^t gamma^e mod N
    verify      0 < c_a, c_b, d, A, B < N^2;   w < N;   0 < z, y < N
                (1 + w N) z^N = A c_a^e   and   c_b^w y^N = B d^e   (mod N^2)

tools/mul_model.py is the model that pins every byte (ctx, the hashed message, the row widths, the draw order);
DESIGN.md §4.28 has the design and the measurements.  The response (w, t) — an exponent that lives modulo N, with the
quotient that moves into y — runs on the device with control flow and addresses that do not depend on a, x or e
(``Engine.response_mod_rows_t``, csrc/mx_response_mod.hpp); everything else is the engine's N^2 modexp,
multi-exponentiation and hash.

What this is and is not — read before use:

  * WHAT IS PROVEN is that d encrypts a b mod N for the a of c_a and the b of c_b, and knowledge of a, r_a and gamma.
    NOTHING is proven about c_b: whether it is a valid ciphertext, or what b is, is its sender's business
    (``range_proof``, ``membership``).  Nothing is proven about the SIZE of a either — a is any residue modulo N.
  * The protocol is the EXACT one: w = x + e a mod N is uniform whatever a is, so a is hidden perfectly for honest
    draws, and the verifier's exponents are no longer than N.  (The statistical variant — x 256 bits longer, x + e a
    sent unreduced — needs no quotient but hides a only statistically and lengthens every exponent by 257 bits.)
  * Soundness is special soundness of the Sigma-protocol in the random-oracle model (SHA-256, a 128-bit challenge), and
    needs EVERY PRIME FACTOR OF N ABOVE 2^128: the caller guarantees that N is a proper key.  ``bits(N) < 260`` is
    refused outright, before any engine call.  It also needs z and y to be units modulo N, and THE VERIFIER REFUSES
    ZERO: A = z = 0 satisfies the first equation and B = y = 0 the second for any statement, so without that check
    anybody could prove that any d holds a b.  Zero is the only non-unit that needs a check: with every prime factor
    above 2^128 any other would factor N.  c_a, c_b and d are refused at zero alike.
  * Hiding rests on x, u and v NEVER REPEATING: they come from a ``device_rng.DeviceRng`` (read its docstring) and its
    nonce discipline.  d is as fresh as gamma is.
  * ``label`` binds a proof to a sender and a session: a proof does not verify under another label or another N.  A
    verdict says NOTHING ABOUT FRESHNESS: whoever saw the statement and its proof can send them again.
  * The verifier takes no inverse of anything the prover sent, and a malformed row (a value out of range, too long,
    negative) is a False verdict for that row, never an exception.
  * r_a and gamma are NOT checked to be units modulo N, as ``encrypt_fresh_batch`` does not check its r.
  * Side channels.  The response kernel's control flow and addresses depend on the row widths only.  The table gathers of
    c_b^a and c_b^x are indexed by the digits of a and x, those of r_a^e and gamma^e by public digits — the same class
    of side channel as every windowed modexp of this engine.
"""

from __future__ import annotations

import hashlib
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from . import limbs as _limbs, proof_flows as _flows
from .range_proof import E_BITS, _engine_of, _host, _int_bytes, _lp, _rows_of

MIN_BITS = 260                   # every prime factor of N must exceed 2^E_BITS; shorter moduli cannot even claim it
TAG = b"mxpaillier/multiplication/v1"


def _check_modulus(n: int) -> None:
    if n < 3 or n % 2 == 0:
        raise ValueError("N must be odd")
    if n.bit_length() < MIN_BITS:
        raise ValueError(f"a modulus of at least {MIN_BITS} bits expected (every prime factor above 2^{E_BITS})")


def shape(n: int) -> dict:
    """Bit lengths and row widths of a proof (tools/mul_model.py: shape)."""
    return _flows.mul_shape(n)


def context(n: int, label: bytes) -> bytes:
    """The 32 bytes that bind a proof to N and the caller's label."""
    return hashlib.sha256(_lp(TAG) + _lp(_int_bytes(n)) + _lp(bytes(label))).digest()


class MultiplicationProofs:
    """The proofs of a batch of statements: the rows of A and B (``[count, limbs(N^2)]``) and of w, z and y
    (``[count, limbs(N)]``) — device tensors where they were made on the device, uint32 numpy rows where they arrived as
    ints.  ``unfit[r]`` marks a row whose integers did not fit the rows (its verdict is False)."""

    FIELDS = ("a", "b", "w", "z", "y")

    def __init__(self, a, b, w, z, y, unfit: Optional[List[bool]] = None) -> None:
        self.a, self.b, self.w, self.z, self.y = a, b, w, z, y
        self.unfit = unfit

    def __len__(self) -> int:
        return int(self.a.shape[0])

    def rows(self) -> Tuple[Any, ...]:
        return tuple(getattr(self, f) for f in self.FIELDS)

    def to_ints(self) -> Tuple[List[int], ...]:
        """(A, B, w, z, y), a list of ints each — what travels to the verifier."""
        return tuple(_limbs.unpack(np.ascontiguousarray(_host(t))) if t.shape[0] else [] for t in self.rows())

    @classmethod
    def from_ints(cls, a: Sequence[int], b: Sequence[int], w: Sequence[int], z: Sequence[int], y: Sequence[int], n: int) -> "MultiplicationProofs":
        """The proofs received as ints, as rows under N.  A value that is negative, no integer or does not fit its row
        becomes a harmless row and a False verdict."""
        sh = shape(n)
        cols = (a, b, w, z, y)
        count = len(a)
        if any(len(c) != count for c in cols):
            raise ValueError("one A, B, w, z and y per statement expected")
        unfit = [False] * count
        packed = []
        for col, words in zip(cols, (sh["limbs2"], sh["limbs2"], sh["limbs_n"], sh["limbs_n"], sh["limbs_n"])):
            vals = []
            for r, v in enumerate(col):
                try:
                    vals.append(int(v))
                except (TypeError, ValueError):
                    unfit[r] = True
                    vals.append(0)
            rows, fits = _rows_of(vals, words)
            unfit = [u or not f for u, f in zip(unfit, fits)]
            packed.append(rows)
        return cls(*packed, unfit)


def _empty(sh: dict) -> MultiplicationProofs:
    return MultiplicationProofs(*(np.zeros((0, sh[w]), dtype=np.uint32) for w in ("limbs2", "limbs2", "limbs_n", "limbs_n", "limbs_n")))


def _check_statement(n: int, label: bytes) -> dict:
    if not isinstance(label, (bytes, bytearray)):
        raise ValueError("the label must be bytes")
    _check_modulus(n)
    return shape(n)


def _default_rng(rng: Any) -> Any:
    if rng is not None:
        return rng
    from .device_rng import DeviceRng

    return DeviceRng()


def prove_batch(n: int, a: Sequence[int], randomness: Sequence[int], gamma: Sequence[int], c_b: Sequence[int], label: bytes,
                rng: Any = None, c_a: Optional[Sequence[int]] = None, engine: Any = None, draws: Any = None
                ) -> Tuple[List[int], MultiplicationProofs]:
    """``(d, proofs)``: d_r = c_b[r]^(a_r) gamma_r^n mod n^2 and the proofs that d_r holds a_r times what c_b[r] holds,
    for the a_r inside c_a[r] = (1 + n)^(a_r) (randomness_r)^n (``c_a``: the ciphertexts if the caller has them, else they
    are recomputed).  ``rng``: a ``DeviceRng`` (default: a fresh one); ``draws``: the two row sets, for tests.
    ValueError — before any engine call — for a modulus below 260 bits, lists of unequal lengths, an a outside [0, n)
    or a c_b outside (0, n^2)."""
    n = int(n)
    sh = _check_statement(n, label)
    a, rands, gam, cb = ([int(v) for v in col] for col in (a, randomness, gamma, c_b))
    count = len(a)
    if any(len(col) != count for col in (rands, gam, cb)) or (c_a is not None and len(c_a) != count):
        raise ValueError("one randomness, one gamma, one c_b (and one c_a) per a expected")
    if any(not 0 <= v < n for v in a):
        raise ValueError("every a must lie in [0, N)")
    if any(not 0 < v < n * n for v in cb):
        raise ValueError("every c_b must lie in (0, N^2)")
    if not count:
        return [], _empty(sh)
    eng = _engine_of(engine)
    if c_a is None:
        c_a = eng.encrypt_batch(a, rands, n)
    ln, limbs2 = sh["limbs_n"], sh["limbs2"]

    def up(vals, words, mod):
        return eng.to_device(_limbs.pack_reduced(list(vals), words, mod).reshape(count, words))

    source = dict(draws=draws) if draws is not None else dict(rng=_default_rng(rng))
    out = eng.mul_prove_t(up(c_a, limbs2, n * n), up(cb, limbs2, n * n), up(a, ln, n), up(rands, ln, n), up(gam, ln, n), n,
                          context(n, label), **source)
    return _limbs.unpack(np.ascontiguousarray(_host(out[0]))), MultiplicationProofs(*out[1:])


def multiply_with_proof(n: int, a: Sequence[int], c_b: Sequence[int], label: bytes, rng: Any = None, engine: Any = None
                        ) -> Tuple[List[int], List[int], MultiplicationProofs]:
    """``(c_a, d, proofs)``: fresh encryptions c_a of the private scalars ``a`` (``Engine.encrypt_fresh_batch``), the
    products d_r = c_b[r]^(a_r) gamma_r^n with gamma drawn on the device as the r of an encryption is, and the proofs
    that d_r holds a_r times what c_b[r] holds.  The randomness is kept for the proof only and not returned."""
    n = int(n)
    sh = _check_statement(n, label)
    a = [int(v) for v in a]
    if len(c_b) != len(a):
        raise ValueError("one c_b per a expected")
    if any(not 0 <= v < n for v in a):
        raise ValueError("every a must lie in [0, N)")
    if any(not 0 < int(v) < n * n for v in c_b):
        raise ValueError("every c_b must lie in (0, N^2)")
    if not a:
        return [], [], _empty(sh)
    eng = _engine_of(engine)
    rng = _default_rng(rng)
    c_a, rands = eng.encrypt_fresh_batch(a, n, rng, return_randomness=True)
    gamma = _limbs.unpack(np.ascontiguousarray(_host(rng.rows_t(eng, len(a), sh["draw_bits"], sh["limbs2"]))))
    d, proofs = prove_batch(n, a, rands, gamma, c_b, label, rng=rng, c_a=c_a, engine=eng)
    return c_a, d, proofs


def verify_batch(n: int, c_a: Sequence[int], c_b: Sequence[int], d: Sequence[int], proofs: MultiplicationProofs, label: bytes,
                 engine: Any = None) -> List[bool]:
    """[is row r a valid proof that d[r] holds the product of what c_a[r] and c_b[r] hold] — never raises for a bad row:
    a value that is negative, zero (any but w), out of range or too long is a False.  ValueError — before any engine
    call — for a modulus below 260 bits or a number of proofs other than the number of statements."""
    n = int(n)
    sh = _check_statement(n, label)
    count = len(c_a)
    if not isinstance(proofs, MultiplicationProofs) or len(c_b) != count or len(d) != count or len(proofs) != count:
        raise ValueError("one c_b, one d and one proof per c_a expected")
    if count == 0:
        return []
    eng = _engine_of(engine)
    cols = [_rows_of(col, sh["limbs2"]) for col in (c_a, c_b, d)]
    if proofs.unfit is None and not isinstance(proofs.a, np.ndarray):
        rows = proofs.rows()
    else:
        rows = tuple(eng.to_device(np.asarray(t)) for t in proofs.rows())
    unfit = proofs.unfit or [False] * count
    verdict = eng.mul_verify_t(*(eng.to_device(rows_) for rows_, _ in cols), *rows, n, context(n, label))
    got = [bool(x) for x in (verdict if isinstance(verdict, np.ndarray) else verdict.cpu().numpy())]
    return [g and not u and all(fit[r] for _, fit in cols) for r, (g, u) in enumerate(zip(got, unfit))]
