"""Decryption with an ordinary Paillier private key — the primes p and q of N — on the GPU engine.

The decrypting party of gradient-boosted trees, vertical logistic regression or encrypted scoring usually holds a plain
key, not a threshold share.  Knowing p and q allows the CRT decryption of Paillier 1999, section 7:

    x_p = (c mod p^2)^(p-1) mod p^2      m_p = L_p(x_p) h_p mod p       L_p(x) = (x - 1) / p
    x_q = (c mod q^2)^(q-1) mod q^2      m_q = L_q(x_q) h_q mod q
    m   = m_p + p ((m_q - m_p) p^-1 mod q)
    h_p = L_p((N + 1)^(p-1) mod p^2)^-1 mod p,  h_q likewise

two modexps with half-length exponents over half-width moduli (``Engine.private_decrypt_t``: both moduli are squares,
so they run on the pair kernel of the partial decryption) instead of one full-width modexp with an exponent as long as N.
The plaintext rows have the format of ``Engine.combine_t``: ``slots.decode_t`` and ``packing.unpack`` take them as they
are.

The status.  A row's status is non-zero when c^(p-1) is not 1 modulo p (bit 0) or c^(q-1) not 1 modulo q (bit 1).  For a
prime p that happens exactly when p divides c: the status detects ciphertexts that share a factor with N (0, multiples of
p or q) and nothing else.  Every c coprime to N is a valid ciphertext of SOME plaintext, so a corrupted or foreign
ciphertext decrypts, without a status, to a wrong plaintext — as it does in every Paillier implementation.  With a
composite "prime" the status fires for most ciphertexts; primality itself is never tested here.

Side channels.  The exponents p - 1 and q - 1 are the secret.  By default the modexps follow a sliding-window tape
that is a function of the exponent's bits, and the table row a window reads is chosen by its digits: timing and table
addresses depend on p and q, in the same class as gmpy2's ``mpz_powm``.  ``Engine.set_fixed_window(True)`` makes the
sequence of operations depend on the bit lengths only (the table rows read still depend on the digits); it applies to
both plans.  The plan cache of the engine holds constants derived from p and q in device memory for as long as the
engine keeps the plan.

This path is for a plain key.  It never applies to the distributed key of this package (``GpuPaillierSharedKey``), whose
primes nobody knows: there the threshold route — partial decryptions and their recombination — is the only one.
"""

from __future__ import annotations

import math
from typing import Any, Iterable, List, Sequence, Tuple


def crt_constants(p: int, q: int) -> Tuple[int, int, int]:
    """(h_p, h_q, p^-1 mod q) of the key with the primes p and q; ValueError for an even or too small prime, p == q, or
    gcd(pq, (p-1)(q-1)) != 1 (then N + 1 does not generate what decryption needs and h_p or h_q does not exist)."""
    if p < 3 or q < 3 or p % 2 == 0 or q % 2 == 0:
        raise ValueError("p and q must be odd primes")
    if p == q:
        raise ValueError("p and q must differ")
    n = p * q
    if math.gcd(n, (p - 1) * (q - 1)) != 1:
        raise ValueError("gcd(pq, (p-1)(q-1)) must be 1")
    try:
        h_p = pow((pow(n + 1, p - 1, p * p) - 1) // p, -1, p)
        h_q = pow((pow(n + 1, q - 1, q * q) - 1) // q, -1, q)
    except ValueError:
        raise ValueError("p and q are no Paillier key: L((N+1)^(p-1)) is not invertible") from None
    return h_p, h_q, pow(p, -1, q)


_NOT_VALID = ("Not a valid ciphertext under this key: c^(p-1) is not 1 modulo p or c^(q-1) not 1 modulo q "
              "(the ciphertext shares a factor with N)")


class PaillierPrivateKey:
    """The private key (p, q) of the public key N = p q with generator N + 1, decrypting batches on the GPU.

    Primality is the caller's business: the constructor refuses an even "prime", p == q and gcd(pq, (p-1)(q-1)) != 1,
    and tests nothing else — two odd composites that pass these checks give a key that decrypts wrongly.  ``engine`` is
    injected so that the host logic is testable without a GPU; the default is the process-wide HIP engine."""

    def __init__(self, p: int, q: int, engine: Any = None) -> None:
        p, q = int(p), int(q)
        self.h_p, self.h_q, self.p_inv = crt_constants(p, q)
        self.p, self.q = p, q
        self.n = p * q
        self.n_square = self.n * self.n
        self._engine = engine

    def _eng(self, engine: Any = None) -> Any:
        if engine is not None:
            return engine
        if self._engine is None:
            from .engine import default_engine

            self._engine = default_engine()
        return self._engine

    def decrypt_t(self, cts_t, engine: Any = None):
        """Device rows [batch, limbs(N^2)] of ciphertexts -> (plaintext rows [batch, limbs(N)], status uint8 [batch]) on
        the device, nothing fetched: ``Engine.private_decrypt_t``.  The caller reads the status (module docstring)."""
        return self._eng(engine).private_decrypt_t(cts_t, self.p, self.q)

    def decrypt_batch(self, cts: Sequence[int], signed: bool = False, engine: Any = None, return_ok: bool = False):
        """[decrypt(c) for c in cts] as one GPU batch.  ``signed=True`` maps m > N/2 to m - N.  A ciphertext with a
        non-zero status raises ValueError — like ``GpuPaillierSharedKey.decrypt_batch`` for a combination that is not 1
        modulo N — unless ``return_ok=True``: then the result is ``(messages, ok)`` and the message is 0 where ok is
        False."""
        vals = cts if isinstance(cts, list) else list(cts)
        if not vals:
            return ([], []) if return_ok else []
        msgs, ok = self._eng(engine).private_decrypt_batch(vals, self.p, self.q)
        if not return_ok and not all(ok):
            raise ValueError(_NOT_VALID)
        if signed:
            half, n = self.n // 2, self.n
            msgs = [m - n if m > half and good else m for m, good in zip(msgs, ok)]
        return (msgs, ok) if return_ok else msgs

    def decrypt(self, ciphertext: int, signed: bool = False) -> int:
        return self.decrypt_batch([ciphertext], signed=signed)[0]

    def decrypt_sequence(self, objs: Iterable[Any], signed: bool = False, engine: Any = None, return_ok: bool = False):
        """decrypt_batch over ciphertext OBJECTS: anything with ``get_value()`` (the reference's PaillierCiphertext,
        ``PlainCiphertext``), read the way ``homomorphic`` reads its operands; plain ints pass through."""
        vals: List[int] = [int(o.get_value()) if hasattr(o, "get_value") else int(o) for o in objs]
        return self.decrypt_batch(vals, signed=signed, engine=engine, return_ok=return_ok)
