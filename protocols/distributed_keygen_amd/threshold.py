"""Threshold Paillier with a dealer: dealt key shares, partial decryptions that carry a proof, and decryption from any
t + 1 verified partials — Damgård–Jurik 2001 §4.1 with s = 1 (the proof is Shoup's, 2000), on the GPU engine.

This is what the safe primes of ``PaillierPrivateKey.generate(.., safe=True)`` are for.  The distributed key of this
package (``GpuPaillierSharedKey``) is a different object: nobody knows its primes, its players are fixed to 1 .. t + 1
and a wrong partial decryption is noticed only because the combination is not 1 modulo N — nobody can tell who sent it.
Here every partial decryption comes with a non-interactive proof that it was made with the dealt share, every row gets a
verdict of its own, the cheater is named, and any other t + 1 parties decrypt.

    deal      p = 2p' + 1, q = 2q' + 1 safe primes, N = pq, m = p'q', n parties, t = the polynomial's degree
              d = m (m^-1 mod N);  f(X) = d + a_1 X + .. + a_t X^t mod N m;  s_i = f(i);  Delta = n!;  x_i = Delta s_i
              v = u^2 mod N^2 for a random unit u;  w_i = v^(x_i) mod N^2;  theta^-1 = (4 Delta^2)^-1 mod N
    partial   c_i = c^(2 x_i) mod N^2                                          (Engine.powmod_nsquare_t)
    proof     log_chat(c_i^2) = log_v(w_i) for chat = c^4:  rho < 2^(X + 256), X = bits(N m Delta)
              a = chat^rho, b = v^rho, e = SHA-256(ctx | chat | c_i^2 | a | b)[:16], z = rho + e x_i   (Engine.dleq_prove_t)
    verify    a, b, c_i < N^2, z < 2^(X + 257), chat^z = a (c_i^2)^e, v^z = b w_i^e           (Engine.dleq_verify_t)
    combine   lambda_i = Delta prod_{j in S, j != i} j / (j - i);  c' = prod c_i^(2 lambda_i);  M = L(c') theta^-1 mod N

tools/proof_model.py is the model that pins every byte (ctx, the hashed message, the row layouts); DESIGN.md §4.25 has
the design and the measurements.

What this is and is not — read before use:

  * THE DEALER KNOWS EVERYTHING: p, q, every share.  ``deal`` runs where the private key lives; the scheme protects
    against parties that misbehave afterwards, not against the dealer.  Dealing is host arithmetic in Python ints, once
    per key; its randomness is ``secrets.SystemRandom`` unless a test injects another source.
  * Hiding is statistical: z = rho + e x_i with rho 128 bits longer than e x_i can get, so a proof reveals x_i with an
    advantage of at most 2^-128 per proof.  rho comes from a ``device_rng.DeviceRng`` (read its docstring too) and
    must never repeat: two proofs with the same rho and different challenges give x_i away.
  * Soundness holds in the random-oracle model (SHA-256 as the oracle, a 128-bit challenge) and NEEDS SAFE PRIMES: the
    squares modulo N^2 must form a cyclic group whose order N m has no small factor.  ``deal`` therefore vets the key
    with ``check_primes(safe=True)`` unless told otherwise.  ctx binds a proof to the key, the party and the
    parameters; a proof does not transfer to another party, key or ciphertext.
  * The commitments a and b travel, not e: the verifier takes no inverse of anything a party sent, and a malformed row
    (a value of N^2 or more, a z that is too long) is a False verdict for that row, never an exception.
  * Decryption results and partial decryptions are NOT fresh ciphertexts, and the combination is a plaintext.
  * Side channels.  The partial decryption follows the tape of the share like every modexp of this engine
    (``Engine.set_fixed_window``); a = chat^rho and b = v^rho gather table rows by the digits of rho — the same class of
    side channel as the tape on the share.  The response z = rho + e x_i is computed with control
    flow and addresses that do not depend on x_i, rho or e (csrc/mx_response.hpp).  Plans and the share's row stay in
    device memory for as long as their objects live.
"""

from __future__ import annotations

import hashlib
import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import limbs as _limbs
from .range_proof import _int_bytes, _lp, _rows_of

E_BITS = 128                     # challenge width
K_BITS = 128                     # statistical hiding margin
MAX_PIECES = 8                   # pieces a row of rho or z may have
TAG = b"mxpaillier/threshold-dleq/v1"

_NOT_ONE = ("Combined decryption minus one is not divisible by N. This might be caused by the "
            "fact that the ciphertext that is being decrypted, differs between the parties.")


def split_shape(n_bits: int, z_bits: int) -> Tuple[int, int]:
    """(pieces, kw): rows of z_bits bits as equal word-aligned pieces of at most (2 n_bits + 64) / 32 words — what the
    multi-exponentiation and the fixed-base tables take as one exponent."""
    kw_max = (2 * n_bits + 64) // 32
    wz = -(-z_bits // 32)
    pieces = -(-wz // kw_max)
    return pieces, -(-wz // pieces)


def lagrange(delta: int, subset: Sequence[int]) -> Dict[int, int]:
    """lambda_i = delta prod_{j in S, j != i} j / (j - i) for i in S: integers (delta = n! clears every denominator),
    some of them negative."""
    out = {}
    for i in subset:
        num, den = delta, 1
        for j in subset:
            if j != i:
                num *= j
                den *= j - i
        out[i] = num // den
    return out


def _engine_of(engine: Any, fallback: Any) -> Any:
    if engine is not None:
        return engine
    if fallback is not None:
        return fallback
    from .engine import default_engine

    return default_engine()


def _cat(parts):
    if isinstance(parts[0], np.ndarray):
        return np.concatenate(parts)
    import torch

    return torch.cat(parts)


class DecryptionProofs:
    """The proofs of one party for a batch of ciphertexts: the rows of a and b (``[count, limbs(N^2)]``) and of z
    (``[count, pieces * kw]``) — device tensors where they were made on the device, uint32 numpy rows where they arrived
    as ints.  ``unfit[r]`` marks a row whose integers did not fit the rows (its verdict is False)."""

    def __init__(self, a, b, z, unfit: Optional[List[bool]] = None) -> None:
        self.a, self.b, self.z = a, b, z
        self.unfit = unfit

    def __len__(self) -> int:
        return int(self.a.shape[0])

    def to_ints(self) -> Tuple[List[int], List[int], List[int]]:
        """(a, b, z) as lists of ints — what travels to the verifiers."""
        return tuple(_limbs.unpack(t if isinstance(t, np.ndarray) else t.detach().cpu().numpy().view(np.uint32))
                     for t in (self.a, self.b, self.z))      # type: ignore[return-value]

    @classmethod
    def from_ints(cls, a: Sequence[int], b: Sequence[int], z: Sequence[int], public_key: "ThresholdPublicKey") -> "DecryptionProofs":
        """The proofs received as ints, as rows under `public_key`."""
        if not len(a) == len(b) == len(z):
            raise ValueError("one a, b and z per ciphertext expected")
        (ra, fa), (rb, fb), (rz, fz) = _rows_of(a, public_key.limbs2), _rows_of(b, public_key.limbs2), _rows_of(z, public_key.z_words)
        return cls(ra, rb, rz, [not (x and y and w) for x, y, w in zip(fa, fb, fz)])


class ThresholdPublicKey:
    """What every party and every verifier holds: N, the number of parties n, the threshold t (the degree: t + 1 partials
    decrypt), v, the verification keys w_1 .. w_n and X = bits(N m Delta) (its only trace of m is that bit length)."""

    def __init__(self, n: int, parties: int, threshold: int, v: int, verification_keys: Sequence[int], x_bits: int,
                 engine: Any = None) -> None:
        n, parties, threshold, x_bits = int(n), int(parties), int(threshold), int(x_bits)
        if parties < 2 or not 0 < threshold < parties:
            raise ValueError("parties >= 2 and 1 <= threshold < parties expected")
        if len(verification_keys) != parties:
            raise ValueError("one verification key per party expected")
        if n < 3 or n % 2 == 0:
            raise ValueError("N must be odd")
        self.n, self.parties, self.threshold, self.v, self.x_bits = n, parties, threshold, int(v), x_bits
        self.verification_keys = [int(w) for w in verification_keys]
        self.n_square = n * n
        self.limbs2 = _limbs.limbs_for(self.n_square)
        self.delta = math.factorial(parties)
        self.theta_inv = pow(4 * self.delta * self.delta, -1, n)
        self.rho_bits = x_bits + E_BITS + K_BITS
        self.z_bits = self.rho_bits + 1
        self.pieces, self.kw = split_shape(n.bit_length(), self.z_bits)
        if self.pieces > MAX_PIECES:
            raise ValueError(f"rows of {self.z_bits} bits need {self.pieces} pieces under this N; at most {MAX_PIECES} are supported "
                             "(fewer parties, or a longer key)")
        self.z_words = self.pieces * self.kw
        self._engine = engine
        self._v_bases: Optional[List[int]] = None

    def _eng(self, engine: Any = None) -> Any:
        self._engine = _engine_of(engine, self._engine)
        return self._engine

    def verification_key(self, index: int) -> int:
        if not isinstance(index, int) or not 1 <= index <= self.parties:
            raise ValueError(f"unknown party {index!r}: the parties are 1 .. {self.parties}")
        return self.verification_keys[index - 1]

    def ctx(self, index: int) -> bytes:
        """The 32 bytes that bind a proof to this key and party: SHA-256 over the domain tag and the length-prefixed
        N, v, w_i, i, n, t (tools/proof_model.py: context)."""
        fields = (self.n, self.v, self.verification_key(index), index, self.parties, self.threshold)
        return hashlib.sha256(_lp(TAG) + b"".join(_lp(_int_bytes(x)) for x in fields)).digest()

    @property
    def v_bases(self) -> List[int]:
        """v^(2^(32 kw j)) mod N^2 for j < pieces: the bases of the fixed-base tables (public; host squarings, once)."""
        if self._v_bases is None:
            out = [self.v % self.n_square]
            for _ in range(self.pieces - 1):
                out.append(pow(out[-1], 1 << (32 * self.kw), self.n_square))
            self._v_bases = out
        return self._v_bases

    # ---- verification
    def verify_t(self, index: int, cts_t, partials_t, proofs: DecryptionProofs, engine: Any = None):
        """bool ``[count]`` on the device: the verdict of every row of party `index` (``Engine.dleq_verify_t``)."""
        eng = self._eng(engine)
        return eng.dleq_verify_t(cts_t, partials_t, proofs.a, proofs.b, proofs.z, self.n, self.v_bases, self.verification_key(index),
                                 self.ctx(index), self.z_bits, self.kw)

    def verify_batch(self, index: int, cts: Sequence[int], partials: Sequence[int], proofs: DecryptionProofs, engine: Any = None) -> List[bool]:
        """[is row r of party `index` a valid proof for (cts[r], partials[r])] — never raises for a bad row: a value
        that is negative, N^2 or more, or too long is a False."""
        w = self.verification_key(index)          # (an unknown index is the caller's mistake: ValueError)
        count = len(cts)
        if len(partials) != count or len(proofs) != count:
            raise ValueError("one partial decryption and one proof per ciphertext expected")
        if count == 0:
            return []
        eng = self._eng(engine)
        c_rows, c_fit = _rows_of(cts, self.limbs2)
        p_rows, p_fit = _rows_of(partials, self.limbs2)
        if proofs.unfit is None and not isinstance(proofs.a, np.ndarray):
            a_t, b_t, z_t = proofs.a, proofs.b, proofs.z
            unfit = [False] * count
        else:
            a_t, b_t, z_t = (eng.to_device(np.asarray(t)) for t in (proofs.a, proofs.b, proofs.z))
            unfit = proofs.unfit or [False] * count
        verdict = eng.dleq_verify_t(eng.to_device(c_rows), eng.to_device(p_rows), a_t, b_t, z_t, self.n, self.v_bases, w,
                                    self.ctx(index), self.z_bits, self.kw)
        got = [bool(x) for x in (verdict if isinstance(verdict, np.ndarray) else verdict.cpu().numpy())]
        return [g and cf and pf and not u for g, cf, pf, u in zip(got, c_fit, p_fit, unfit)]

    # ---- combination
    def _subset(self, indices) -> List[int]:
        idx = sorted(indices)
        for i in idx:
            self.verification_key(i)              # ValueError for an unknown index
        if len(idx) < self.threshold + 1:
            raise KeyError(f"{self.threshold + 1} partial decryptions needed, {len(idx)} given")
        return idx[: self.threshold + 1]

    def combine_t(self, partials: Dict[int, Any], engine: Any = None):
        """{index: partial rows ``[count, limbs(N^2)]``} of any t + 1 parties (of more, the t + 1 lowest indices are
        used) -> (plaintext rows ``[count, limbs(N)]``, status uint8 ``[count]``) in ``Engine.combine_t``'s format:
        ``slots.decode_t`` and ``packing.unpack`` take the rows unchanged.  c' = prod c_i^(2 lambda_i) runs through
        ``Engine.multiexp_nsquare_t`` — the weights are public and signed — and L(c') theta^-1 through ``combine_t``."""
        idx = self._subset(partials.keys())
        eng = self._eng(engine)
        lam = lagrange(self.delta, idx)
        count = int(partials[idx[0]].shape[0])
        if any(tuple(partials[i].shape) != (count, self.limbs2) for i in idx):
            raise ValueError(f"partial rows [count, {self.limbs2}] expected, the same count from every party")
        if count == 0:
            return eng.combine_t(partials[idx[0]].reshape(1, 0, self.limbs2), self.n, self.theta_inv)
        weights = [{k * count + r: 2 * lam[i] for k, i in enumerate(idx)} for r in range(count)]
        folded_t = eng.multiexp_nsquare_t(_cat([partials[i] for i in idx]), weights, self.n)
        return eng.combine_t(folded_t.reshape(1, count, self.limbs2), self.n, self.theta_inv)

    def combine_batch(self, partials: Dict[int, Sequence[int]], engine: Any = None) -> List[int]:
        """{index: partial decryptions} of any t + 1 parties -> plaintexts.  KeyError for too few indices, ValueError
        for an unknown index or a combination that is not 1 modulo N (a wrong partial: verify, then combine others)."""
        idx = self._subset(partials.keys())
        eng = self._eng(engine)
        count = len(partials[idx[0]])
        if any(len(partials[i]) != count for i in idx):
            raise ValueError("the same number of partial decryptions from every party expected")
        if count == 0:
            return []
        rows = {i: eng.to_device(_limbs.pack_reduced(list(partials[i]), self.limbs2, self.n_square)) for i in idx}
        out_t, status_t = self.combine_t(rows, engine=eng)
        if np.asarray(status_t if isinstance(status_t, np.ndarray) else status_t.cpu().numpy()).any():
            raise ValueError(_NOT_ONE)
        return _limbs.unpack(eng.to_host(out_t))

    def decrypt_verified(self, cts: Sequence[int], contributions: Dict[int, Tuple[Sequence[int], DecryptionProofs]],
                         engine: Any = None) -> Tuple[List[int], List[int]]:
        """(plaintexts, cheaters): verify every party's column against `cts`, drop the parties with any False row (the
        `cheaters`, in index order), and combine the first t + 1 that remain.  ValueError, naming the cheaters, if fewer
        remain; ValueError for an unknown index."""
        for i in contributions:
            self.verification_key(i)
        honest, cheaters = {}, []
        for i in sorted(contributions):
            col, proofs = contributions[i]
            if len(col) == len(cts) == len(proofs) and all(self.verify_batch(i, cts, col, proofs, engine=engine)):
                honest[i] = col
            else:
                cheaters.append(i)
        if len(honest) < self.threshold + 1:
            raise ValueError(f"only {len(honest)} of the needed {self.threshold + 1} parties sent valid proofs; invalid: {cheaters}")
        return self.combine_batch(honest, engine=engine), cheaters


class ThresholdKeyShare:
    """Party `index`'s share: the exponent x_i = Delta s_i (the secret) beside the public key."""

    def __init__(self, public_key: ThresholdPublicKey, index: int, x: int, engine: Any = None) -> None:
        public_key.verification_key(index)
        x = int(x)
        if x < 0 or x.bit_length() > public_key.x_bits:
            raise ValueError("the share does not belong to this key")
        self.public_key, self.index, self.x = public_key, int(index), x
        self._engine = engine
        self._x_t: Any = None
        self._own_rng: Any = None

    def __repr__(self) -> str:
        return f"ThresholdKeyShare(index={self.index}, parties={self.public_key.parties}, threshold={self.public_key.threshold})"

    def _eng(self, engine: Any = None) -> Any:
        eng = _engine_of(engine, self._engine)
        if eng is not self._engine:
            self._engine, self._x_t = eng, None
        return eng

    def _rng(self, rng: Any) -> Any:
        if rng is not None:
            return rng
        if self._own_rng is None:
            from .device_rng import DeviceRng

            self._own_rng = DeviceRng()
        return self._own_rng

    def partial_decrypt_t(self, cts_t, prove: bool = False, rng: Any = None, rho_t: Any = None, engine: Any = None):
        """Ciphertext rows ``[count, limbs(N^2)]`` -> the rows of c^(2 x_i), or ``(rows, DecryptionProofs)`` with
        ``prove=True``: rho from ``rng`` (default: a ``DeviceRng`` the share keeps), or ``rho_t`` for tests."""
        pk = self.public_key
        eng = self._eng(engine)
        if tuple(cts_t.shape[1:]) != (pk.limbs2,):
            raise ValueError(f"ciphertext rows of {pk.limbs2} words expected")
        partials_t = eng.powmod_nsquare_t(cts_t, pk.n, 2 * self.x)
        if not prove:
            return partials_t
        if self._x_t is None:
            self._x_t = eng.to_device(_limbs.pack([self.x], _limbs.limbs_for_bits(pk.x_bits)))
        source = dict(rho_t=rho_t) if rho_t is not None else dict(rng=self._rng(rng))
        a_t, b_t, z_t = eng.dleq_prove_t(cts_t, partials_t, pk.n, pk.v_bases, pk.ctx(self.index), self._x_t, pk.rho_bits, pk.kw, **source)
        return partials_t, DecryptionProofs(a_t, b_t, z_t)

    def partial_decrypt_batch(self, cts: Sequence[int], prove: bool = False, rng: Any = None, rho_t: Any = None, engine: Any = None):
        """[c^(2 x_i) mod N^2 for c in cts], or ``(partials, DecryptionProofs)`` with ``prove=True``.  Ciphertexts are
        taken modulo N^2."""
        pk = self.public_key
        eng = self._eng(engine)
        vals = cts if isinstance(cts, list) else list(cts)
        if not vals:
            empty = np.zeros((0, pk.limbs2), dtype=np.uint32)
            return ([], DecryptionProofs(empty, empty, np.zeros((0, pk.z_words), dtype=np.uint32))) if prove else []
        cts_t = eng.to_device(_limbs.pack_reduced(vals, pk.limbs2, pk.n_square))
        got = self.partial_decrypt_t(cts_t, prove=prove, rng=rng, rho_t=rho_t, engine=eng)
        if not prove:
            return _limbs.unpack(eng.to_host(got))
        return _limbs.unpack(eng.to_host(got[0])), got[1]


def deal(key: Any, parties: int, threshold: int, rng: Any = None, check: bool = True, engine: Any = None
         ) -> Tuple[ThresholdPublicKey, List[ThresholdKeyShare]]:
    """Share the private key `key` (a ``PaillierPrivateKey`` of two safe primes) among `parties` players so that any
    `threshold` + 1 of them decrypt: ``(ThresholdPublicKey, [ThresholdKeyShare of party 1 .. n])``.

    ``check=True`` runs ``key.check_primes(safe=True)`` and refuses a key that fails it (soundness needs safe primes:
    module docstring).  ``rng``: anything with ``randrange`` (default ``secrets.SystemRandom()``); the draw order is
    a_1 .. a_t, then candidates for u until one is a unit.  ValueError — before anything is drawn or launched — for
    ``parties < 2``, ``threshold`` outside [1, parties), or so many parties that rows of X + 257 bits need more than
    MAX_PIECES pieces of (2 bits(N) + 64) / 32 words."""
    parties, threshold = int(parties), int(threshold)
    if parties < 2:
        raise ValueError("at least two parties expected")
    if not 0 < threshold < parties:
        raise ValueError("1 <= threshold < parties expected (threshold + 1 parties decrypt)")
    p, q = int(key.p), int(key.q)
    n = p * q
    m = ((p - 1) // 2) * ((q - 1) // 2)
    nm = n * m
    delta = math.factorial(parties)
    x_bits = (nm * delta).bit_length()
    pieces, _ = split_shape(n.bit_length(), x_bits + E_BITS + K_BITS + 1)
    if pieces > MAX_PIECES:
        raise ValueError(f"{parties} parties are too many for this key: rows of {x_bits + 257} bits need {pieces} pieces, at most "
                         f"{MAX_PIECES} are supported")
    if p % 4 != 3 or q % 4 != 3 or p == q:
        raise ValueError("p and q must be distinct safe primes")
    if check and not key.check_primes(safe=True):
        raise ValueError("p and q are not both safe primes: the proofs would not be sound")
    if rng is None:
        import secrets

        rng = secrets.SystemRandom()
    d = m * pow(m, -1, n)
    coeffs = [d] + [rng.randrange(nm) for _ in range(threshold)]
    xs = [delta * (sum(a * i ** k for k, a in enumerate(coeffs)) % nm) for i in range(1, parties + 1)]
    n2 = n * n
    while True:
        u = rng.randrange(2, n2)
        if math.gcd(u, n) == 1:
            break
    v = u * u % n2
    public = ThresholdPublicKey(n, parties, threshold, v, [pow(v, x, n2) for x in xs], x_bits, engine=engine)
    return public, [ThresholdKeyShare(public, i + 1, x, engine=engine) for i, x in enumerate(xs)]
