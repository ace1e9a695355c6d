"""Range proofs for Paillier ciphertexts: a sender proves that c = (1 + N)^m r^N holds a value of the promised size, and
the receiver checks it before a homomorphic map (``histogram``, ``cumsum``, ``matmul``, ``slots``, ``packing`` ...)
multiplies it into everybody else's — the Paillier range proof with a Pedersen commitment over an auxiliary RSA modulus
(Fujisaki-Okamoto 1997, MacKenzie-Reiter 2001; Pi^enc of Canetti-Gennaro-Goldfeder-Makriyannis-Peled 2021, Fig. 14), on
the GPU engine.  This is the second thing the safe primes of ``PaillierPrivateKey.generate(.., safe=True)`` are for.

    parameters  Nh = ph qh (safe primes), t = tau^2, s = t^lambda mod Nh — made by the VERIFIER, who proves s in <t>
    statement   c = (1 + N)^m r^N mod N^2 with 0 <= m < 2^l;   l + 258 <= bits(N) - 1
    prove       alpha < 2^(l + 256), mu < 2^(Bh + 128), gamma < 2^(Bh + 384), rho a residue modulo N    (Bh = bits(Nh))
                S = s^m t^mu mod Nh,  A = (1 + N)^alpha rho^N mod N^2,  C = s^alpha t^gamma mod Nh
                e = SHA-256(ctx | c | S | A | C)[:16];  z1 = alpha + e m,  z2 = rho r^e mod N,  z3 = gamma + e mu
    verify      S, C < Nh;  A, c < N^2;  z2 < N;  z1 < 2^(l + 257);  z3 < 2^(Bh + 385)
                (1 + N)^z1 z2^N = A c^e (mod N^2);   s^z1 t^z3 = C S^e (mod Nh)

tools/range_model.py is the model that pins every byte (ctx, the hashed message, the row widths, the draw order);
DESIGN.md §4.26 has the design and the measurements.  The products modulo Nh run through ``Engine.multiexp_mod_t``
(csrc/mx_multiexp.hpp) where that measured faster — auxiliary moduli above 2084 bits — and through one modexp per term
elsewhere, as does rho r^e modulo N; z1 and z3 through ``Engine.response_rows_t`` (csrc/mx_response.hpp).

What this is and is not — read before use:

  * WHAT IS PROVEN is |m| < 2^(l + 257) — the usual slack of E + K + 1 = 257 bits — and NOT m < 2^l: an honest prover
    with m = 2^l, or a good deal more, still passes.  Size the slots and bounds of what consumes the ciphertext for
    l + 257 bits.  It is a proof of KNOWLEDGE of m and r.  It bounds the WHOLE plaintext, not each slot of a slot-packed
    one: a proof per slot is out of scope here — ``membership`` proves that a ciphertext holds one of a few public
    values EXACTLY (a bit, a one-hot ballot ``slots.one_hot_values``, a small slot value before ``packing.pack``).
  * No sign appears anywhere: m is a non-negative integer.  A caller with signed values v in [-2^(l-1), 2^(l-1)) proves
    m = v + 2^(l-1) (and the receiver subtracts the offset's ciphertext homomorphically, or accounts for it in the sum).
  * Soundness holds under the strong RSA assumption in Nh, in the random-oracle model (SHA-256, a 128-bit challenge),
    and only against a prover who does NOT know ph, qh or lambda: the verifier makes the parameters
    (``RangeParameters.generate``), keeps the secret part to itself and may throw it away.
  * Hiding is statistical, 2^-128 per proof, and rests on (a) s lying in the group t generates — the prover checks the
    verifier's ``prove_parameters`` with ``verify_parameters``, 128 binary-challenge rounds, host arithmetic in Python
    ints once per parameter set — and (b) alpha, mu, gamma, rho NEVER REPEATING: they come from a
    ``device_rng.DeviceRng`` (read its docstring) and its nonce discipline.
  * ``label`` binds a proof to a sender and a session: a proof does not verify under another label, another N, other
    parameters or another l.  A verdict says NOTHING ABOUT FRESHNESS: whoever saw (c, proof) can send it again under
    the same label.
  * The commitments travel, not e: the verifier takes no inverse of anything the prover sent, and a malformed row (a
    value out of range, too long, negative) is a False verdict for that row, never an exception.
  * rho is NOT checked to be a unit modulo N, as ``encrypt_fresh_batch`` does not check its r: at real key lengths a
    non-unit does not occur, and it would factor N.
  * Side channels.  The multi-exponentiations gather table rows by the digits of m, mu, alpha, gamma — the same class of
    side channel as every windowed modexp of this engine.  The responses z1 and z3 are computed with
    control flow and addresses that do not depend on the secrets (csrc/mx_response.hpp).
"""

from __future__ import annotations

import hashlib
import math
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from . import limbs as _limbs, proof_flows as _flows
from .proof_flows import E_BITS, K_BITS  # noqa: F401  (the challenge width and the statistical hiding margin)

ROUNDS = 128                     # rounds of the parameter proof
TAG = b"mxpaillier/range-proof/v1"
PTAG = b"mxpaillier/range-parameters/v1"


def _lp(data: bytes) -> bytes:
    return len(data).to_bytes(4, "big") + data


def _int_bytes(x: int) -> bytes:
    return int(x).to_bytes(max(1, (int(x).bit_length() + 7) // 8), "big")


def _engine_of(engine: Any) -> Any:
    if engine is not None:
        return engine
    from .engine import default_engine

    return default_engine()


def _host(rows_t) -> np.ndarray:
    return rows_t if isinstance(rows_t, np.ndarray) else rows_t.detach().cpu().numpy().view(np.uint32)


def _rows_of(values: Sequence[int], words: int) -> Tuple[np.ndarray, List[bool]]:
    """ints -> uint32 rows; a value that is negative or does not fit the row becomes a zero row and False."""
    vals = [int(v) for v in values]
    fits = [0 <= v < 1 << (32 * words) for v in vals]
    return _limbs.pack([v if f else 0 for v, f in zip(vals, fits)], words).reshape(len(vals), words), fits


def shape(n: int, nh: int, bits: int) -> dict:
    """Bit lengths and row widths of a proof (tools/range_model.py: shape).  ValueError — the refusal every entry point
    makes before any engine call — unless 1 <= bits and bits + E + K + 2 <= bits(N) - 1."""
    n = int(n)
    if n < 3 or n % 2 == 0:
        raise ValueError("N must be odd")
    return _flows.range_shape(n, nh, bits)


class RangeParameters:
    """The verifier's public parameters (Nh, s, t).  ``generate`` returns them with the secret part; the prover receives
    ``to_ints()`` and the proof of ``prove_parameters`` and checks it with ``verify_parameters``."""

    def __init__(self, nh: int, s: int, t: int) -> None:
        nh, s, t = int(nh), int(s), int(t)
        if nh < 3 or nh % 2 == 0:
            raise ValueError("the auxiliary modulus must be odd")
        if not (0 < s < nh and 0 < t < nh):
            raise ValueError("s and t must lie in (0, Nh)")
        self.nh, self.s, self.t = nh, s, t
        self.bits = nh.bit_length()
        self.limbs = _limbs.limbs_for(nh)

    def __repr__(self) -> str:
        return f"RangeParameters(bits={self.bits})"

    def to_ints(self) -> Tuple[int, int, int]:
        return self.nh, self.s, self.t

    @classmethod
    def from_ints(cls, nh: int, s: int, t: int) -> "RangeParameters":
        return cls(nh, s, t)

    @classmethod
    def from_primes(cls, ph: int, qh: int, lam: int, tau: int) -> Tuple["RangeParameters", Tuple[int, int, int]]:
        """(parameters, (lambda, ph, qh)) from chosen secrets: t = tau^2, s = t^lambda mod ph qh."""
        ph, qh, lam, tau = int(ph), int(qh), int(lam), int(tau)
        nh = ph * qh
        if ph == qh or ph % 4 != 3 or qh % 4 != 3:
            raise ValueError("ph and qh must be distinct safe primes")
        if math.gcd(tau, nh) != 1 or not 0 <= lam < ((ph - 1) // 2) * ((qh - 1) // 2):
            raise ValueError("tau must be a unit modulo Nh and lambda must lie below ph' qh'")
        t = tau * tau % nh
        return cls(nh, pow(t, lam, nh), t), (lam, ph, qh)

    @classmethod
    def generate(cls, bits: int, engine: Any = None, rng: Any = None, rand: Any = None, check: bool = True
                 ) -> Tuple["RangeParameters", Tuple[int, int, int]]:
        """(parameters, (lambda, ph, qh)) with a fresh Nh of `bits` bits: two safe primes from
        ``PaillierPrivateKey.generate(bits, safe=True)`` (``rng``: its ``DeviceRng``), vetted with
        ``check_primes(safe=True)`` unless ``check=False``; tau and lambda from ``rand`` (anything with ``randrange``,
        default ``secrets.SystemRandom()``; draw order lambda, then candidates for tau until one is a unit).  The
        secret part must not reach a prover."""
        from .private_key import PaillierPrivateKey

        key = PaillierPrivateKey.generate(int(bits), rng=rng, engine=engine, safe=True)
        if check and not key.check_primes(safe=True, engine=engine):
            raise ValueError("the generated primes are not both safe primes")
        if rand is None:
            import secrets

            rand = secrets.SystemRandom()
        ph, qh = int(key.p), int(key.q)
        lam = rand.randrange(((ph - 1) // 2) * ((qh - 1) // 2))
        while True:
            tau = rand.randrange(2, ph * qh)
            if math.gcd(tau, ph * qh) == 1:
                break
        return cls.from_primes(ph, qh, lam, tau)

    def _parameter_challenge(self, commitments: Sequence[int]) -> List[int]:
        msg = _lp(PTAG) + b"".join(_lp(_int_bytes(x)) for x in (self.nh, self.s, self.t, *commitments))
        word = int.from_bytes(hashlib.sha256(msg).digest()[: ROUNDS // 8], "big")
        return [(word >> (ROUNDS - 1 - i)) & 1 for i in range(ROUNDS)]

    def prove_parameters(self, secret: Tuple[int, int, int], rand: Any = None) -> Tuple[List[int], List[int]]:
        """The proof (a_0 .. a_127, z_0 .. z_127) that s lies in the group t generates, from the secret
        (lambda, ph, qh): a_i = t^(r_i), bits e_i from SHA-256, z_i = r_i + e_i lambda mod ph' qh'."""
        lam, ph, qh = (int(x) for x in secret)
        if ph * qh != self.nh or pow(self.t, lam, self.nh) != self.s:
            raise ValueError("the secret does not belong to these parameters")
        if rand is None:
            import secrets

            rand = secrets.SystemRandom()
        order = ((ph - 1) // 2) * ((qh - 1) // 2)
        rs = [rand.randrange(order) for _ in range(ROUNDS)]
        commitments = [pow(self.t, r, self.nh) for r in rs]
        return commitments, [(r + e * lam) % order for r, e in zip(rs, self._parameter_challenge(commitments))]

    def verify_parameters(self, proof: Tuple[Sequence[int], Sequence[int]]) -> bool:
        """True iff t^(z_i) = a_i s^(e_i) in all 128 rounds (and s, t are units): what the prover's zero-knowledge rests
        on when the verifier made Nh.  Never raises for a malformed proof."""
        try:
            commitments, zs = proof
            commitments, zs = [int(a) for a in commitments], [int(z) for z in zs]
        except (TypeError, ValueError):
            return False
        nh = self.nh
        if len(commitments) != ROUNDS or len(zs) != ROUNDS or math.gcd(self.s, nh) != 1 or math.gcd(self.t, nh) != 1:
            return False
        if any(not 0 < a < nh for a in commitments) or any(not 0 <= z < nh for z in zs):
            return False
        es = self._parameter_challenge(commitments)
        return all(pow(self.t, z, nh) == a * (self.s if e else 1) % nh for a, z, e in zip(commitments, zs, es))


def context(n: int, params: RangeParameters, bits: int, label: bytes) -> bytes:
    """The 32 bytes that bind a proof to N, the parameters, the claimed length and the caller's label."""
    fields = [_int_bytes(x) for x in (n, params.nh, params.s, params.t, bits)] + [bytes(label)]
    return hashlib.sha256(_lp(TAG) + b"".join(_lp(f) for f in fields)).digest()


class RangeProofs:
    """The proofs of a batch of ciphertexts: the rows of S and C (``[count, limbs(Nh)]``), A (``[count, limbs(N^2)]``),
    z1, z2 and z3 — device tensors where they were made on the device, uint32 numpy rows where they arrived as ints.
    ``unfit[r]`` marks a row whose integers did not fit the rows (its verdict is False)."""

    FIELDS = ("s", "a", "c", "z1", "z2", "z3")

    def __init__(self, s, a, c, z1, z2, z3, unfit: Optional[List[bool]] = None) -> None:
        self.s, self.a, self.c, self.z1, self.z2, self.z3 = s, a, c, z1, z2, z3
        self.unfit = unfit

    def __len__(self) -> int:
        return int(self.s.shape[0])

    def rows(self) -> Tuple[Any, ...]:
        return tuple(getattr(self, f) for f in self.FIELDS)

    def to_ints(self) -> Tuple[List[int], ...]:
        """(S, A, C, z1, z2, z3) as lists of ints — what travels to the verifier."""
        return tuple(_limbs.unpack(_host(t)) for t in self.rows())

    @classmethod
    def from_ints(cls, s: Sequence[int], a: Sequence[int], c: Sequence[int], z1: Sequence[int], z2: Sequence[int], z3: Sequence[int],
                  n: int, params: RangeParameters, bits: int) -> "RangeProofs":
        """The proofs received as ints, as rows under (N, params, l)."""
        sh = shape(n, params.nh, bits)
        cols = (s, a, c, z1, z2, z3)
        if any(len(col) != len(s) for col in cols):
            raise ValueError("one S, A, C, z1, z2 and z3 per ciphertext expected")
        widths = (sh["limbs_h"], sh["limbs2"], sh["limbs_h"], sh["z1_words"], sh["limbs_n"], sh["z3_words"])
        packed = [_rows_of(col, w) for col, w in zip(cols, widths)]
        unfit = [not all(p[1][r] for p in packed) for r in range(len(s))]
        return cls(*(p[0] for p in packed), unfit)


def _check_statement(n: int, params: RangeParameters, bits: int, label: bytes) -> dict:
    if not isinstance(params, RangeParameters):
        raise ValueError("RangeParameters expected")
    if not isinstance(label, (bytes, bytearray)):
        raise ValueError("the label must be bytes")
    return shape(n, params.nh, bits)


def prove_batch(n: int, params: RangeParameters, bits: int, messages: Sequence[int], randomness: Sequence[int], label: bytes,
                rng: Any = None, ciphertexts: Optional[Sequence[int]] = None, engine: Any = None, draws: Any = None) -> RangeProofs:
    """The proofs that c_r = (1 + n)^(m_r) (r_r)^n mod n^2 hold values of `bits` bits, for messages m_r >= 0 and the
    randomness r_r the ciphertexts were made with (``ciphertexts``: the c_r if the caller has them, else they are
    recomputed).  ``rng``: a ``DeviceRng`` (default: a fresh one); ``draws``: the four row sets, for tests.  ValueError —
    before any engine call — for a length N cannot carry, lists of unequal lengths, a negative message or one that does
    not fit a row of z1.  A message of 2^bits or more is NOT refused: the proof then fails, or passes within the slack
    (module docstring); the ciphertext of a message of N or more is that of m mod N, as ``Engine.encrypt_batch`` makes
    it.  The modexp of the message term is as long as the longest message of the batch (at least `bits`): its duration
    shows that length, never a message."""
    n = int(n)
    sh = _check_statement(n, params, bits, label)
    msgs, rands = [int(m) for m in messages], [int(r) for r in randomness]
    if len(msgs) != len(rands) or (ciphertexts is not None and len(ciphertexts) != len(msgs)):
        raise ValueError("one randomness (and one ciphertext) per message expected")
    if any(m < 0 or m >> (32 * sh["z1_words"]) for m in msgs):
        raise ValueError("messages must be non-negative and fit a row of z1 (a signed value v is proven as v + 2^(l - 1))")
    if not msgs:
        return RangeProofs(*(np.zeros((0, sh[w]), dtype=np.uint32) for w in ("limbs_h", "limbs2", "limbs_h", "z1_words", "limbs_n", "z3_words")))
    eng = _engine_of(engine)
    n2 = n * n
    if ciphertexts is None:
        ciphertexts = eng.encrypt_batch(msgs, rands, n)
    if draws is None and rng is None:
        from .device_rng import DeviceRng

        rng = DeviceRng()
    cts_t = eng.to_device(_limbs.pack_reduced(list(ciphertexts), sh["limbs2"], n2).reshape(len(msgs), sh["limbs2"]))
    m_t = eng.to_device(_limbs.pack(msgs, sh["z1_words"]).reshape(len(msgs), sh["z1_words"]))
    r_t = eng.to_device(_limbs.pack_reduced(rands, sh["limbs_n"], n).reshape(len(msgs), sh["limbs_n"]))
    source = dict(draws=draws) if draws is not None else dict(rng=rng)
    message_bits = max(int(bits), max(m.bit_length() for m in msgs))          # honest messages: the modexp s^m is l bits long
    return RangeProofs(*eng.range_prove_t(cts_t, m_t, r_t, n, params.nh, params.s, params.t, int(bits), context(n, params, bits, label),
                                          message_bits=message_bits, **source))


def encrypt_with_proof(n: int, params: RangeParameters, bits: int, messages: Sequence[int], label: bytes, rng: Any = None,
                       engine: Any = None) -> Tuple[List[int], RangeProofs]:
    """(ciphertexts, proofs): fresh encryptions of the messages (``Engine.encrypt_fresh_batch``, the randomness drawn
    on the device and kept for the proof) with their range proofs.  Messages must lie in [0, 2^bits)."""
    n = int(n)
    _check_statement(n, params, bits, label)
    msgs = [int(m) for m in messages]
    if any(not 0 <= m < 1 << int(bits) for m in msgs):
        raise ValueError("messages in [0, 2^bits) expected")
    eng = _engine_of(engine)
    if rng is None:
        from .device_rng import DeviceRng

        rng = DeviceRng()
    cts, rands = eng.encrypt_fresh_batch(msgs, n, rng, return_randomness=True)
    return cts, prove_batch(n, params, bits, msgs, rands, label, rng=rng, ciphertexts=cts, engine=eng)


def verify_batch(n: int, params: RangeParameters, bits: int, ciphertexts: Sequence[int], proofs: RangeProofs, label: bytes,
                 engine: Any = None) -> List[bool]:
    """[is row r a valid proof that ciphertexts[r] holds a value below 2^(bits + 257)] — never raises for a bad row: a
    value that is negative, out of range or too long is a False.  ValueError — before any engine call — for a length N
    cannot carry or a number of proofs other than the number of ciphertexts."""
    n = int(n)
    sh = _check_statement(n, params, bits, label)
    count = len(ciphertexts)
    if len(proofs) != count:
        raise ValueError("one proof per ciphertext expected")
    if count == 0:
        return []
    eng = _engine_of(engine)
    c_rows, c_fit = _rows_of(ciphertexts, sh["limbs2"])
    if proofs.unfit is None and not isinstance(proofs.s, np.ndarray):
        rows = proofs.rows()
    else:
        rows = tuple(eng.to_device(np.asarray(t)) for t in proofs.rows())
    unfit = proofs.unfit or [False] * count
    verdict = eng.range_verify_t(eng.to_device(c_rows), *rows, n, params.nh, params.s, params.t, int(bits), context(n, params, bits, label))
    got = [bool(x) for x in (verdict if isinstance(verdict, np.ndarray) else verdict.cpu().numpy())]
    return [g and f and not u for g, f, u in zip(got, c_fit, unfit)]
