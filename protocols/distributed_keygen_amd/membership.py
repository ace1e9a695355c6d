"""One-of-k membership proofs for Paillier ciphertexts: a sender proves that c = (1 + N)^m r^N holds one of a public list
of values S = (s_0 .. s_(k-1)) — EXACTLY, and without saying which — and the receiver checks it before ``histogram``,
``sum_groups`` or a threshold decryption takes the ciphertext into everybody else's tally.  The Cramer-Damgard-Schoenmakers
OR-composition of the Sigma-protocol for N-th residues (Damgard-Jurik 2001 §5; Baudron-Fouque-Pointcheval-Poupard-Stern
2001), on the GPU engine.  Where ``range_proof`` bounds the size of a plaintext with 257 bits of slack, this proof has
none: S = {0, 1} is the bit proof, S = ``slots.one_hot_values(N, b, k)`` is the validity of a one-hot ballot for
slot-packed tallies, and S = {0 .. 2^b - 1} per value followed by the ciphertext-level ``packing.pack`` gives a
slot-packed ciphertext every slot of which is proven.

    statement   c = (1 + N)^(s_i) r^N mod N^2 for some i the prover knows, together with r
                u_j = c (1 + (N - s_j) N) mod N^2 = c (1 + N)^(-s_j),   ub_j = c^-1 (1 + s_j N) mod N^2 = u_j^-1
    prove       zt_j of bits(N) + 64 bits and et_j of 128 bits for ALL j, then et_i = 0        (zt_i serves as omega)
                a_j = zt_j^N ub_j^(et_j) mod N^2;   e = SHA-256(ctx | c | a_0 .. a_(k-1))[:16]
                e_i = e - sum_(j != i) et_j mod 2^128;   z_i = (omega mod N) r^(e_i) mod N,  z_j = zt_j mod N otherwise
    verify      c < N^2;  0 < a_j < N^2;  0 < z_j < N;  sum_j e_j = e (mod 2^128);  z_j^N = a_j u_j^(e_j) (mod N^2) for every j

tools/member_model.py is the model that pins every byte (ctx, the hashed message, the row widths, the draw order);
DESIGN.md §4.27 has the design and the measurements.  The challenge arithmetic — masking the real slot, splitting e,
summing the e_j — runs on the device with control flow and addresses that do not depend on i
(``Engine.member_challenges_t``, csrc/mx_member.hpp); everything else is the engine's N^2 modexp, multi-exponentiation,
hash and inverse.

What this is and is not — read before use:

  * WHAT IS PROVEN is m in S modulo N, exactly, and knowledge of r: no slack.  The cost is linear in k — k modexps of N
    bits and k of 128 bits on each side, 2 k rows of N^2 plus k of N and k challenges to send — so S stays small
    (k <= 16); a long range is ``range_proof``'s business.
  * Soundness is special soundness of the Sigma-protocol in the random-oracle model (SHA-256, a 128-bit challenge), and
    needs EVERY PRIME FACTOR OF N ABOVE 2^128: the caller guarantees that N is a proper key.  ``bits(N) < 260`` is
    refused outright, before any engine call.  It also needs every z_j to be a unit modulo N, and THE VERIFIER REFUSES
    ZERO: a_j = z_j = 0 satisfies 0^N = 0 u_j^(e_j) for any ciphertext and any e_j, so without that check anybody could
    forge a proof with no witness (every slot zero, or one zero slot beside k - 1 simulated ones).  Zero is the only
    non-unit that needs a check: with every prime factor above 2^128 any other non-unit would factor N; and z_j != 0
    forces a_j != 0, which is checked all the same.  No auxiliary modulus, no safe primes, no parameters from the verifier:
    it works for the distributed key, a dealt key and a plain private key alike.
  * Hiding (which s_i it is) is perfect for honest draws and rests on the zt_j and et_j NEVER REPEATING: they come from
    a ``device_rng.DeviceRng`` (read its docstring) and its nonce discipline.
  * ``label`` binds a proof to a sender and a session: a proof does not verify under another label, another N, another
    list or the same list in another order.  A verdict says NOTHING ABOUT FRESHNESS: whoever saw (c, proof) can send it
    again under the same label.
  * The commitments and the split challenges travel: the verifier takes no inverse of anything the prover sent, and a
    malformed row (a value out of range, too long, negative) is a False verdict for that row, never an exception.
  * r is NOT checked to be a unit modulo N, as ``encrypt_fresh_batch`` does not check it: at real key lengths a
    non-unit does not occur, and it would factor N.  The prover inverts its OWN ciphertexts (ValueError for a non-unit).
  * Side channels.  Every slot is drawn, exponentiated, masked, split and placed alike: the real slot is selected by
    compare-and-mask arithmetic, never by a branch or an address.  The table gathers of ub_j^(et_j) are indexed by the
    digits of et_j — zero for the real slot —, the same class of side channel as every windowed modexp of this engine
    (INTEGRATION.md §3).
"""

from __future__ import annotations

import hashlib
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from . import limbs as _limbs, proof_flows as _flows
from .range_proof import E_BITS, _engine_of, _host, _int_bytes, _lp, _rows_of

MIN_BITS = 260                   # every prime factor of N must exceed 2^E_BITS; shorter moduli cannot even claim it
MIN_K, MAX_K = 2, 16
TAG = b"mxpaillier/membership/v1"


def _check_values(n: int, values: Sequence[int]) -> List[int]:
    vals = [int(s) for s in values]
    if n < 3 or n % 2 == 0:
        raise ValueError("N must be odd")
    if n.bit_length() < MIN_BITS:
        raise ValueError(f"a modulus of at least {MIN_BITS} bits expected (every prime factor above 2^{E_BITS})")
    if not MIN_K <= len(vals) <= MAX_K:
        raise ValueError(f"a list of {MIN_K} .. {MAX_K} values expected")
    if len(set(vals)) != len(vals) or any(not 0 <= s < n for s in vals):
        raise ValueError("distinct values in [0, N) expected")
    return vals


def shape(n: int, k: int) -> dict:
    """Bit lengths and row widths of a proof (tools/member_model.py: shape)."""
    return _flows.member_shape(n, k)


def context(n: int, values: Sequence[int], label: bytes) -> bytes:
    """The 32 bytes that bind a proof to N, the list of values in its order and the caller's label."""
    fields = [_int_bytes(n), _int_bytes(len(values))] + [_int_bytes(s) for s in values] + [bytes(label)]
    return hashlib.sha256(_lp(TAG) + b"".join(_lp(f) for f in fields)).digest()


class MembershipProofs:
    """The proofs of a batch of ciphertexts: the rows of the k commitments a (``[count, k limbs(N^2)]``), of the k
    challenges e (``[count, 4 k]``) and of the k responses z (``[count, k limbs(N)]``), slot j in words j w .. (j + 1) w - 1
    — device tensors where they were made on the device, uint32 numpy rows where they arrived as ints.  ``unfit[r]`` marks
    a row whose integers did not fit the rows (its verdict is False)."""

    FIELDS = ("a", "e", "z")

    def __init__(self, a, e, z, k: int, unfit: Optional[List[bool]] = None) -> None:
        self.a, self.e, self.z, self.k = a, e, z, int(k)
        self.unfit = unfit

    def __len__(self) -> int:
        return int(self.a.shape[0])

    def rows(self) -> Tuple[Any, ...]:
        return tuple(getattr(self, f) for f in self.FIELDS)

    def to_ints(self) -> Tuple[List[List[int]], ...]:
        """(a, e, z), each a list of k ints per ciphertext — what travels to the verifier."""
        out = []
        for t in self.rows():
            h = np.ascontiguousarray(_host(t))
            flat = _limbs.unpack(h.reshape(h.shape[0] * self.k, -1)) if h.shape[0] else []
            out.append([flat[r * self.k : (r + 1) * self.k] for r in range(h.shape[0])])
        return tuple(out)

    @classmethod
    def from_ints(cls, a: Sequence[Sequence[int]], e: Sequence[Sequence[int]], z: Sequence[Sequence[int]], n: int, k: int) -> "MembershipProofs":
        """The proofs received as ints, as rows under (N, k).  A row with other than k entries in a, e or z, or with a
        value that is negative or does not fit its row, becomes a harmless row and a False verdict."""
        sh = shape(n, k)
        if len(a) != len(e) or len(a) != len(z):
            raise ValueError("one list of a, of e and of z per ciphertext expected")
        count = len(a)
        unfit = [False] * count
        packed = []
        for col, w in ((a, sh["limbs2"]), (e, sh["e_words"]), (z, sh["limbs_n"])):
            flat: List[int] = []
            for r, entry in enumerate(col):
                try:
                    entry = [int(v) for v in entry]
                except (TypeError, ValueError):
                    entry = []
                if len(entry) != k:
                    unfit[r], entry = True, [0] * k
                flat.extend(entry)
            rows, fits = _rows_of(flat, w)
            for r in range(count):
                unfit[r] = unfit[r] or not all(fits[r * k : (r + 1) * k])
            packed.append(rows.reshape(count, k * w))
        return cls(*packed, k, unfit)


def _check_statement(n: int, values: Sequence[int], label: bytes) -> Tuple[List[int], dict]:
    if not isinstance(label, (bytes, bytearray)):
        raise ValueError("the label must be bytes")
    vals = _check_values(n, values)
    return vals, shape(n, len(vals))


def _empty(sh: dict) -> MembershipProofs:
    k = sh["k"]
    return MembershipProofs(*(np.zeros((0, k * sh[w]), dtype=np.uint32) for w in ("limbs2", "e_words", "limbs_n")), k)


def prove_batch(n: int, values: Sequence[int], messages: Sequence[int], randomness: Sequence[int], label: bytes, rng: Any = None,
                ciphertexts: Optional[Sequence[int]] = None, engine: Any = None, draws: Any = None) -> MembershipProofs:
    """The proofs that c_r = (1 + n)^(m_r) (r_r)^n mod n^2 hold one of ``values``, for messages m_r IN ``values`` and the
    randomness r_r the ciphertexts were made with (``ciphertexts``: the c_r if the caller has them, else they are
    recomputed).  ``rng``: a ``DeviceRng`` (default: a fresh one); ``draws``: the two row sets, for tests.  ValueError —
    before any engine call — for a modulus below 260 bits, a list that is not 2 .. 16 distinct values in [0, N), lists
    of unequal lengths or a message that is not in ``values``: the honest algorithm has no proof for it."""
    n = int(n)
    vals, sh = _check_statement(n, values, label)
    msgs, rands = [int(m) for m in messages], [int(r) for r in randomness]
    if len(msgs) != len(rands) or (ciphertexts is not None and len(ciphertexts) != len(msgs)):
        raise ValueError("one randomness (and one ciphertext) per message expected")
    where = {s: j for j, s in enumerate(vals)}
    if any(m not in where for m in msgs):
        raise ValueError("every message must be one of the values")
    if not msgs:
        return _empty(sh)
    eng = _engine_of(engine)
    if ciphertexts is None:
        ciphertexts = eng.encrypt_batch(msgs, rands, n)
    if draws is None and rng is None:
        from .device_rng import DeviceRng

        rng = DeviceRng()
    count = len(msgs)
    cts_t = eng.to_device(_limbs.pack_reduced(list(ciphertexts), sh["limbs2"], n * n).reshape(count, sh["limbs2"]))
    index_t = eng.to_device(np.array([where[m] for m in msgs], dtype=np.uint32))
    r_t = eng.to_device(_limbs.pack_reduced(rands, sh["limbs_n"], n).reshape(count, sh["limbs_n"]))
    source = dict(draws=draws) if draws is not None else dict(rng=rng)
    return MembershipProofs(*eng.member_prove_t(cts_t, index_t, r_t, n, vals, context(n, vals, label), **source), sh["k"])


def encrypt_with_proof(n: int, values: Sequence[int], messages: Sequence[int], label: bytes, rng: Any = None,
                       engine: Any = None) -> Tuple[List[int], MembershipProofs]:
    """(ciphertexts, proofs): fresh encryptions of the messages (``Engine.encrypt_fresh_batch``, the randomness drawn
    on the device and kept for the proof) with their membership proofs.  Every message must be one of ``values``."""
    n = int(n)
    vals, _ = _check_statement(n, values, label)
    msgs = [int(m) for m in messages]
    if any(m not in vals for m in msgs):
        raise ValueError("every message must be one of the values")
    eng = _engine_of(engine)
    if rng is None:
        from .device_rng import DeviceRng

        rng = DeviceRng()
    if not msgs:
        return [], _empty(shape(n, len(vals)))
    cts, rands = eng.encrypt_fresh_batch(msgs, n, rng, return_randomness=True)
    return cts, prove_batch(n, vals, msgs, rands, label, rng=rng, ciphertexts=cts, engine=eng)


def verify_batch(n: int, values: Sequence[int], ciphertexts: Sequence[int], proofs: MembershipProofs, label: bytes,
                 engine: Any = None) -> List[bool]:
    """[is row r a valid proof that ciphertexts[r] holds one of ``values``] — never raises for a bad row: a value that is
    negative, zero (an a_j or a z_j), out of range or too long is a False.  ValueError — before any engine call — for a modulus below 260 bits,
    a bad list, proofs for another k or a number of proofs other than the number of ciphertexts."""
    n = int(n)
    vals, sh = _check_statement(n, values, label)
    count = len(ciphertexts)
    if not isinstance(proofs, MembershipProofs) or proofs.k != sh["k"] or len(proofs) != count:
        raise ValueError("one proof over the same number of values per ciphertext expected")
    if count == 0:
        return []
    eng = _engine_of(engine)
    c_rows, c_fit = _rows_of(ciphertexts, sh["limbs2"])
    if proofs.unfit is None and not isinstance(proofs.a, np.ndarray):
        rows = proofs.rows()
    else:
        rows = tuple(eng.to_device(np.asarray(t)) for t in proofs.rows())
    unfit = proofs.unfit or [False] * count
    verdict = eng.member_verify_t(eng.to_device(c_rows), *rows, n, vals, context(n, vals, label))
    got = [bool(x) for x in (verdict if isinstance(verdict, np.ndarray) else verdict.cpu().numpy())]
    return [g and f and not u for g, f, u in zip(got, c_fit, unfit)]
