"""The product of two ENCRYPTED values under a dealt threshold key: from c_a = Enc(a) and c_b = Enc(b), a ciphertext of
a b mod N — which Paillier does not give for free — by the protocol of Cramer-Damgard-Nielsen 2001 over ``threshold.py``
(a dealt key, partial decryptions that carry proofs, ``decrypt_verified``) and ``multiplication.py`` (the proof of
correct multiplication).  A square for an encrypted variance and the dot product of two encrypted vectors are this,
row by row, followed by the homomorphic sum.

    mask      party i draws d_i in [0, N) and publishes D_i = Enc(d_i) and E_i = c_b^(d_i) gamma_i^N with the proof that
              E_i holds d_i b for the d_i inside D_i                                              (``mask_batch``)
    masked    everybody verifies every contribution; c_m = c_a prod D_i over the ACCEPTED parties   (``masked_batch``)
    open      the parties open c_m with ``partial_decrypt_batch(prove=True)`` / ``decrypt_verified``: m = a + sum d_i mod N
    finish    c_ab = c_b^m (prod E_i)^-1 mod N^2 = Enc((a + sum d_i) b - sum d_i b)                  (``finish_batch``)

What this is and is not — read before use:

  * m is PUBLIC and uniform as soon as ONE accepted party drew its d_i honestly and kept it: ``masked_batch`` needs
    threshold + 1 accepted contributions, one more than the parties an adversary controls, so one of them is honest.
    A party that sent a contribution knows nothing it must keep afterwards: d_i, its randomness and gamma_i are dropped
    once the proofs are made.
  * A contribution whose proofs do not ALL verify is left out whole and its sender is named; the product is computed
    from the others.  The opening names its own cheaters (``decrypt_verified``).
  * Every contribution is bound to the key, the party and the caller's ``label`` — the session: a contribution does not
    verify for another party, label or c_b.  A label must not be used for two products.
  * The result is NOT FRESH beyond the gamma_i of the accepted parties: re-randomise it before it leaves the group if
    that matters.  c_a and c_b are taken as they are: whether they are valid ciphertexts of values of the right size is
    their senders' business (``range_proof``, ``membership``).
  * The key must be a proper one — ``multiplication`` refuses N below 260 bits — and dealt (``threshold.deal``).
  * ``multiply`` and ``square`` run ALL parties in one process, as ``decrypt_verified`` does for the tests and examples:
    a deployment runs ``mask_batch`` and ``partial_decrypt_batch`` at each party and the rest at anybody.
"""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import limbs as _limbs
from . import multiplication
from .multiplication import MultiplicationProofs
from .range_proof import _host
from .threshold import ThresholdKeyShare, ThresholdPublicKey


class MaskContribution:
    """What party ``index`` publishes for a batch of products: D = Enc(d_i), E = c_b^(d_i) gamma_i^N and the proofs."""

    def __init__(self, index: int, D: Sequence[int], E: Sequence[int], proofs: MultiplicationProofs) -> None:
        self.index, self.D, self.E, self.proofs = int(index), list(D), list(E), proofs

    def __len__(self) -> int:
        return len(self.D)


def party_label(pk: ThresholdPublicKey, index: int, label: bytes) -> bytes:
    """The label of party `index`'s proofs: the caller's label, the party and the size of the group."""
    pk.verification_key(index)          # (an unknown index is the caller's mistake: ValueError)
    if not isinstance(label, (bytes, bytearray)):
        raise ValueError("the label must be bytes")
    return b"secure_product/%d/%d/%d/" % (index, pk.parties, pk.threshold) + bytes(label)


def _check_cts(pk: ThresholdPublicKey, *cols: Sequence[int]) -> int:
    count = len(cols[0])
    if any(len(c) != count for c in cols):
        raise ValueError("columns of one length expected")
    if any(not 0 < int(v) < pk.n_square for c in cols for v in c):
        raise ValueError("ciphertexts in (0, N^2) expected")
    return count


def mask_batch(pk: ThresholdPublicKey, index: int, c_b: Sequence[int], label: bytes, rng: Any = None, engine: Any = None) -> MaskContribution:
    """Party `index`'s contribution to the products with the ciphertexts ``c_b``: a mask d_i per row drawn on the device,
    D_i = Enc(d_i), E_i = c_b^(d_i) gamma_i^N and the multiplication proofs (``multiplication.multiply_with_proof``).
    Nothing secret is kept."""
    plabel = party_label(pk, index, label)
    _check_cts(pk, c_b)
    eng = pk._eng(engine)
    rng = multiplication._default_rng(rng)
    sh = multiplication.shape(pk.n)
    multiplication._check_modulus(pk.n)
    if not len(c_b):
        return MaskContribution(index, [], [], multiplication._empty(sh))
    masks = [v % pk.n for v in _limbs.unpack(np.ascontiguousarray(_host(rng.rows_t(eng, len(c_b), sh["draw_bits"], sh["limbs2"]))))]
    D, E, proofs = multiplication.multiply_with_proof(pk.n, masks, c_b, plabel, rng=rng, engine=eng)
    return MaskContribution(index, D, E, proofs)


def _product_rows(pk: ThresholdPublicKey, eng: Any, first: Sequence[int], first_weights: Sequence[int], others: Sequence[Sequence[int]],
                  sign: int) -> List[int]:
    """[first[r]^(first_weights[r]) prod_k others[k][r]^sign mod N^2]: ONE signed multi-exponentiation."""
    count = len(first)
    flat = [int(v) for v in first] + [int(v) for col in others for v in col]
    inputs_t = eng.to_device(_limbs.pack_reduced(flat, pk.limbs2, pk.n_square).reshape(len(flat), pk.limbs2))
    weights = [{r: int(first_weights[r]), **{(k + 1) * count + r: sign for k in range(len(others))}} for r in range(count)]
    return _limbs.unpack(np.ascontiguousarray(_host(eng.multiexp_nsquare_t(inputs_t, weights, pk.n))))


def masked_batch(pk: ThresholdPublicKey, c_a: Sequence[int], c_b: Sequence[int], contributions: Sequence[MaskContribution], label: bytes,
                 engine: Any = None) -> Tuple[List[int], List[MaskContribution], List[int]]:
    """``(c_m, accepted, cheaters)``: every contribution verified against ``c_b`` under its party's label, the parties
    with any False row (or a contribution of another length, or a second one) named in ``cheaters``, and
    c_m = c_a prod D_i over the ``accepted`` ones, in index order.  ValueError, naming the cheaters, unless at least
    threshold + 1 are accepted; ValueError for an unknown party."""
    count = _check_cts(pk, c_a, c_b)
    for c in contributions:
        party_label(pk, c.index, label)
    eng = pk._eng(engine)
    accepted: Dict[int, MaskContribution] = {}
    cheaters: List[int] = []
    for c in sorted(contributions, key=lambda c: c.index):
        good = (c.index not in accepted and c.index not in cheaters and len(c.D) == len(c.E) == len(c.proofs) == count
                and all(multiplication.verify_batch(pk.n, c.D, c_b, c.E, c.proofs, party_label(pk, c.index, label), engine=eng)))
        if good:
            accepted[c.index] = c
        elif c.index not in cheaters:
            accepted.pop(c.index, None)
            cheaters.append(c.index)
    if len(accepted) < pk.threshold + 1:
        raise ValueError(f"only {len(accepted)} of the needed {pk.threshold + 1} parties sent valid contributions; invalid: {cheaters}")
    kept = [accepted[i] for i in sorted(accepted)]
    if count == 0:
        return [], kept, cheaters
    return _product_rows(pk, eng, c_a, [1] * count, [c.D for c in kept], 1), kept, cheaters


def finish_batch(pk: ThresholdPublicKey, c_b: Sequence[int], m: Sequence[int], accepted: Sequence[MaskContribution], engine: Any = None) -> List[int]:
    """c_ab = c_b^m (prod E_i)^-1 mod N^2 over the accepted contributions, for the opened m = a + sum d_i mod N: the
    ciphertexts of a b.  ValueError for a row whose prod E_i has no inverse.  Not fresh beyond the gamma_i."""
    count = _check_cts(pk, c_b)
    if len(m) != count or any(len(c.E) != count for c in accepted) or not accepted:
        raise ValueError("one m and one E of every accepted party per c_b expected")
    if any(not 0 <= int(v) < pk.n for v in m):
        raise ValueError("every m must lie in [0, N)")
    if count == 0:
        return []
    return _product_rows(pk, pk._eng(engine), c_b, m, [c.E for c in accepted], -1)


def multiply(pk: ThresholdPublicKey, shares: Sequence[ThresholdKeyShare], c_a: Sequence[int], c_b: Sequence[int], label: bytes,
             rng: Any = None, engine: Any = None, contributions: Optional[Dict[int, MaskContribution]] = None
             ) -> Tuple[List[int], List[int]]:
    """``(c_ab, cheaters)`` with ALL parties in one process: every share's party masks (``contributions``: what some
    parties sent instead, by index — for tests), the contributions are verified, c_m is opened by the accepted parties
    with proofs, and the product is finished.  For tests and examples, as ``decrypt_verified`` is."""
    eng = pk._eng(engine)
    sent = [(contributions or {}).get(s.index) or mask_batch(pk, s.index, c_b, label, rng=rng, engine=eng) for s in shares]
    c_m, accepted, cheaters = masked_batch(pk, c_a, c_b, sent, label, engine=eng)
    openers = {c.index for c in accepted}
    partials = {s.index: s.partial_decrypt_batch(c_m, prove=True, rng=rng, engine=eng) for s in shares if s.index in openers}
    m, bad = pk.decrypt_verified(c_m, partials, engine=eng)
    return finish_batch(pk, c_b, m, accepted, engine=eng), sorted(set(cheaters) | set(bad))


def square(pk: ThresholdPublicKey, shares: Sequence[ThresholdKeyShare], c: Sequence[int], label: bytes, rng: Any = None,
           engine: Any = None) -> Tuple[List[int], List[int]]:
    """``multiply`` of the ciphertexts with themselves: Enc(x^2), for an encrypted variance."""
    return multiply(pk, shares, c, c, label, rng=rng, engine=engine)
