"""Slot-packed plaintexts: many small values per Paillier plaintext, packed BEFORE encryption.

``packing.pack`` puts k values into one ciphertext after they were encrypted one by one, to make threshold decryption
cheaper.  A party that still holds its values in the clear does better: with g = N + 1 it packs

    P_j = (sum_{i < k} m_(j k + i) 2^(b i)) mod N,    k = packing.slots_per_ciphertext(N, b) = floor((bits(N) - 2) / b)

and encrypts P_j — k times fewer encryptions (63 times at key_length 2048 and b = 32).  Every linear operation of
``homomorphic`` (``scale``, ``add``, ``sum_groups``, ``linear_map``, ``matmul``, the bias) acts on the integer P_j and
therefore on all slots at once: a public weight multiplies every slot, a sum adds slot by slot.  One public W over a batch
of samples packed ACROSS slots (slot i = sample i, one ciphertext per feature) costs 1/k of the ciphertexts, of the kernel
time and of the partial decryptions.  The result already has the layout ``packing.unpack`` reads, so the ciphertext-level
``pack`` is not needed; a bias is encoded like a value, once per slot: ``encode([beta] * k, ...)``.  A convolution
(``homomorphic.conv2d`` / ``conv1d``) acts on all slots at once in the same way — k images, one per slot, under one public
kernel for the price of one; ``slot_bits_for(value_bits, weight_bits, terms=C * kh * kw, bias_bits=...)`` gives the head
room an output needs.

The layout is packing.py's and is decided there: value j k + i in bits [b i, b (i + 1)) of plaintext j, the last
plaintext holding the remaining values with its missing slots at 0; signed values in [-2^(b-1), 2^(b-1)), unsigned in
[0, 2^b).  The codec between an int64 tensor and the plaintext rows of the engine runs on the device
(csrc/mx_slots.hpp: ``Engine.slots_encode_t`` / ``slots_decode_t``) and takes signed slots of 1 .. 64 and unsigned slots of
1 .. 63 bits; wider slots stay with ``packing.unpack``.

What the code CANNOT check: ``encode`` checks its inputs only.  After homomorphic operations a slot whose value has left
[-2^(b-1), 2^(b-1)) (or [0, 2^b)) carries into its neighbours, and every slot above it decodes wrong WITHOUT any error.
Choose b with ``slot_bits_for`` from what the map can produce, not from what the inputs are.

``engine`` is injected for tests; the default is the process-wide HIP engine.
"""

from __future__ import annotations

from typing import Any, List, Optional, Sequence

import numpy as np

from . import limbs as _limbs
from .homomorphic import _engine, _values
from .packing import _as_ciphertexts, _scheme_modulus, slots_per_ciphertext

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def _slots(n: int, slot_bits: int, signed: bool) -> int:
    """k of the layout, after the limits of the int64 codec."""
    top = 64 if signed else 63
    if not 1 <= int(slot_bits) <= top:
        raise ValueError(f"the device codec takes {'signed' if signed else 'unsigned'} slots of 1 .. {top} bits (int64 values); "
                         "wider slots stay with packing.unpack")
    return slots_per_ciphertext(n, slot_bits)


def _int64_values(values: Any) -> Any:
    """Python ints, a numpy integer array or a torch tensor -> what ``Engine.slots_encode_t`` takes: a tensor as it is,
    anything else as a numpy int64 vector.  ValueError for an int outside int64, before anything is uploaded."""
    if hasattr(values, "is_cuda"):                                   # a torch tensor, host or device
        return values
    if isinstance(values, np.ndarray):
        if values.dtype.kind not in "iu":
            raise ValueError("an integer array expected")
        if values.dtype.kind == "u" and values.dtype.itemsize == 8 and values.size and int(values.max()) > INT64_MAX:
            raise ValueError("a value lies outside int64")
        return np.ascontiguousarray(values.reshape(-1), dtype=np.int64)
    vals = [int(v) for v in values]
    for idx, v in enumerate(vals):
        if not INT64_MIN <= v <= INT64_MAX:
            raise ValueError(f"value {idx} ({v}) lies outside int64")
    return np.array(vals, dtype=np.int64)


def _ints(eng: Any, rows_t: Any) -> List[int]:
    return _limbs.unpack(eng.to_host(rows_t))


def encode(values: Any, n: int, slot_bits: int, signed: bool = True, engine: Any = None) -> List[int]:
    """The packed plaintexts of ``values`` (a sequence of Python ints, a numpy integer array or a torch tensor):
    ceil(count / k) residues in [0, N).  ValueError, with the index of the first offender, for a value outside the slot
    range; for a Python int outside int64 before any upload."""
    n, b = int(n), int(slot_bits)
    _slots(n, b, signed)
    eng = _engine(engine)
    return _ints(eng, eng.slots_encode_t(_int64_values(values), n, b, signed))


def decode_t(rows_t: Any, n: int, slot_bits: int, count: int, signed: bool = True, engine: Any = None) -> Any:
    """Device rows of packed plaintexts (``[ceil(count / k), >= limbs(N)]``, e.g. what ``Engine.combine_t`` returns,
    ``packed=True`` included) -> the ``count`` slot values as an int64 tensor on the device.  Nothing is fetched."""
    n, b = int(n), int(slot_bits)
    _slots(n, b, signed)
    return _engine(engine).slots_decode_t(rows_t, n, b, int(count), signed)


def decode(plaintexts: Sequence[int], n: int, slot_bits: int, count: int, signed: bool = True, engine: Any = None) -> List[int]:
    """The ``count`` slot values of packed plaintexts (residues, one per packed ciphertext, in order):
    ``packing.unpack`` with the field extraction on the device."""
    n, b, count = int(n), int(slot_bits), int(count)
    k = _slots(n, b, signed)
    outputs = -(-count // k)
    if count < 0 or len(plaintexts) != outputs:
        raise ValueError(f"{count} values of {b} bits need {outputs} packed plaintexts, got {len(plaintexts)}")
    if not count:
        return []
    eng = _engine(engine)
    rows_t = eng.to_device(_limbs.pack_reduced(list(plaintexts), _limbs.limbs_for(n), n))
    return eng.slots_decode_t(rows_t, n, b, count, signed).tolist()


def encrypt_t(values: Any, randomizer: Any, slot_bits: int, signed: bool = True, exponents: Optional[Sequence[int]] = None) -> Any:
    """``encrypt`` that leaves its result on the device: ``[ceil(count / k), limbs(N^2)]`` ciphertext rows.  From the
    values to the rows nothing passes through Python ints: ``Engine.slots_encode_t`` -> ``fixed_base_encrypt_t`` with the
    randomiser's table and exponent rows (``randomizer.FastRandomizer``: the host draw, its device generator or
    explicit ``exponents``, chosen as ``FastRandomizer.encrypt`` chooses them) on the randomiser's engine."""
    n, b = randomizer.n, int(slot_bits)
    _slots(n, b, signed)
    eng = _engine(randomizer._engine)
    rows_t = eng.slots_encode_t(_int64_values(values), n, b, signed)
    exps = randomizer._exponents(exponents, int(rows_t.shape[0]))
    table = eng.fixed_base_table(n, randomizer.h_s, randomizer.exp_bits, randomizer.window)
    return eng.fixed_base_encrypt_t(table, eng.fixed_base_exponent_rows(exps, randomizer.exp_bits), rows_t)


def encrypt(values: Any, randomizer: Any, slot_bits: int, signed: bool = True, exponents: Optional[Sequence[int]] = None) -> List[int]:
    """ceil(count / k) ciphertexts ``(1 + P_j N) h_s^(a_j) mod N^2`` of the packed plaintexts P_j of ``values`` under the
    key of ``randomizer`` — ``FastRandomizer.encrypt(encode(values))`` without the plaintexts ever leaving the device."""
    return _ints(_engine(randomizer._engine), encrypt_t(values, randomizer, slot_bits, signed, exponents))


def slot_bits_for(value_bits: int, weight_bits: int = 0, terms: int = 1, bias_bits: int = 0) -> int:
    """The smallest signed slot that y = sum_{t < terms} w_t x_t + beta cannot overflow, for inputs x_t in
    [-2^(value_bits-1), 2^(value_bits-1)), public weights |w_t| < 2^weight_bits and a bias |beta| < 2^bias_bits
    (``weight_bits`` = 0: the terms are added unscaled, w_t = 1; ``bias_bits`` = 0: no bias).

    With X = 2^(value_bits-1), W = 2^weight_bits - 1 and B = 2^bias_bits - 1 (0 without a bias) the extremes are reached
    and are
        weight_bits > 0:   y in [-(terms W X + B), terms W X + B]      (w = -W, x = -X gives the upper one)
        weight_bits = 0:   y in [-(terms X + B), terms (X - 1) + B]
    and a signed slot of b bits holds [-2^(b-1), 2^(b-1) - 1], so b is the smallest width with -2^(b-1) <= min y and
    max y <= 2^(b-1) - 1.  With s = value_bits + weight_bits + ceil(log2 terms): terms W X < 2^(s-1) (and
    terms X <= 2^(s-1) on the negative side, terms (X - 1) < 2^(s-1) on the positive one, for unscaled terms), so without
    a bias b <= s; with a bias of bias_bits < s, B < 2^(s-1) and b <= s + 1.  A wider bias needs more, and gets it.
    Pure host code."""
    v, wb, t, bb = int(value_bits), int(weight_bits), int(terms), int(bias_bits)
    if v < 1 or wb < 0 or t < 1 or bb < 0:
        raise ValueError("value_bits >= 1, weight_bits >= 0, terms >= 1 and bias_bits >= 0 expected")
    x, bias = 1 << (v - 1), (1 << bb) - 1
    if wb:
        hi = t * ((1 << wb) - 1) * x + bias
        lo = -hi
    else:
        lo, hi = -(t * x + bias), t * (x - 1) + bias
    return max((-lo - 1).bit_length(), hi.bit_length()) + 1


def one_hot_values(n: int, slot_bits: int, k: int) -> List[int]:
    """[2^(slot_bits j) for j < k]: the plaintexts of a one-hot ballot over k choices in the slot layout — a vote for
    choice j is 1 in slot j and 0 elsewhere — as the public list of a membership proof (``membership.prove_batch``).
    A sum of up to 2^slot_bits - 1 such ballots (unsigned slots) decodes slot by slot into the tally.  ValueError
    unless 1 <= k <= ``packing.slots_per_ciphertext(n, slot_bits)``.  Pure host code."""
    n, b, k = int(n), int(slot_bits), int(k)
    cap = slots_per_ciphertext(n, b)
    if not 1 <= k <= cap:
        raise ValueError(f"1 .. {cap} slots of {b} bits fit a plaintext modulo a {n.bit_length()}-bit N, got {k}")
    return [1 << (b * j) for j in range(k)]


async def decrypt_sequence_slots(scheme: Any, ciphertexts: Sequence[Any], slot_bits: int, count: int, signed: bool = True,
                                 receivers: Optional[List[str]] = None, engine: Any = None) -> Optional[List[int]]:
    """Threshold-decrypt ciphertexts of slot-packed plaintexts (``encrypt``, or results of ``homomorphic`` operations on
    them) and decode the ``count`` slot values: ``packing.decrypt_sequence_packed`` without the ``pack`` step — the
    ciphertexts are packed already.  Runs ``scheme._decrypt_sequence_raw`` (``receivers`` as there) on them as they are;
    returns None when this party is not a receiver.  Every party calls with the same sequence in the same order."""
    cts = list(ciphertexts)
    self_receive = receivers is None or "self" in receivers
    if not cts:
        return decode([], _scheme_modulus(scheme), slot_bits, count, signed, engine) if self_receive else None
    proto = next((c for c in cts if not isinstance(c, int)), None)
    n = None if proto is not None else _scheme_modulus(scheme)
    vals, n = _values(cts, n)
    objs = cts if all(not isinstance(c, int) for c in cts) else _as_ciphertexts(vals, proto, n)
    res = await scheme._decrypt_sequence_raw(objs, receivers)
    if res is None:
        return None
    return decode([r.value for r in res], n, slot_bits, count, signed, engine)
