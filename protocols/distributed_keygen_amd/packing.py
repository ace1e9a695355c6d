"""Packed threshold decryption: many small plaintexts per Paillier ciphertext.

With g = N + 1 the product

    C = prod_{i < k} c_i^(2^(b i))  mod N^2   encrypts   S = sum_{i < k} m_i 2^(b i)

so ONE threshold decryption of C returns k values of b bits: every party runs one partial decryption instead of k and
sends one instead of k.  Decrypting C reveals the slot values and nothing else, as long as every value fits its slot.
The layout is decided here and nowhere else:

  * ``slots_per_ciphertext(n, b)`` = k = floor((bits(N) - 2) / b): a function of N and b only.  Every party must arrive
    at bit-identical packed ciphertexts, so nothing device-dependent (CU count, launch shape, timing) enters it;
  * input order is slot order: value ``j k + i`` goes to bits [b i, b (i + 1)) of output j, the last output holding
    the remaining ``count - (outputs - 1) k`` values;
  * signed slots hold values in [-2^(b-1), 2^(b-1)): S is read as ``v - N`` when the plaintext v exceeds N // 2, and
    each field is offset by 2^(b-1) before it is extracted; unsigned slots hold values in [0, 2^b).  Since
    k b <= bits(N) - 2, |S| < N / 2 and both readings are unambiguous.

Preconditions the code cannot check:

  * every value must lie in its slot's range, or its neighbours come out wrong WITHOUT any error;
  * every party must call ``decrypt_sequence_packed`` with the same sequence, in the same order, with the same
    ``slot_bits`` and ``signed`` (they then compute bit-identical packed ciphertexts and their partial decryptions
    combine).

The packing runs on the GPU (``Engine.ciphertext_pack_batch``, csrc/mx_pack_n2.hpp); ``engine`` is injected for tests,
the default is the process-wide HIP engine.  Decoding the slot integers further (a fixed-point encoding of the
scheme, for example) stays with the caller.
"""

from __future__ import annotations

from typing import Any, List, Optional, Sequence

import numpy as np

from .homomorphic import _engine, _values

NUMPY_MAX_SLOT_BITS = 64          # fields of up to 64 bits are unpacked as uint64 arrays


def slots_per_ciphertext(n: int, slot_bits: int) -> int:
    """k = floor((bits(N) - 2) / slot_bits): values of ``slot_bits`` bits one ciphertext modulo N^2 carries.  ValueError
    when not even one fits."""
    n, b = int(n), int(slot_bits)
    if b < 1:
        raise ValueError("slot_bits must be at least 1")
    k = (n.bit_length() - 2) // b
    if k < 1:
        raise ValueError(f"a slot of {b} bits does not fit a plaintext modulo a {n.bit_length()}-bit N")
    return k


def pack(cts: Sequence[Any], slot_bits: int, n: Optional[int] = None, engine: Any = None, randomizer: Any = None) -> List[int]:
    """[prod_{i < k} c_(j k + i)^(2^(b i)) mod N^2 for every output j]: ceil(len(cts) / k) ciphertexts, k =
    ``slots_per_ciphertext(n, slot_bits)``.  Ciphertexts are ints or objects with ``get_value()`` (read once per distinct
    object; ``n`` then defaults to ``.scheme.public_key.n``).  Returns canonical residues, not fresh ciphertexts — unless
    a ``randomizer`` (randomizer.FastRandomizer of the same N) is given: the packed rows are then multiplied by powers of
    its fixed base on the device before they are fetched.  Parties that must agree on the packed ciphertexts bit for bit
    (``decrypt_sequence_packed``) pack WITHOUT one."""
    vals, n = _values(list(cts), n)
    k = slots_per_ciphertext(n, slot_bits)
    if not vals:
        return []
    from .homomorphic import _fresh

    return _engine(engine).ciphertext_pack_batch(vals, n, int(slot_bits), k, **_fresh(randomizer, n, -(-len(vals) // k)))


def _offset(slot_bits: int, k: int) -> int:
    """2^(b-1) * sum_{i < k} 2^(b i): adds 2^(b-1) to every field."""
    return ((1 << (slot_bits * k)) - 1) // ((1 << slot_bits) - 1) << (slot_bits - 1)


def _fields_plain(totals: Sequence[int], slot_bits: int, k: int) -> List[int]:
    mask = (1 << slot_bits) - 1
    return [(t >> (slot_bits * i)) & mask for t in totals for i in range(k)]


def _fields_numpy(totals: Sequence[int], slot_bits: int, k: int) -> np.ndarray:
    """[outputs * k] uint64 fields of ``slot_bits`` <= 64 bits: the little-endian bytes of every total, each field read
    as the 8 bytes at its first byte plus the ninth, shifted — no per-slot Python loop."""
    nbytes = (slot_bits * k + 7) // 8
    width = nbytes + 16                                    # room for the 9-byte read of the last field
    buf = np.frombuffer(b"".join(t.to_bytes(width, "little") for t in totals), dtype=np.uint8).reshape(len(totals), width)
    bit = np.arange(k, dtype=np.int64) * slot_bits
    first, shift = bit >> 3, (bit & 7).astype(np.uint64)
    lo = np.ascontiguousarray(buf[:, first[:, None] + np.arange(8)]).view("<u8")[..., 0]   # [outputs, k]
    hi = buf[:, first + 8].astype(np.uint64)
    with np.errstate(over="ignore"):
        up = np.where(shift == 0, np.uint64(0), hi << ((np.uint64(64) - shift) % np.uint64(64)))
        field = (lo >> shift) | up
        if slot_bits < 64:
            field &= np.uint64((1 << slot_bits) - 1)
    return field.reshape(-1)


def unpack(plaintexts: Sequence[int], slot_bits: int, count: int, n: int, signed: bool = True,
           use_numpy: Optional[bool] = None) -> List[int]:
    """The ``count`` slot values of packed plaintexts (residues v in [0, N), one per packed ciphertext, in order).

    ``signed``: S = v - N when v > N // 2, values in [-2^(b-1), 2^(b-1)); otherwise values in [0, 2^b).  The last
    plaintext holds ``count - (outputs - 1) k`` values.  Fields of up to 64 bits are extracted with numpy
    (``use_numpy`` forces either path, for tests)."""
    n, b, count = int(n), int(slot_bits), int(count)
    k = slots_per_ciphertext(n, b)
    outputs = -(-count // k)
    if count < 0 or len(plaintexts) != outputs:
        raise ValueError(f"{count} values of {b} bits need {outputs} packed plaintexts, got {len(plaintexts)}")
    if not count:
        return []
    half = n // 2
    mask = (1 << (b * k)) - 1            # (values outside their slots' range come out wrong, but both paths agree)
    if signed:
        off = _offset(b, k)
        totals = []
        for v in plaintexts:
            v = int(v) % n
            totals.append(((v - n if v > half else v) + off) & mask)
    else:
        totals = [int(v) % n & mask for v in plaintexts]
    if use_numpy is None:
        use_numpy = b <= NUMPY_MAX_SLOT_BITS
    if use_numpy:
        if b > NUMPY_MAX_SLOT_BITS:
            raise ValueError(f"the numpy path takes slots of at most {NUMPY_MAX_SLOT_BITS} bits")
        field = _fields_numpy(totals, b, k)[:count]
        if signed:          # field - 2^(b-1), wrapping in 64 bits: the result fits int64
            return (field - np.uint64(1 << (b - 1))).view(np.int64).tolist()
        return field.tolist()
    fields = _fields_plain(totals, b, k)[:count]
    if signed:
        return [f - (1 << (b - 1)) for f in fields]
    return fields


def _scheme_modulus(scheme: Any) -> Optional[int]:
    pk = getattr(scheme, "public_key", None)
    if pk is not None and getattr(pk, "n", None) is not None:
        return int(pk.n)
    key = getattr(scheme, "secret_key", None)
    return int(key.n) if key is not None and getattr(key, "n", None) is not None else None


def _as_ciphertexts(values: Sequence[int], proto: Any, n: int) -> List[Any]:
    """Ciphertext objects ``scheme._decrypt_sequence_raw`` accepts: ``type(c)(value, c.scheme)`` of the first ciphertext
    object (the constructor shape of the reference's and the stand-in's class), otherwise shared_key.PlainCiphertext."""
    if proto is not None:
        cls, sch = type(proto), getattr(proto, "scheme", None)
        try:
            return [cls(v, sch) for v in values]
        except TypeError:
            pass
    from .shared_key import PlainCiphertext

    return [PlainCiphertext(v, n) for v in values]


async def decrypt_sequence_packed(scheme: Any, ciphertexts: Sequence[Any], slot_bits: int, signed: bool = True,
                                  receivers: Optional[List[str]] = None, engine: Any = None) -> Optional[List[int]]:
    """Threshold-decrypt many small values with ceil(count / k) decryptions instead of count: pack the ciphertexts
    (``pack``), run ``scheme._decrypt_sequence_raw`` on the packed ones (``receivers`` as there) and unpack the
    plaintexts.  Returns the ``count`` slot integers, or None when this party is not a receiver (as the reference).

    ``scheme`` is this party's DistributedPaillier (the reference's, the stand-in's, patched by ``patch.install()`` or
    not).  Preconditions (module docstring): every value lies in its slot's range — otherwise its neighbours come out
    wrong without any error; every party calls with the same sequence, in the same order, with the same ``slot_bits``
    and ``signed``."""
    cts = list(ciphertexts)
    self_receive = receivers is None or "self" in receivers
    if not cts:
        return [] if self_receive else None
    proto = next((c for c in cts if not isinstance(c, int)), None)
    n = None if proto is not None else _scheme_modulus(scheme)
    vals, n = _values(cts, n)
    packed = pack(vals, slot_bits, n=n, engine=engine)
    res = await scheme._decrypt_sequence_raw(_as_ciphertexts(packed, proto, n), receivers)
    if res is None:
        return None
    return unpack([r.value for r in res], slot_bits, len(cts), n, signed=signed)
