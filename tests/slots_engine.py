"""A Python-int double of the engine methods slots.py drives: ``slots_encode_t`` / ``slots_decode_t`` computed from the
layout's definition on Python ints, the row transport (``to_device`` / ``to_host``) as the identity on numpy rows, and the
three fixed-base calls of ``slots.encrypt`` over ``pow``.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

import numpy as np

from protocols.distributed_keygen_amd import limbs
from protocols.distributed_keygen_amd.packing import slots_per_ciphertext


class SlotsEngine:
    def __init__(self):
        self.calls = []

    # ---- transport: "device" rows are numpy uint32 rows
    def to_device(self, rows):
        return np.ascontiguousarray(rows, dtype="<u4")

    @staticmethod
    def to_host(rows_t):
        return np.ascontiguousarray(rows_t, dtype="<u4")

    # ---- the codec, from the definition
    def slots_encode_t(self, values_t, n, slot_bits, signed=True):
        vals = [int(v) for v in np.asarray(values_t).reshape(-1)]
        self.calls.append(("encode", len(vals), slot_bits, signed))
        k = slots_per_ciphertext(n, slot_bits)
        lo, hi = (-(1 << (slot_bits - 1)), 1 << (slot_bits - 1)) if signed else (0, 1 << slot_bits)
        for idx, v in enumerate(vals):
            if not lo <= v < hi:
                raise ValueError(f"value {idx} ({v}) does not fit a slot of {slot_bits} bits")
        out = [sum(m << (slot_bits * i) for i, m in enumerate(vals[j : j + k])) % n for j in range(0, len(vals), k)]
        return limbs.pack(out, limbs.limbs_for(n))

    def slots_decode_t(self, rows_t, n, slot_bits, count, signed=True):
        self.calls.append(("decode", count, slot_bits, signed))
        k = slots_per_ciphertext(n, slot_bits)
        if rows_t.shape[0] != -(-count // k):
            raise ValueError("wrong number of plaintext rows")
        if rows_t.shape[1] < limbs.limbs_for(n):
            raise ValueError("plaintext rows narrower than N")
        out = []
        for v in limbs.unpack(rows_t[:, : limbs.limbs_for(n)]):
            s = v - n if signed and v > n // 2 else v
            if signed:
                s += sum(1 << (slot_bits * i + slot_bits - 1) for i in range(k))
            for i in range(k):
                f = (s >> (slot_bits * i)) & ((1 << slot_bits) - 1)
                out.append(f - (1 << (slot_bits - 1)) if signed else f)
        return np.array(out[:count], dtype=np.int64)

    # ---- fixed-base encryption over pow
    def fixed_base_table(self, n, base, exp_bits, window=0):
        self.calls.append(("table", exp_bits, window))
        return (n, base % (n * n), exp_bits)

    def fixed_base_exponent_rows(self, exponents, exp_bits):
        if isinstance(exponents, np.ndarray):
            vals = limbs.unpack(exponents)
        else:
            vals = [int(e) for e in exponents]
        assert all(0 <= e < 1 << exp_bits for e in vals)
        return vals

    def fixed_base_encrypt_t(self, table, exps_t, messages_t):
        n, base, _ = table
        n2 = n * n
        msgs = limbs.unpack(messages_t)
        assert len(msgs) == len(exps_t)
        self.calls.append(("encrypt", len(msgs)))
        return limbs.pack([(1 + m * n) * pow(base, e, n2) % n2 for m, e in zip(msgs, exps_t)], limbs.limbs_for(n2))
