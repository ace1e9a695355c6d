"""Pure-Python engine doubles for the tests of the device random-row generator: the int-level fixed-base functions and
the `fixed_base` keyword over Python ints, plus the generator's raw call computed by tools/chacha_model.py, every call
recorded.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

import random
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import chacha_model as cm  # noqa: E402


def exponent_ints(exps):
    """Exponent rows (uint32 little-endian words) or ints -> ints."""
    if isinstance(exps, np.ndarray):
        return [int.from_bytes(np.ascontiguousarray(row, dtype="<u4").tobytes(), "little") for row in exps]
    return [int(e) for e in exps]


class ByteSource:
    """A deterministic stand-in for os.urandom that records what was asked of it."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.asked = []

    def __call__(self, nbytes):
        self.asked.append(nbytes)
        return self.rng.randbytes(nbytes)


class DeviceRows(np.ndarray):
    """What the recording engine hands out as "device" rows: tells them from host arrays (FastRandomizer.draw)."""


class RecordingEngine:
    """Engine.fixed_base_*_batch, the two ciphertext functions the tests drive through homomorphic.linear_map and
    packing.pack (with the `fixed_base` keyword) and chacha20_rows_t, over Python ints.  ``calls`` records ("power" |
    "encrypt" | "randomize", count, exp_bits, window) and ("chacha", key words, nonce words, counter0, count, bits,
    row_words); ``exponent_kinds`` the kind of every exponent operand that reached a fixed_base_* call: "device" (rows
    of the generator), "host" (a numpy array to upload) or "ints"."""

    def __init__(self):
        self.calls = []
        self.exponent_kinds = []

    def chacha20_rows_t(self, key, nonce, counter0, count, bits, row_words=None):
        row_words = -(-bits // 32) if row_words is None else row_words
        self.calls.append(("chacha", tuple(key), tuple(nonce), counter0, count, bits, row_words))
        rows = cm.rows_words(list(key), list(nonce), counter0, count, bits, row_words)
        return np.array(rows, dtype="<u4").reshape(count, row_words).view(DeviceRows)

    def chacha_calls(self):
        return [c for c in self.calls if c[0] == "chacha"]

    def _powers(self, exps, n, base, exp_bits):
        self.exponent_kinds.append("device" if isinstance(exps, DeviceRows) else "host" if isinstance(exps, np.ndarray) else "ints")
        vals = exponent_ints(exps)
        assert all(0 <= e < 1 << exp_bits for e in vals)
        return [pow(base, e, n * n) for e in vals]

    def fixed_base_power_batch(self, exponents, n, base, exp_bits, window=0):
        self.calls.append(("power", len(exponents), exp_bits, window))
        return self._powers(exponents, n, base, exp_bits)

    def fixed_base_encrypt_batch(self, messages, exponents, n, base, exp_bits, window=0):
        self.calls.append(("encrypt", len(messages), exp_bits, window))
        return [(1 + (m % n) * n) * h % (n * n) for m, h in zip(messages, self._powers(exponents, n, base, exp_bits))]

    def fixed_base_randomize_batch(self, ciphertexts, exponents, n, base, exp_bits, window=0):
        self.calls.append(("randomize", len(ciphertexts), exp_bits, window))
        return [c % (n * n) * h % (n * n) for c, h in zip(ciphertexts, self._powers(exponents, n, base, exp_bits))]

    def _fresh(self, values, fixed_base):
        if fixed_base is None:
            return values
        n, base, exp_bits, window, exps = fixed_base
        assert len(exps) == len(values)
        return self.fixed_base_randomize_batch(values, exps, n, base, exp_bits, window)

    def ciphertext_linear_map_batch(self, cts, weights, n, bias=None, fixed_base=None):
        n2 = n * n
        out = []
        for j, row in enumerate(weights):
            items = row.items() if isinstance(row, dict) else enumerate(row)
            acc = 1 + ((bias[j] % n) * n if bias is not None else 0)
            for i, w in items:
                acc = acc * pow(cts[i], w, n2) % n2
            out.append(acc % n2)
        return self._fresh(out, fixed_base)

    def ciphertext_pack_batch(self, cts, n, slot_bits, slots, fixed_base=None):
        n2 = n * n
        out = []
        for j in range(0, len(cts), slots):
            acc = 1
            for i, c in enumerate(cts[j : j + slots]):
                acc = acc * pow(c % n2, 1 << (slot_bits * i), n2) % n2
            out.append(acc)
        return self._fresh(out, fixed_base)
