"""A Python-int double of the engine methods primes.py and the key generation of private_key.py drive — ``mr_split_t`` /
``miller_rabin_t`` / ``miller_rabin_base2_t`` / ``probable_prime_t`` / ``prime_search_t`` on numpy rows — computed by the
model of the kernels (tools/mr_model.py) with the random rows of a ``FakeRng`` (or anything else with ``rows_t``).  It
extends the encryption's double, so a key generated over it encrypts and decrypts.  Lives in tests/ only; the product
never imports it."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

from crt_enc_engine import CrtEncEngine, FakeRng  # noqa: F401

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import chacha_model  # noqa: E402
import mr_model  # noqa: E402

from protocols.distributed_keygen_amd import limbs, primes  # noqa: E402


class MrEngine(CrtEncEngine):
    @staticmethod
    def to_device(rows):
        return np.ascontiguousarray(rows, dtype=np.uint32)

    @staticmethod
    def to_host(rows_t):
        return rows_t

    def chacha20_rows_t(self, key, nonce, counter0, count, bits, row_words=None):
        """What a real ``DeviceRng`` asks of its engine, from the model of the kernel."""
        words = row_words or (bits + 31) // 32
        return np.array(chacha_model.rows_words(list(key), list(nonce), counter0, count, bits, words), dtype=np.uint32).reshape(count, words)

    def _draw(self, rng):
        return lambda count, bits, row_words: limbs.unpack(rng.rows_t(self, count, bits, row_words))

    def _candidates(self, cands_t, bits, above=3):
        if cands_t.ndim != 2:
            raise ValueError("candidates must be rows [S, limbs]")
        bits = 32 * cands_t.shape[1] if bits is None else int(bits)
        vals = limbs.unpack(cands_t)
        if any(n % 2 == 0 or n < above or n.bit_length() > bits for n in vals):
            raise ValueError(f"candidates must be odd, at least {above} and of at most `bits` bits")
        return vals, bits

    def mr_split_t(self, cands_t, bits=None):
        vals, _ = self._candidates(cands_t, bits)
        self.calls.append(("mr_split", len(vals)))
        parts = [mr_model.split(n) for n in vals]
        return limbs.pack([d for d, _ in parts], cands_t.shape[1]), np.array([s for _, s in parts], dtype=np.int32)

    def miller_rabin_t(self, cands_t, bases_t, group_size, out_t=None, bits=None):
        if int(group_size) < 1:
            raise ValueError("group_size must be at least 1")
        vals, _ = self._candidates(cands_t, bits)
        if tuple(bases_t.shape) != (len(vals) * group_size, cands_t.shape[1]):
            raise ValueError("bases_t must hold group_size rows per candidate")
        self.calls.append(("miller_rabin", len(vals), group_size))
        bases = limbs.unpack(bases_t)
        return np.array([mr_model.round_passes(vals[k // group_size], b) for k, b in enumerate(bases)], dtype=np.uint8)

    def miller_rabin_base2_t(self, cands_t, bits=None, out_t=None):
        vals, bits = self._candidates(cands_t, bits)
        self.calls.append(("base2", len(vals)))
        return np.array([mr_model.base2(n, bits) for n in vals], dtype=np.uint8)

    def probable_prime_t(self, cands_t, bits, rounds, rng):
        if int(rounds) < 1:
            raise ValueError("rounds must be at least 1")
        vals, bits = self._candidates(cands_t, bits, above=primes.SIEVE_BOUND)
        self.calls.append(("probable_prime", len(vals), rounds))
        return np.array(mr_model.probable_prime(vals, bits, int(rounds), self._draw(rng)), dtype=np.uint8)

    def prime_search_t(self, count, bits, rng, rounds=64, batch=None):
        if count < 0 or bits < 16 or rounds < 1:
            raise ValueError("count >= 0, bits >= 16 and rounds >= 1 expected")
        batch = primes.default_batch(count, bits) if batch is None else int(batch)
        self.calls.append(("prime_search", count, bits, batch))
        found, _ = mr_model.prime_search(count, bits, self._draw(rng), rounds, batch)
        return limbs.pack(found, limbs.limbs_for_bits(bits))
