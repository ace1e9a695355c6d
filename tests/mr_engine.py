"""A Python-int double of the engine PRIMITIVES primes.py and the key generation of private_key.py drive —
``chacha20_rows_t`` / ``sieve_t`` / ``mr_split_t`` / ``miller_rabin_t`` / ``miller_rabin_base2_t`` / ``generator_shares_t``
— on CPU ``int32`` tensors, each from the model of its kernel (tools/mr_model.py, tools/chacha_model.py), with the random
rows of a ``FakeRng`` or of a real ``DeviceRng``.  ``probable_prime_t`` and ``prime_search_t`` are NOT written again
here: they are the shipped compositions of ``PrivateKeyFlows`` — range check, compaction, the one draw per batch, the loop
of the search — recorded; tools/mr_model.py's pipeline is the oracle the tests compare them with.  It extends the
encryption's double, so a key generated over it encrypts and decrypts.  Lives in tests/ only; the product never imports
it."""

from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import torch

from crt_enc_engine import CrtEncEngine, FakeRng, _is_pair  # noqa: F401
from crt_engine import _flags_t, _ints, _rows_t

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import chacha_model  # noqa: E402
import mr_model  # noqa: E402

from protocols.distributed_keygen_amd import primes  # noqa: E402

_PRODUCTS = {}


def _product(prime_list):
    key = tuple(prime_list)
    if key not in _PRODUCTS:
        _PRODUCTS[key] = math.prod(key)
    return _PRODUCTS[key]


def _drawn_batch(default_batch, count, bits, batch):
    """The rows per draw of an accepted search, for its record (a search for nothing draws nothing)."""
    return int(batch) if batch is not None else default_batch(count, bits) if count else 0


class MrEngine(CrtEncEngine):
    def chacha20_rows_t(self, key, nonce, counter0, count, bits, row_words=None):
        """What a real ``DeviceRng`` asks of its engine, from the model of the kernel."""
        words = row_words or (bits + 31) // 32
        rows = np.array(chacha_model.rows_words(list(key), list(nonce), counter0, count, bits, words), dtype=np.uint32)
        return self.to_device(rows.reshape(count, words))

    # ---- the primitives of the prime search, in ints
    def sieve_t(self, cands_t, prime_list, out_t=None):
        self.calls.append(("sieve", len(cands_t)))
        product = _product(prime_list)
        return _flags_t(math.gcd(n, product) != 1 for n in _ints(cands_t))

    def mr_split_t(self, cands_t, bits=None, _checked=False):
        rows, words, _ = self._mr_candidates(cands_t, bits, checked=_checked)
        self.calls.append(("mr_split", rows))
        parts = [mr_model.split(n) for n in _ints(cands_t)]
        return _rows_t([d for d, _ in parts], words), torch.tensor([s for _, s in parts], dtype=torch.int32)

    def miller_rabin_t(self, cands_t, bases_t, group_size, out_t=None, bits=None, _checked=False):
        if int(group_size) < 1:
            raise ValueError("group_size must be at least 1")
        rows, words, _ = self._mr_candidates(cands_t, bits, checked=_checked)
        if tuple(bases_t.shape) != (rows * group_size, words):
            raise ValueError("bases_t must hold group_size rows per candidate")
        self.calls.append(("miller_rabin", rows, group_size))
        vals = _ints(cands_t)
        return _flags_t(mr_model.round_passes(vals[k // group_size], b) for k, b in enumerate(_ints(bases_t)))

    def miller_rabin_base2_t(self, cands_t, bits=None, out_t=None, _checked=False):
        rows, _, bits = self._mr_candidates(cands_t, bits, checked=_checked)
        self.calls.append(("base2", rows))
        return _flags_t(mr_model.base2(n, bits) for n in _ints(cands_t))

    def generator_shares_t(self, mods, group_size, rng=None, draws_t=None, out_t=None):
        """Device ``(rows, bits)`` moduli only: ONE draw of S * G rows of bits + 64 bits, row c * G + k modulo candidate c."""
        if not _is_pair(mods) or int(group_size) < 1 or (rng is None) == (draws_t is None):
            raise ValueError("a device (rows, bits) pair, group_size >= 1 and exactly one of rng and draws_t expected")
        mods_t, bits = mods
        total = len(mods_t) * group_size
        self.calls.append(("generator_shares", len(mods_t), group_size))
        if total and draws_t is None:
            draws_t = rng.rows_t(self, total, bits + 64, (bits + 64 + 31) // 32)
        ms = _ints(mods_t)
        return _rows_t([d % ms[k // group_size] for k, d in enumerate(_ints(draws_t) if total else [])], mods_t.shape[1])

    # ---- the shipped compositions, recorded
    def probable_prime_t(self, cands_t, bits, rounds, rng, **kwargs):
        return self._recorded(("probable_prime", len(cands_t), rounds), super().probable_prime_t, cands_t, bits, rounds, rng, **kwargs)

    def prime_search_t(self, count, bits, rng, rounds=64, batch=None):
        return self._recorded(lambda: ("prime_search", count, bits, _drawn_batch(primes.default_batch, count, bits, batch)),
                              super().prime_search_t, count, bits, rng, rounds=rounds, batch=batch)
