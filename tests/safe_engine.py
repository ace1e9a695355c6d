"""A Python-int double of the engine PRIMITIVES behind the safe-prime layer of primes.py and private_key.py —
``safe_sieve_t`` / ``safe_double_t`` — on CPU ``int32`` tensors.  ``safe_prime_t`` and ``safe_prime_search_t`` are NOT
written again here: they are the shipped compositions of ``PrivateKeyFlows``, recorded, and tools/mr_model.py's pipeline
is the oracle the tests compare them with.  It extends the double of the prime search (mr_engine.py), so a safe-prime key
generated over it encrypts and decrypts.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

import math

from crt_engine import _flags_t, _ints, _rows_t
from mr_engine import FakeRng, MrEngine, _drawn_batch, _product, mr_model  # noqa: F401

from protocols.distributed_keygen_amd import primes


class SafeEngine(MrEngine):
    def safe_sieve_t(self, halves_t, prime_list, out_t=None):
        rows, _ = self._word_rows(halves_t, "halves")
        prime_list = [int(p) for p in prime_list]
        if not prime_list or any(p < 3 or p % 2 == 0 or p >= 1 << 31 for p in prime_list):
            raise ValueError("a list of odd primes in [3, 2^31) expected")
        self.calls.append(("safe_sieve", rows))
        product = _product(prime_list)                 # an odd l divides h (2h + 1) iff h = 0 or h = (l - 1) / 2 modulo l
        return _flags_t(math.gcd(h * (2 * h + 1), product) != 1 for h in _ints(halves_t))

    def safe_double_t(self, halves_t, _checked=False):
        rows, words = self._word_rows(halves_t, "halves")
        vals = _ints(halves_t)
        if any(h >> (32 * words - 1) for h in vals):
            raise ValueError("2h + 1 does not fit the rows' width")
        self.calls.append(("safe_double", rows))
        return _rows_t([2 * h + 1 for h in vals], words)

    # ---- the shipped compositions, recorded
    def safe_prime_t(self, halves_t, bits, rounds, rng, **kwargs):
        return self._recorded(("safe_prime", len(halves_t), rounds), super().safe_prime_t, halves_t, bits, rounds, rng, **kwargs)

    def safe_prime_search_t(self, count, bits, rng, rounds=64, batch=None):
        return self._recorded(lambda: ("safe_prime_search", count, bits, _drawn_batch(primes.default_safe_batch, count, bits, batch)),
                              super().safe_prime_search_t, count, bits, rng, rounds=rounds, batch=batch)
