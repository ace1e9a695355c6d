"""A Python-int double of the engine methods behind the safe-prime layer of primes.py and private_key.py —
``safe_sieve_t`` / ``safe_double_t`` / ``safe_prime_t`` / ``safe_prime_search_t`` on numpy rows — computed by the model
of the pipeline (tools/mr_model.py).  It extends the double of the prime search (mr_engine.py), so a safe-prime key
generated over it encrypts and decrypts.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

import numpy as np

from mr_engine import FakeRng, MrEngine, mr_model  # noqa: F401

from protocols.distributed_keygen_amd import limbs, primes


class SafeEngine(MrEngine):
    def safe_sieve_t(self, halves_t, prime_list, out_t=None):
        prime_list = [int(p) for p in prime_list]
        if not prime_list or any(p < 3 or p % 2 == 0 or p >= 1 << 31 for p in prime_list):
            raise ValueError("a list of odd primes in [3, 2^31) expected")
        self.calls.append(("safe_sieve", len(halves_t)))
        return np.array([any(h % l == 0 or h % l == (l - 1) // 2 for l in prime_list) for h in limbs.unpack(halves_t)], dtype=np.uint8)

    def safe_double_t(self, halves_t):
        vals = limbs.unpack(halves_t)
        if any(h >> (32 * halves_t.shape[1] - 1) for h in vals):
            raise ValueError("2h + 1 does not fit the rows' width")
        self.calls.append(("safe_double", len(vals)))
        return limbs.pack([2 * h + 1 for h in vals], halves_t.shape[1])

    def safe_prime_t(self, halves_t, bits, rounds, rng):
        if int(rounds) < 1:
            raise ValueError("rounds must be at least 1")
        if not 3 <= int(bits) <= 32 * halves_t.shape[1]:
            raise ValueError("bits must lie in [3, 32 * limbs]")
        vals, _ = self._candidates(halves_t, int(bits) - 1, above=primes.SIEVE_BOUND)
        self.calls.append(("safe_prime", len(vals), rounds))
        return np.array(mr_model.safe_prime(vals, int(bits), int(rounds), self._draw(rng)), dtype=np.uint8)

    def safe_prime_search_t(self, count, bits, rng, rounds=64, batch=None):
        if count < 0 or bits < 16 or rounds < 1:
            raise ValueError("count >= 0, bits >= 16 and rounds >= 1 expected")
        batch = primes.default_safe_batch(count, bits) if batch is None else int(batch)
        self.calls.append(("safe_prime_search", count, bits, batch))
        found, _ = mr_model.safe_prime_search(count, bits, self._draw(rng), rounds, batch)
        return limbs.pack(found, limbs.limbs_for_bits(bits))
