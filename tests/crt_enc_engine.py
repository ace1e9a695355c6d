"""A Python-int double of the engine methods the encryption side of private_key.py drives — ``crt_prime_split_t`` /
``crt_lift_t`` / ``private_noise_t`` / ``private_encrypt_t`` / ``private_randomize_t`` on numpy rows and the int-level
``private_encrypt_batch`` / ``private_randomize_batch`` — computed by the model of the kernels (tools/crt_model.py:
CrtEncPlan, the same Montgomery products, constants and bounds, asserted as it goes) with ``pow`` for the modexps.  It
extends the decryption's double, so a key object over it encrypts and decrypts.  Lives in tests/ only; the product never
imports it."""

from __future__ import annotations

import random

import numpy as np

from crt_engine import CrtEngine, crt_model

from protocols.distributed_keygen_amd import limbs


class FakeRng:
    """Stands in for device_rng.DeviceRng: rows of random bits from a seeded host generator."""

    def __init__(self, seed=0):
        self.rng = random.Random(seed)
        self.calls = []

    def rows_t(self, engine, count, bits, row_words=None):
        self.calls.append((count, bits, row_words))
        return limbs.pack([self.rng.getrandbits(bits) for _ in range(count)], row_words or (bits + 31) // 32)


class CrtEncEngine(CrtEngine):
    def __init__(self):
        super().__init__()
        self._enc_plans = {}

    def enc_plan(self, p, q, limbs_r=0):
        key = (p, q, limbs_r)
        if key not in self._enc_plans:
            self._enc_plans[key] = crt_model.CrtEncPlan(p, q, limbs_r)
        return self._enc_plans[key]

    def random_rows_t(self, rng, count, bits, row_words=None):
        return rng.rows_t(self, count, bits, row_words)

    # ---- tensor level: "device" rows are numpy uint32 rows
    def crt_prime_split_t(self, rows_t, p, q):
        plan = self.enc_plan(p, q, rows_t.shape[1])
        res = [plan.prime_split(r) for r in limbs.unpack(rows_t)]
        self.calls.append(("prime_split", len(res)))
        return np.stack([limbs.pack([h[k] for h in res], plan.limbs_half) for k in (0, 1)]).reshape(2, len(res), plan.limbs_half)

    def crt_lift_t(self, rho_p_t, rho_q_t, p, q, messages_t=None, halves_t=None, packed=False):
        plan = self.enc_plan(p, q)
        if messages_t is not None and halves_t is not None:
            raise ValueError("a message or a ciphertext, not both")
        batch = rho_p_t.shape[0]
        if messages_t is not None and (messages_t.shape[0] != batch or messages_t.shape[1] < plan.limbs_n):
            raise ValueError("one message row per noise row expected, no narrower than N")
        rp, rq = limbs.unpack(rho_p_t), limbs.unpack(rho_q_t)
        ms = [None] * batch if messages_t is None else limbs.unpack(messages_t)
        hs = [None] * batch if halves_t is None else list(zip(limbs.unpack(halves_t[0]), limbs.unpack(halves_t[1])))
        res = [plan.lift(a, b, m=m, halves=h) for a, b, m, h in zip(rp, rq, ms, hs)]
        self.calls.append(("lift", batch, "message" if messages_t is not None else "halves" if halves_t is not None else "noise"))
        rows = limbs.pack([c for c, _ in res], plan.limbs2).reshape(batch, plan.limbs2)
        status = np.array([s for _, s in res], dtype=np.uint8)
        if packed:
            return np.concatenate([rows, status.astype(np.uint32)[:, None]], axis=1)
        return rows, status

    def _noise_halves(self, count, p, q, randomness_t, rng, draws_t):
        if (randomness_t is not None) + (rng is not None) + (draws_t is not None) != 1:
            raise ValueError("exactly one of randomness_t, rng and draws_t expected")
        plan = self.enc_plan(p, q)
        if randomness_t is not None:
            if randomness_t.shape[0] != count:
                raise ValueError("one randomness row per ciphertext expected")
            kept = randomness_t
            mod = self.crt_prime_split_t(randomness_t, p, q)
            sp = [pow(v, plan.e_p, p) for v in limbs.unpack(mod[0])]
            sq = [pow(v, plan.e_q, q) for v in limbs.unpack(mod[1])]
        else:
            if draws_t is None:
                bits = (p * q).bit_length() + 64
                draws_t = self.random_rows_t(rng, count, bits, max(plan.limbs2, (bits + 31) // 32))
            elif draws_t.shape[0] != count:
                raise ValueError("one draw per ciphertext expected")
            kept = draws_t
            mod = self.crt_split_t(draws_t.reshape(count, -1), p, q)
            sp, sq = limbs.unpack(mod[0]), limbs.unpack(mod[1])
        rho_p = limbs.pack([pow(v, p, p * p) for v in sp], plan.limbs_half).reshape(count, plan.limbs_half)
        rho_q = limbs.pack([pow(v, q, q * q) for v in sq], plan.limbs_half).reshape(count, plan.limbs_half)
        return rho_p, rho_q, kept

    def private_noise_t(self, count, p, q, randomness_t=None, rng=None, draws_t=None, side_by_side=True, packed=False):
        rho_p, rho_q, _ = self._noise_halves(count, p, q, randomness_t, rng, draws_t)
        return self.crt_lift_t(rho_p, rho_q, p, q, packed=packed)

    def private_encrypt_t(self, messages_t, p, q, randomness_t=None, rng=None, draws_t=None, side_by_side=True, packed=False,
                          return_randomness=False):
        rho_p, rho_q, kept = self._noise_halves(messages_t.shape[0], p, q, randomness_t, rng, draws_t)
        out = self.crt_lift_t(rho_p, rho_q, p, q, messages_t=messages_t, packed=packed)
        if not return_randomness:
            return out
        return (out, kept) if packed else (*out, kept)

    def private_randomize_t(self, cts_t, p, q, randomness_t=None, rng=None, draws_t=None, side_by_side=True, packed=False,
                            return_randomness=False):
        halves = self.crt_split_t(cts_t, p, q)
        rho_p, rho_q, kept = self._noise_halves(cts_t.shape[0], p, q, randomness_t, rng, draws_t)
        out = self.crt_lift_t(rho_p, rho_q, p, q, halves_t=halves, packed=packed)
        if not return_randomness:
            return out
        return (out, kept) if packed else (*out, kept)

    # ---- int level
    def _batch(self, run_t, rows, count, p, q, randomness, rng, return_randomness):
        if (randomness is None) == (rng is None):
            raise ValueError("exactly one of randomness and rng expected")
        if randomness is not None and len(randomness) != count:
            raise ValueError("one randomness per value expected")
        if count == 0:
            return ([], [], []) if return_randomness else ([], [])
        n = p * q
        r_t = None if randomness is None else limbs.pack([int(r) % n for r in randomness], limbs.limbs_for(n)).reshape(count, -1)
        out_t, status, kept = run_t(rows(), p, q, randomness_t=r_t, rng=rng, return_randomness=True)
        out = limbs.unpack(out_t), [not bool(s) for s in status]
        if not return_randomness:
            return out
        return (*out, list(randomness) if randomness is not None else limbs.unpack(kept))

    def private_encrypt_batch(self, messages, p, q, randomness=None, rng=None, return_randomness=False):
        self.calls.append(("encrypt", len(messages)))
        n = p * q
        width = limbs.limbs_for(n)
        return self._batch(self.private_encrypt_t, lambda: limbs.pack([int(m) % n for m in messages], width).reshape(len(messages), width),
                           len(messages), p, q, randomness, rng, return_randomness)

    def private_randomize_batch(self, ciphertexts, p, q, randomness=None, rng=None, return_randomness=False):
        self.calls.append(("randomize", len(ciphertexts)))
        n2 = (p * q) ** 2
        width = limbs.limbs_for(n2)
        return self._batch(self.private_randomize_t, lambda: limbs.pack([int(c) % n2 for c in ciphertexts], width).reshape(len(ciphertexts), width),
                           len(ciphertexts), p, q, randomness, rng, return_randomness)
