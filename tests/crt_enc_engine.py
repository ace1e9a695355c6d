"""A Python-int double of the engine PRIMITIVES the encryption side of private_key.py drives — ``crt_prime_split_t`` /
``crt_lift_t`` / ``powmod_shared_t`` / ``powmod_multi_t`` / ``random_rows_t`` — on CPU ``int32`` tensors, computed by the
model of the kernels (tools/crt_model.py: CrtEncPlan, the same Montgomery products, constants and bounds, asserted as it
goes) with ``pow`` for the modexps.  ``private_noise_t``, ``private_encrypt_t``, ``private_randomize_t`` and the int-level
batches are NOT written again here: they are the shipped compositions of ``PrivateKeyFlows``, recorded.  It extends the
decryption's double, so a key object over it encrypts and decrypts.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

import random

import torch

from crt_engine import CrtEngine, _ints, _rows_t, _with_status, crt_model

from protocols.distributed_keygen_amd import limbs


class FakeRng:
    """Stands in for device_rng.DeviceRng: rows of random bits from a seeded host generator."""

    def __init__(self, seed=0):
        self.rng = random.Random(seed)
        self.calls = []

    def rows_t(self, engine, count, bits, row_words=None):
        self.calls.append((count, bits, row_words))
        return _rows_t([self.rng.getrandbits(bits) for _ in range(count)], row_words or (bits + 31) // 32)


def _is_pair(x):
    return isinstance(x, tuple) and len(x) == 2 and hasattr(x[0], "data_ptr")


class CrtEncEngine(CrtEngine):
    _fixed_window = False

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

    # ---- the primitives of the encryption, in ints
    def crt_prime_split_t(self, rows_t, p, q):
        plan = self.enc_plan(p, q, rows_t.shape[1])
        res = [plan.prime_split(r) for r in _ints(rows_t)]
        self.calls.append(("prime_split", len(res)))
        return torch.stack([_rows_t([h[k] for h in res], plan.limbs_half) for k in (0, 1)])

    def crt_lift_t(self, rho_p_t, rho_q_t, p, q, messages_t=None, halves_t=None, packed=False):
        plan = self.enc_plan(p, q)
        if messages_t is not None and halves_t is not None:
            raise ValueError("a message or a ciphertext, not both")
        batch = rho_p_t.shape[0]
        if messages_t is not None and (messages_t.shape[0] != batch or messages_t.shape[1] < plan.limbs_n):
            raise ValueError("one message row per noise row expected, no narrower than N")
        rp, rq = _ints(rho_p_t), _ints(rho_q_t)
        ms = [None] * batch if messages_t is None else _ints(messages_t)
        hs = [None] * batch if halves_t is None else list(zip(_ints(halves_t[0]), _ints(halves_t[1])))
        res = [plan.lift(a, b, m=m, halves=h) for a, b, m, h in zip(rp, rq, ms, hs)]
        self.calls.append(("lift", batch, "message" if messages_t is not None else "halves" if halves_t is not None else "noise"))
        return _with_status(_rows_t([c for c, _ in res], plan.limbs2), torch.tensor([s for _, s in res], dtype=torch.uint8), packed)

    def powmod_shared_t(self, bases_t, mod, exp, out_t=None):
        if exp < 0:
            raise ValueError("negative exponent: invert the base first (paillier_shared_key.py:89-91)")
        self.calls.append(("powmod_shared", len(bases_t)))
        return _rows_t([pow(b, exp, mod) for b in _ints(bases_t)], bases_t.shape[1])

    def powmod_multi_t(self, bases_t, mods, exps, group_size, out_t=None):
        """One modulus and one exponent per `group_size` rows, each a list of ints or a device pair (rows, bits)."""
        ms, mod_bits = (_ints(mods[0]), mods[1]) if _is_pair(mods) else (list(mods), limbs.max_bits(mods))
        es, exp_bits = (_ints(exps[0]), exps[1]) if _is_pair(exps) else (list(exps), limbs.max_bits(exps))
        if len(ms) != len(es) or len(bases_t) != len(ms) * group_size:
            raise ValueError("one modulus and one exponent per group expected")
        assert all(m.bit_length() <= mod_bits for m in ms) and all(e.bit_length() <= exp_bits for e in es)          # the caller's bounds
        self.calls.append(("powmod_multi", len(ms), group_size, exp_bits))
        return _rows_t([pow(b, es[k // group_size], ms[k // group_size]) for k, b in enumerate(_ints(bases_t))], bases_t.shape[1])

    # ---- the shipped compositions, recorded
    def private_encrypt_batch(self, messages, p, q, **kwargs):
        return self._recorded(("encrypt", len(messages)), super().private_encrypt_batch, messages, p, q, **kwargs)

    def private_randomize_batch(self, ciphertexts, p, q, **kwargs):
        return self._recorded(("randomize", len(ciphertexts)), super().private_randomize_batch, ciphertexts, p, q, **kwargs)
