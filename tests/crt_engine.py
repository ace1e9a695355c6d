"""A Python-int double of the engine methods private_key.py drives — ``private_decrypt_batch`` and the tensor-level
``crt_split_t`` / ``crt_recombine_t`` / ``private_decrypt_t`` on numpy rows — computed by the model of the kernels
(tools/crt_model.py: the same Montgomery products, constants and bounds, asserted as it goes) with ``pow`` for the two
modexps.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import crt_model  # noqa: E402

from protocols.distributed_keygen_amd import limbs  # noqa: E402


class CrtEngine:
    def __init__(self):
        self.calls = []
        self._plans = {}

    def plan(self, p, q, limbs2=0):
        key = (p, q, limbs2)
        if key not in self._plans:
            self._plans[key] = crt_model.CrtPlan(p, q, limbs2)
        return self._plans[key]

    # ---- tensor level: "device" rows are numpy uint32 rows
    def crt_split_t(self, cts_t, p, q):
        plan = self.plan(p, q, cts_t.shape[1])
        halves = [plan.split(c) for c in limbs.unpack(cts_t)]
        self.calls.append(("split", len(halves)))
        return np.stack([limbs.pack([h[k] for h in halves], plan.limbs_half) for k in (0, 1)]) if halves else \
            np.zeros((2, 0, plan.limbs_half), dtype=np.uint32)

    def crt_recombine_t(self, xp_t, xq_t, p, q, packed=False, limbs2=0):
        plan = self.plan(p, q, limbs2)
        res = [plan.recombine(a, b) for a, b in zip(limbs.unpack(xp_t), limbs.unpack(xq_t))]
        self.calls.append(("recombine", len(res), packed))
        rows = limbs.pack([m for m, _ in res], plan.limbs_n) if res else np.zeros((0, plan.limbs_n), dtype=np.uint32)
        status = np.array([s for _, s in res], dtype=np.uint8)
        if packed:
            return np.concatenate([rows, status.astype(np.uint32)[:, None]], axis=1)
        return rows, status

    def private_decrypt_t(self, cts_t, p, q, packed=False):
        half = self.crt_split_t(cts_t, p, q)
        plan = self.plan(p, q, cts_t.shape[1])
        xp = limbs.pack([pow(c, p - 1, p * p) for c in limbs.unpack(half[0])], plan.limbs_half)
        xq = limbs.pack([pow(c, q - 1, q * q) for c in limbs.unpack(half[1])], plan.limbs_half)
        return self.crt_recombine_t(xp.reshape(-1, plan.limbs_half), xq.reshape(-1, plan.limbs_half), p, q, packed, cts_t.shape[1])

    # ---- int level
    def private_decrypt_batch(self, cts, p, q):
        self.calls.append(("decrypt", len(cts)))
        if len(cts) == 0:
            return [], []
        n2 = (p * q) ** 2
        rows, status = self.private_decrypt_t(limbs.pack([int(c) % n2 for c in cts], limbs.limbs_for(n2)), p, q)
        return limbs.unpack(rows), [not bool(s) for s in status]
