"""A Python-int double of the engine PRIMITIVES private-key decryption drives — ``crt_split_t`` / ``crt_recombine_t`` /
``powmod_nsquare_t``, the staging between ints and rows, ``nsquare_plan`` and ``_crt_pair`` — on CPU ``int32`` tensors,
computed by the model of the kernels (tools/crt_model.py: the same Montgomery products, constants and bounds, asserted as
it goes) with ``pow`` for the modexps.  ``private_decrypt_t`` and ``private_decrypt_batch`` are NOT written again here:
the double inherits ``PrivateKeyFlows`` and runs the shipped compositions over these primitives, recording what it is
asked.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import crt_model  # noqa: E402

from protocols.distributed_keygen_amd import limbs  # noqa: E402
from protocols.distributed_keygen_amd.key_flows import PrivateKeyFlows  # noqa: E402

# the records of the shipped compositions; everything else in ``calls`` is a primitive
MARKERS = ("decrypt", "encrypt", "randomize", "probable_prime", "prime_search", "safe_prime", "safe_prime_search")


def _rows(values, words):
    return limbs.pack(list(values), words).reshape(len(values), words) if len(values) else np.zeros((0, words), dtype=np.uint32)


def _host(rows_t):
    """Rows, a CPU tensor or numpy already, as contiguous uint32 numpy rows."""
    return np.ascontiguousarray(np.asarray(rows_t)).view(np.uint32)


def _ints(rows_t):
    return limbs.unpack(_host(rows_t)) if len(rows_t) else []


def _rows_t(values, words):
    return torch.from_numpy(_rows(values, words).view(np.int32))


def _flags_t(flags):
    return torch.tensor([1 if f else 0 for f in flags], dtype=torch.uint8)


def _with_status(rows_t, status_t, packed):
    """(rows, status), or ONE tensor whose last word is the status: the formats of combine_t."""
    return torch.cat([rows_t, status_t.to(torch.int32).view(-1, 1)], dim=1) if packed else (rows_t, status_t)


class CrtEngine(PrivateKeyFlows):
    torch = torch
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []
        self._plans = {}
        self._depth = 0

    def plan(self, p, q, limbs2=0):
        key = (p, q, limbs2)
        if key not in self._plans:
            self._plans[key] = crt_model.CrtPlan(p, q, limbs2)
        return self._plans[key]

    def _recorded(self, marker, run, *args, **kwargs):
        """Run a shipped composition and record `marker` in front of the primitives it called: only once it has accepted
        the call, and only for the composition the caller asked for, not for those it runs inside.  A callable marker is
        evaluated then."""
        at = len(self.calls)
        self._depth += 1
        try:
            out = run(*args, **kwargs)
        finally:
            self._depth -= 1
        if not self._depth:
            self.calls.insert(at, marker() if callable(marker) else marker)
        return out

    # ---- rows in and out
    @staticmethod
    def to_device(rows):
        return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.uint32).view(np.int32))

    to_host = staticmethod(_host)

    def _empty_rows(self, limbs_, rows=0):
        return torch.empty((rows, limbs_), dtype=torch.int32)

    def _staged_rows(self, which, values, limbs_, moduli, nested=0):
        return self.to_device(limbs.pack_reduced(values, limbs_, moduli))

    def _fetched_ints(self, which, rows_t, groups=None):
        return _ints(rows_t)

    _download_ints = staticmethod(_ints)

    def nsquare_plan(self, n, exp):
        return None

    def _crt_pair(self, run_p, run_q, side_by_side):
        return run_p(), run_q()

    # ---- the primitives of the decryption, in ints
    def crt_split_t(self, cts_t, p, q):
        plan = self.plan(p, q, cts_t.shape[1])
        halves = [plan.split(c) for c in _ints(cts_t)]
        self.calls.append(("split", len(halves)))
        return torch.stack([_rows_t([h[k] for h in halves], plan.limbs_half) for k in (0, 1)])

    def crt_recombine_t(self, xp_t, xq_t, p, q, packed=False, limbs2=0):
        plan = self.plan(p, q, limbs2)
        res = [plan.recombine(a, b) for a, b in zip(_ints(xp_t), _ints(xq_t))]
        self.calls.append(("recombine", len(res), packed))
        return _with_status(_rows_t([m for m, _ in res], plan.limbs_n), torch.tensor([s for _, s in res], dtype=torch.uint8), packed)

    def powmod_nsquare_t(self, bases_t, n, exp, out_t=None):
        if exp < 0:
            raise ValueError("negative exponent: invert the base first (paillier_shared_key.py:89-91)")
        self.calls.append(("powmod_nsquare", len(bases_t)))
        return _rows_t([pow(b, exp, n * n) for b in _ints(bases_t)], bases_t.shape[1])

    # ---- the shipped compositions, recorded
    def private_decrypt_batch(self, cts, p, q):
        return self._recorded(("decrypt", len(cts)), super().private_decrypt_batch, cts, p, q)
