"""A Python-int double of the engine PRIMITIVES threshold.py drives — ``sha256_rows_t`` / ``dleq_response_t`` /
``multiexp_nsquare_rows_t`` / the fixed-base tables and the existing ``powmod_nsquare_t`` / ``mulmod_t`` /
``multiexp_nsquare_t`` / ``combine_t`` — on CPU ``int32`` tensors; every step is Python ints and hashlib.  ``dleq_prove_t``
and ``dleq_verify_t`` are NOT written again here: the double inherits ``ProofFlows`` and runs the shipped composition
(piece bases by squarings, one multi-exponentiation whose weight block is the exponent rows, fixed-base products piece by
piece) over these primitives, recording what it is asked.  It extends the safe-prime double, which works on
the same CPU tensors and runs the shipped private-key compositions, so ``deal(check=True)`` runs over it.  Lives in tests/ only; the product
never imports it."""

from __future__ import annotations

import hashlib

import numpy as np

from crt_engine import _flags_t, _host, _ints, _rows, _rows_t  # noqa: F401
from safe_engine import FakeRng, SafeEngine  # noqa: F401

from protocols.distributed_keygen_amd import limbs
from protocols.distributed_keygen_amd.proof_flows import ProofFlows


class ProofEngine(ProofFlows, SafeEngine):
    def __init__(self):
        super().__init__()
        self.statuses = []          # what every response primitive returned, for _proved

    def _proved(self, marker, prove, *args, **kwargs):
        """Record `marker`, run the shipped prover and check that no response it computed overflowed its rows."""
        self.calls.append(marker)
        first = len(self.statuses)
        out = prove(*args, **kwargs)
        assert not any(bool(s.any()) for s in self.statuses[first:]), "a response of the prover overflowed its rows"
        return out

    def _response_t(self, full, wz):
        """(z, status) of a response primitive from the sums `full` over the integers; the status is kept for _proved."""
        self.statuses.append(_flags_t(f >> (32 * wz) for f in full))
        return _rows_t([f & ((1 << (32 * wz)) - 1) for f in full], wz), self.statuses[-1]

    # ---- existing entry points, in ints
    def mulmod_t(self, a_t, b_t, mod, out_t=None):
        return _rows_t([x * y % mod for x, y in zip(_ints(a_t), _ints(b_t))], a_t.shape[1])

    def multiexp_nsquare_t(self, inputs_t, weights, n, bias=None, window=0):
        n2 = n * n
        xs = _ints(inputs_t)
        self.calls.append(("multiexp", len(xs), len(weights)))
        out = []
        for row in weights:
            items = row.items() if isinstance(row, dict) else enumerate(row)
            acc = 1
            for i, w in items:
                acc = acc * pow(xs[i], w, n2) % n2          # (a negative weight: ValueError like pow if there is no inverse)
            out.append(acc)
        return _rows_t(out, inputs_t.shape[1])

    def combine_t(self, partials_t, n, theta_inv, out_t=None, status_t=None, packed=False):
        n2 = n * n
        n_partials, batch, limbs2 = partials_t.shape
        cols = [_ints(partials_t[k]) for k in range(n_partials)]
        self.calls.append(("combine", n_partials, batch))
        out, status = [], []
        for r in range(batch):
            acc = 1
            for col in cols:
                acc = acc * col[r] % n2
            status.append(0 if acc % n == 1 else 1)
            out.append((acc - 1) // n * theta_inv % n if acc % n == 1 else 0)
        return _rows(out, limbs.limbs_for(n)), np.array(status, dtype=np.uint8)

    # ---- the primitives of the decryption proofs
    def sha256_rows_t(self, prefix, row_sets, count=None):
        prefix = bytes(prefix)
        if len(prefix) != 32 or len(row_sets) > 8:
            raise ValueError("a 32-byte prefix and at most 8 row sets expected")
        rows = int(count) if count is not None else row_sets[0].shape[0]
        self.calls.append(("sha256_rows", rows, [t.shape[1] for t in row_sets]))
        sets = [_host(t) for t in row_sets]
        digests = []
        for r in range(rows):
            msg = prefix + b"".join(np.ascontiguousarray(t[r][::-1]).astype(">u4").tobytes() for t in sets)
            digests.append(int.from_bytes(hashlib.sha256(msg).digest(), "big"))
        return _rows_t(digests, 8)

    def dleq_response_t(self, rho_t, e_t, x_t, out_t=None):
        (x,) = _ints(x_t.view(1, -1))
        self.calls.append(("dleq_response", len(rho_t), rho_t.shape[1], e_t.shape[1], x_t.numel()))
        return self._response_t([r + e * x for r, e in zip(_ints(rho_t), _ints(e_t))], rho_t.shape[1])

    def multiexp_nsquare_rows_t(self, inputs_t, index_t, weights_t, terms, weight_bits, n, window=0, _checked=False):
        n2 = n * n
        if weight_bits < 1 or weight_bits > 2 * n.bit_length() + 64:
            raise ValueError("weight_bits in 1 .. 2 bits(n) + 64 expected")          # the limit of mx_multiexp_nsquare_run
        ww = (weight_bits + 31) // 32
        rows = index_t.shape[0]
        if tuple(index_t.shape) != (rows, terms) or weights_t.numel() != rows * terms * ww:
            raise ValueError("index [rows, terms] and weights of terms x ww words per row expected")
        xs = _ints(inputs_t)
        if rows and (int(index_t.min()) < 0 or int(index_t.max()) >= len(xs)):
            raise ValueError("index out of range")
        ws = _ints(weights_t.reshape(rows * terms, ww))
        self.calls.append(("multiexp_rows", len(xs), rows, terms, weight_bits))
        out = []
        for r in range(rows):
            acc = 1
            for t in range(terms):
                acc = acc * pow(xs[int(index_t[r][t])], ws[r * terms + t], n2) % n2
            out.append(acc)
        return _rows_t(out, inputs_t.shape[1])

    def fixed_base_table(self, n, base, exp_bits, window=0):
        """A table is just (n, base, exp_bits), refused outside the tables' limit."""
        if exp_bits < 1 or exp_bits > 2 * n.bit_length() + 64:
            raise ValueError("exp_bits in 1 .. 2 bits(n) + 64 expected")
        return n, base, exp_bits

    def fixed_base_power_t(self, table, exps_t):
        n, _, _ = table
        return self.fixed_base_randomize_t(table, exps_t, _rows_t([1] * len(exps_t), limbs.limbs_for(n * n)))

    def fixed_base_randomize_t(self, table, exps_t, cts_t):
        n, base, exp_bits = table
        if exps_t.shape[1] != (exp_bits + 31) // 32:
            raise ValueError("exponent rows of the table's width expected")
        n2 = n * n
        return _rows_t([f * pow(base, e, n2) % n2 for f, e in zip(_ints(cts_t), _ints(exps_t))], limbs.limbs_for(n2))

    # ---- the shipped compositions, recorded
    def dleq_prove_t(self, cts_t, partials_t, n, v_bases, ctx, x_t, rho_bits, kw, **source):
        return self._proved(("dleq_prove", cts_t.shape[0], len(v_bases), kw), super().dleq_prove_t,
                            cts_t, partials_t, n, v_bases, ctx, x_t, rho_bits, kw, **source)

    def dleq_verify_t(self, cts_t, partials_t, a_t, b_t, z_t, n, v_bases, w, ctx, z_bits, kw):
        self.calls.append(("dleq_verify", cts_t.shape[0], len(v_bases), kw))
        return super().dleq_verify_t(cts_t, partials_t, a_t, b_t, z_t, n, v_bases, w, ctx, z_bits, kw)


def tamperings(pub, cts, col, proofs, other_ct):
    """(name, index, cts, partials, a, b, z) with row 1 — and only row 1 — spoiled."""
    a, b, z = proofs.to_ints()
    n2 = pub.n_square

    def at1(vals, v):
        return vals[:1] + [v] + vals[2:]

    return [
        ("c_i", 2, cts, at1(col, col[1] * 4 % n2), a, b, z),
        ("a", 2, cts, col, at1(a, a[1] * 4 % n2), b, z),
        ("b", 2, cts, col, a, at1(b, b[1] + 1), z),
        ("z", 2, cts, col, a, b, at1(z, z[1] + 1)),
        ("another ciphertext", 2, at1(cts, other_ct), col, a, b, z),
        ("z out of range", 2, cts, col, a, b, at1(z, z[1] + (1 << pub.z_bits))),
        ("z beyond its row", 2, cts, col, a, b, at1(z, z[1] + (1 << (32 * pub.z_words)))),
        ("a >= N^2", 2, cts, col, at1(a, a[1] + n2), b, z),
        ("b >= N^2", 2, cts, col, a, at1(b, b[1] + n2), z),
        ("c_i >= N^2", 2, cts, at1(col, col[1] + n2), a, b, z),
        ("negative", 2, cts, col, at1(a, -a[1]), b, z),
    ]
