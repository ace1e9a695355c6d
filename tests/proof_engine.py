"""A Python-int double of the engine methods threshold.py drives — the new ``sha256_rows_t`` / ``dleq_response_t`` /
``multiexp_nsquare_rows_t`` / ``dleq_prove_t`` / ``dleq_verify_t`` and the existing ``powmod_nsquare_t`` / ``mulmod_t`` /
``multiexp_nsquare_t`` / ``combine_t`` it composes them with — on numpy rows.  ``dleq_prove_t`` and ``dleq_verify_t`` are
COMPOSED here the way the engine composes them (piece bases by squarings, one multi-exponentiation whose weight block is
the exponent rows viewed as [count][pieces][kw], fixed-base products piece by piece), so the piece split is exercised, at
any number of pieces; every step is Python ints and hashlib.  It extends the safe-prime double, so ``deal(check=True)``
runs over it.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

import hashlib

import numpy as np

from safe_engine import FakeRng, SafeEngine  # noqa: F401

from protocols.distributed_keygen_amd import limbs


def _rows(values, words):
    return limbs.pack(list(values), words).reshape(len(values), words) if len(values) else np.zeros((0, words), dtype=np.uint32)


class ProofEngine(SafeEngine):
    # ---- existing entry points, in ints
    def powmod_nsquare_t(self, bases_t, n, exp, out_t=None):
        if exp < 0:
            raise ValueError("negative exponent: invert the base first (paillier_shared_key.py:89-91)")
        self.calls.append(("powmod_nsquare", len(bases_t)))
        return _rows([pow(b, exp, n * n) for b in limbs.unpack(bases_t)], bases_t.shape[1])

    def mulmod_t(self, a_t, b_t, mod, out_t=None):
        return _rows([x * y % mod for x, y in zip(limbs.unpack(a_t), limbs.unpack(b_t))], a_t.shape[1])

    def multiexp_nsquare_t(self, inputs_t, weights, n, bias=None, window=0):
        n2 = n * n
        xs = limbs.unpack(inputs_t)
        self.calls.append(("multiexp", len(xs), len(weights)))
        out = []
        for row in weights:
            items = row.items() if isinstance(row, dict) else enumerate(row)
            acc = 1
            for i, w in items:
                acc = acc * pow(xs[i], w, n2) % n2          # (a negative weight: ValueError like pow if there is no inverse)
            out.append(acc)
        return _rows(out, inputs_t.shape[1])

    def combine_t(self, partials_t, n, theta_inv, out_t=None, status_t=None, packed=False):
        n2 = n * n
        n_partials, batch, limbs2 = partials_t.shape
        cols = [limbs.unpack(partials_t[k]) for k in range(n_partials)]
        self.calls.append(("combine", n_partials, batch))
        out, status = [], []
        for r in range(batch):
            acc = 1
            for col in cols:
                acc = acc * col[r] % n2
            status.append(0 if acc % n == 1 else 1)
            out.append((acc - 1) // n * theta_inv % n if acc % n == 1 else 0)
        return _rows(out, limbs.limbs_for(n)), np.array(status, dtype=np.uint8)

    # ---- the new entry points
    def sha256_rows_t(self, prefix, row_sets, count=None):
        prefix = bytes(prefix)
        if len(prefix) != 32 or len(row_sets) > 8:
            raise ValueError("a 32-byte prefix and at most 8 row sets expected")
        rows = int(count) if count is not None else row_sets[0].shape[0]
        self.calls.append(("sha256_rows", rows, [t.shape[1] for t in row_sets]))
        digests = []
        for r in range(rows):
            msg = prefix + b"".join(np.ascontiguousarray(t[r][::-1]).astype(">u4").tobytes() for t in row_sets)
            digests.append(int.from_bytes(hashlib.sha256(msg).digest(), "big"))
        return _rows(digests, 8)

    def dleq_response_t(self, rho_t, e_t, x_t, out_t=None):
        wz = rho_t.shape[1]
        (x,) = limbs.unpack(np.asarray(x_t).reshape(1, -1))
        full = [r + e * x for r, e in zip(limbs.unpack(rho_t), limbs.unpack(e_t))]
        self.calls.append(("dleq_response", len(full), wz, e_t.shape[1], np.asarray(x_t).size))
        return _rows([f & ((1 << (32 * wz)) - 1) for f in full], wz), np.array([1 if f >> (32 * wz) else 0 for f in full], dtype=np.uint8)

    def multiexp_nsquare_rows_t(self, inputs_t, index_t, weights_t, terms, weight_bits, n, window=0):
        n2 = n * n
        if weight_bits < 1 or weight_bits > 2 * n.bit_length() + 64:
            raise ValueError("weight_bits in 1 .. 2 bits(n) + 64 expected")          # the limit of mx_multiexp_nsquare_run
        ww = (weight_bits + 31) // 32
        rows = index_t.shape[0]
        if tuple(index_t.shape) != (rows, terms) or weights_t.size != rows * terms * ww:
            raise ValueError("index [rows, terms] and weights of terms x ww words per row expected")
        xs = limbs.unpack(inputs_t)
        if rows and (int(index_t.min()) < 0 or int(index_t.max()) >= len(xs)):
            raise ValueError("index out of range")
        ws = limbs.unpack(np.ascontiguousarray(weights_t).reshape(rows * terms, ww))
        self.calls.append(("multiexp_rows", len(xs), rows, terms, weight_bits))
        out = []
        for r in range(rows):
            acc = 1
            for t in range(terms):
                acc = acc * pow(xs[int(index_t[r][t])], ws[r * terms + t], n2) % n2
            out.append(acc)
        return _rows(out, inputs_t.shape[1])

    def _fixed_base_t(self, base, exp_bits, exps_t, n, operand_t=None):
        """fixed_base_power_t / fixed_base_randomize_t through a table of `base` for exponents below 2^exp_bits."""
        if exp_bits < 1 or exp_bits > 2 * n.bit_length() + 64 or exps_t.shape[1] != (exp_bits + 31) // 32:
            raise ValueError("exp_bits in 1 .. 2 bits(n) + 64 and exponent rows of that width expected")    # the tables' limit
        n2 = n * n
        ops = limbs.unpack(operand_t) if operand_t is not None else [1] * len(exps_t)
        return _rows([f * pow(base, e, n2) % n2 for f, e in zip(ops, limbs.unpack(np.ascontiguousarray(exps_t)))], limbs.limbs_for(n2))

    def _bases_t(self, cts_t, n, pieces, kw):
        out = [self.powmod_nsquare_t(cts_t, n, 4)]
        for _ in range(pieces - 1):
            out.append(self.powmod_nsquare_t(out[-1], n, 1 << (32 * kw)))
        return out

    def _powers_t(self, bases, exps_t, n, kw):
        pieces, count = len(bases), exps_t.shape[0]
        index_t = (np.arange(count, dtype=np.int32).reshape(-1, 1) + count * np.arange(pieces, dtype=np.int32).reshape(1, -1))
        return self.multiexp_nsquare_rows_t(np.concatenate(bases), index_t, exps_t.reshape(count, pieces, kw), pieces, 32 * kw, n)

    def _fixed_t(self, v_bases, exps_t, n, kw):
        out_t = None
        for j, base in enumerate(v_bases):
            out_t = self._fixed_base_t(base, 32 * kw, exps_t[:, j * kw : (j + 1) * kw], n, out_t)
        return out_t

    def dleq_prove_t(self, cts_t, partials_t, n, v_bases, ctx, x_t, rho_bits, kw, rng=None, rho_t=None):
        count, pieces = cts_t.shape[0], len(v_bases)
        zw = pieces * kw
        if (rng is None) == (rho_t is None):
            raise ValueError("exactly one of rng and rho_t expected")
        if not 1 <= rho_bits < 32 * zw or 32 * kw > 2 * n.bit_length() + 64:
            raise ValueError("pieces that hold rho_bits + 1 bits expected")
        if rho_t is None:
            rho_t = rng.rows_t(self, count, rho_bits, zw)
        self.calls.append(("dleq_prove", count, pieces, kw))
        bases = self._bases_t(cts_t, n, pieces, kw)
        ci2_t = self.mulmod_t(partials_t, partials_t, n * n)
        a_t = self._powers_t(bases, rho_t, n, kw)
        b_t = self._fixed_t(v_bases, rho_t, n, kw)
        e_t = np.ascontiguousarray(self.sha256_rows_t(ctx, [bases[0], ci2_t, a_t, b_t])[:, 4:8])
        z_t, status = self.dleq_response_t(rho_t, e_t, x_t)
        assert not status.any()
        return a_t, b_t, z_t

    def dleq_verify_t(self, cts_t, partials_t, a_t, b_t, z_t, n, v_bases, w, ctx, z_bits, kw):
        count, pieces = cts_t.shape[0], len(v_bases)
        n2 = n * n
        if z_t.shape[1] != pieces * kw or any(t.shape != cts_t.shape for t in (partials_t, a_t, b_t)):
            raise ValueError("rows of the wrong shape")
        self.calls.append(("dleq_verify", count, pieces, kw))
        ok = np.array([z < 1 << z_bits for z in limbs.unpack(z_t)], dtype=bool)
        for t in (cts_t, partials_t, a_t, b_t):
            ok &= np.array([v < n2 for v in limbs.unpack(t)], dtype=bool)
        one = _rows([1], cts_t.shape[1])
        cts_t, partials_t, a_t, b_t = (np.where(ok[:, None], t, one) for t in (cts_t, partials_t, a_t, b_t))
        z_t = np.where(ok[:, None], z_t, 0).astype(np.uint32)
        bases = self._bases_t(cts_t, n, pieces, kw)
        ci2_t = self.mulmod_t(partials_t, partials_t, n2)
        e_t = np.ascontiguousarray(self.sha256_rows_t(ctx, [bases[0], ci2_t, a_t, b_t])[:, 4:8])
        left_t = self._powers_t(bases, z_t, n, kw)
        own = np.arange(count, dtype=np.int32).reshape(-1, 1)
        right_t = self.mulmod_t(a_t, self.multiexp_nsquare_rows_t(ci2_t, own, e_t, 1, 128, n), n2)
        left_v = self._fixed_t(v_bases, z_t, n, kw)
        right_v = self._fixed_base_t(w, 128, e_t, n, b_t)
        return ok & (left_t == right_t).all(axis=1) & (left_v == right_v).all(axis=1)


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
