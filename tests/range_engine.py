"""A Python-int double of the engine PRIMITIVES range_proof.py drives — ``multiexp_mod_t`` / ``response_rows_t`` /
``powmod_multi_t`` / ``shamir_fma_t`` and the int-level encryption — on CPU ``int32`` tensors; every step is Python ints.
``range_prove_t``, ``range_verify_t`` and ``range_bounds_t`` are NOT written again here: the double runs the shipped
composition it inherits (``ProofFlows``: products of two powers routed as the engine routes them, the wide draw of rho
cut at a word boundary and reduced by a multiply-add, challenge rows over four row sets of two widths, per-row
responses) over these primitives, so widths, layouts, the draw order and the screening are the engine's own.  It extends
the double of the decryption proofs.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

from proof_engine import ProofEngine, _ints, _rows_t

from protocols.distributed_keygen_amd import limbs


class RangeEngine(ProofEngine):
    # ---- existing entry points, in ints
    def encrypt_batch(self, messages, randomness, n):
        n2 = n * n
        self.calls.append(("encrypt", len(messages)))
        return [(1 + (m % n) * n) % n2 * pow(r, n, n2) % n2 for m, r in zip(messages, randomness)]

    def encrypt_fresh_batch(self, messages, n, rng, return_randomness=False):
        rs = _ints(rng.rows_t(self, len(messages), n.bit_length() + 64, limbs.limbs_for(n * n)))
        out = self.encrypt_batch(messages, rs, n)
        return (out, rs) if return_randomness else out

    def shamir_fma_t(self, a_t, b_t, c_t, prime, out_t=None):
        return _rows_t([(a * b + c) % prime for a, b, c in zip(_ints(a_t), _ints(b_t), _ints(c_t))], a_t.shape[1])

    # ---- the primitives of the range proofs
    def multiexp_mod_t(self, inputs_t, index_t, weights_t, terms, weight_bits, mod, window=0, term_bits=None, _checked=False):
        if mod < 3 or mod % 2 == 0:
            raise ValueError("modulus must be odd and >= 3")
        if terms < 1 or not 1 <= weight_bits <= 16384:
            raise ValueError("terms >= 1 and weight_bits in 1 .. 16384 expected")          # the limit of mx_multiexp_run
        ww = (weight_bits + 31) // 32
        rows = index_t.shape[0]
        if tuple(index_t.shape) != (rows, terms) or weights_t.numel() != rows * terms * ww:
            raise ValueError("index [rows, terms] and weights of terms x ww words per row expected")
        xs = _ints(inputs_t)
        if rows and (int(index_t.min()) < 0 or int(index_t.max()) >= len(xs)):
            raise ValueError("index out of range")
        ws = _ints(weights_t.reshape(rows * terms, ww))
        assert all(w >> weight_bits == 0 for w in ws)
        if term_bits is not None:                       # the caller's promise: term t stays below 2^term_bits[t] in every row
            if len(term_bits) != terms or any(not 0 <= b <= weight_bits for b in term_bits):
                raise ValueError("one length in 0 .. weight_bits per term expected")
            assert all(ws[r * terms + t] >> term_bits[t] == 0 for r in range(rows) for t in range(terms))
        self.calls.append(("multiexp_mod", len(xs), rows, terms, weight_bits, mod.bit_length()))
        out = []
        for r in range(rows):
            acc = 1
            for t in range(terms):
                acc = acc * pow(xs[int(index_t[r][t])], ws[r * terms + t], mod) % mod
            out.append(acc)
        return _rows_t(out, inputs_t.shape[1])

    def response_rows_t(self, rho_t, e_t, x_t, out_t=None):
        self.calls.append(("response_rows", len(rho_t), rho_t.shape[1], e_t.shape[1], x_t.shape[1]))
        return self._response_t([r + e * x for r, e, x in zip(_ints(rho_t), _ints(e_t), _ints(x_t))], rho_t.shape[1])

    # ---- the shipped compositions, recorded, and what the mirror asserted of their operands
    def _one_plus_mn_t(self, m_t, n):
        assert all(m < n for m in _ints(m_t))
        return super()._one_plus_mn_t(m_t, n)

    def _reduce_wide_t(self, rows_t, n):
        assert not rows_t[:, (n.bit_length() - 1) // 32 + 3 :].any()
        return super()._reduce_wide_t(rows_t, n)

    def range_prove_t(self, cts_t, *args, **kwargs):
        return self._proved(("range_prove", cts_t.shape[0]), super().range_prove_t, cts_t, *args, **kwargs)

    def range_verify_t(self, cts_t, *args, **kwargs):
        self.calls.append(("range_verify", cts_t.shape[0]))
        return super().range_verify_t(cts_t, *args, **kwargs)


def tamperings(n, params, proofs_ints, cts, other_ct):
    """(name, cts, S, A, C, z1, z2, z3) with row 1 — and only row 1 — spoiled."""
    s, a, c, z1, z2, z3 = proofs_ints
    n2, nh = n * n, params.nh

    def at1(vals, v):
        return vals[:1] + [v] + vals[2:]

    return [
        ("c", at1(cts, cts[1] * (1 + n) % n2), s, a, c, z1, z2, z3),
        ("another ciphertext", at1(cts, other_ct), s, a, c, z1, z2, z3),
        ("S", cts, at1(s, s[1] * params.t % nh), a, c, z1, z2, z3),
        ("A", cts, s, at1(a, a[1] * (1 + n) % n2), c, z1, z2, z3),
        ("C", cts, s, a, at1(c, c[1] * params.t % nh), z1, z2, z3),
        ("z1", cts, s, a, c, at1(z1, z1[1] + 1), z2, z3),
        ("z2", cts, s, a, c, z1, at1(z2, z2[1] * 2 % n), z3),
        ("z3", cts, s, a, c, z1, z2, at1(z3, z3[1] + 1)),
        ("S >= Nh", cts, at1(s, s[1] + nh), a, c, z1, z2, z3),
        ("A >= N^2", cts, s, at1(a, a[1] + n2), c, z1, z2, z3),
        ("C >= Nh", cts, s, a, at1(c, c[1] + nh), z1, z2, z3),
        ("z2 >= N", cts, s, a, c, z1, at1(z2, z2[1] + n), z3),
        ("c >= N^2", at1(cts, cts[1] + n2), s, a, c, z1, z2, z3),
        ("negative", cts, s, at1(a, -a[1]), c, z1, z2, z3),
        ("z1 beyond its row", cts, s, a, c, at1(z1, z1[1] + (1 << 8192)), z2, z3),
    ]
