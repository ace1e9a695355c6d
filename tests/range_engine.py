"""A Python-int double of the engine methods range_proof.py drives — the new ``multiexp_mod_t`` / ``response_rows_t`` /
``range_prove_t`` / ``range_verify_t`` and the existing entry points they are composed with — on numpy rows.
``range_prove_t`` and ``range_verify_t`` are COMPOSED here the way the engine composes them (products of two powers routed as the engine routes them — a shared-base
multi-exponentiation or one modexp per term —, the wide draw of rho cut at a word boundary and reduced by a multiply-add, challenge rows over
four row sets of two widths, per-row responses), so widths, layouts and the draw order are exercised; every step is
Python ints and hashlib.  It extends the double of the decryption proofs.  Lives in tests/ only; the product never
imports it."""

from __future__ import annotations

import numpy as np

from proof_engine import ProofEngine, _rows

from protocols.distributed_keygen_amd import limbs
from protocols.distributed_keygen_amd.engine import Engine


def _wide(rows_t, words):
    out = np.zeros((rows_t.shape[0], words), dtype=np.uint32)
    out[:, : rows_t.shape[1]] = rows_t
    return out


class RangeEngine(ProofEngine):
    range_shape = staticmethod(Engine.range_shape)

    # ---- existing entry points, in ints
    def encrypt_batch(self, messages, randomness, n):
        n2 = n * n
        self.calls.append(("encrypt", len(messages)))
        return [(1 + (m % n) * n) % n2 * pow(r, n, n2) % n2 for m, r in zip(messages, randomness)]

    def encrypt_fresh_batch(self, messages, n, rng, return_randomness=False):
        rs = limbs.unpack(rng.rows_t(self, len(messages), n.bit_length() + 64, limbs.limbs_for(n * n)))
        out = self.encrypt_batch(messages, rs, n)
        return (out, rs) if return_randomness else out

    def shamir_fma_t(self, a_t, b_t, c_t, prime, out_t=None):
        return _rows([(a * b + c) % prime for a, b, c in zip(limbs.unpack(a_t), limbs.unpack(b_t), limbs.unpack(c_t))], a_t.shape[1])

    # ---- the new entry points
    def multiexp_mod_t(self, inputs_t, index_t, weights_t, terms, weight_bits, mod, window=0, term_bits=None):
        if mod < 3 or mod % 2 == 0:
            raise ValueError("modulus must be odd and >= 3")
        if terms < 1 or not 1 <= weight_bits <= 16384:
            raise ValueError("terms >= 1 and weight_bits in 1 .. 16384 expected")          # the limit of mx_multiexp_run
        ww = (weight_bits + 31) // 32
        rows = index_t.shape[0]
        if tuple(index_t.shape) != (rows, terms) or weights_t.size != rows * terms * ww:
            raise ValueError("index [rows, terms] and weights of terms x ww words per row expected")
        xs = limbs.unpack(inputs_t)
        if rows and (int(index_t.min()) < 0 or int(index_t.max()) >= len(xs)):
            raise ValueError("index out of range")
        ws = limbs.unpack(np.ascontiguousarray(weights_t).reshape(rows * terms, ww))
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
        return _rows(out, inputs_t.shape[1])

    def response_rows_t(self, rho_t, e_t, x_t, out_t=None):
        wz = rho_t.shape[1]
        full = [r + e * x for r, e, x in zip(limbs.unpack(rho_t), limbs.unpack(e_t), limbs.unpack(x_t))]
        self.calls.append(("response_rows", len(full), wz, e_t.shape[1], x_t.shape[1]))
        return _rows([f & ((1 << (32 * wz)) - 1) for f in full], wz), np.array([1 if f >> (32 * wz) else 0 for f in full], dtype=np.uint8)

    range_uses_multiexp = classmethod(Engine.range_uses_multiexp.__func__)
    RANGE_MULTIEXP_MIN_BITS = Engine.RANGE_MULTIEXP_MIN_BITS

    def powmod_multi_t(self, bases_t, mods, exps, group_size, out_t=None):
        """Device pairs only: (modulus rows, bits) and (exponent rows, bits), one group per `group_size` rows."""
        (mods_t, mod_bits), (exps_t, exp_bits) = mods, exps
        ms, es = limbs.unpack(mods_t), limbs.unpack(np.ascontiguousarray(exps_t))
        if len(ms) != len(es) or len(bases_t) != len(ms) * group_size:
            raise ValueError("one modulus and one exponent per group expected")
        assert all(m.bit_length() <= mod_bits for m in ms) and all(e.bit_length() <= exp_bits for e in es)          # the caller's bounds
        self.calls.append(("powmod_multi", len(ms), group_size, exp_bits))
        return _rows([pow(b, es[k // group_size], ms[k // group_size]) for k, b in enumerate(limbs.unpack(bases_t))], bases_t.shape[1])

    def _shared_pair_t(self, base0, base1, w0_t, w1_t, mod, bits0, bits1, route=None):
        if bits1 > bits0:
            base0, base1, w0_t, w1_t, bits0, bits1 = base1, base0, w1_t, w0_t, bits1, bits0
        count = w0_t.shape[0]
        lm = limbs.limbs_for(mod)
        if route is None:
            route = "multiexp" if self.range_uses_multiexp(mod) else "modexps"
        if route == "modexps":
            mods = (np.tile(_rows([mod], lm), (count, 1)), mod.bit_length())
            p0 = self.powmod_multi_t(np.tile(_rows([base0 % mod], lm), (count, 1)), mods, (w0_t, bits0), 1)
            return self.mulmod_t(p0, self.powmod_multi_t(np.tile(_rows([base1 % mod], lm), (count, 1)), mods, (w1_t, bits1), 1), mod)
        ww = max(w0_t.shape[1], w1_t.shape[1])
        index_t = np.tile(np.array([[0, 1]], dtype=np.int32), (count, 1))
        weights_t = np.stack([_wide(w0_t, ww), _wide(w1_t, ww)], axis=1)
        return self.multiexp_mod_t(_rows([base0 % mod, base1 % mod], lm), index_t, weights_t, 2, 32 * ww, mod, term_bits=(bits0, bits1))

    def _own_pair_t(self, first_t, second_t, e_t, mod):
        count = e_t.shape[0]
        mods = (np.tile(_rows([mod], first_t.shape[1]), (count, 1)), mod.bit_length())
        return self.mulmod_t(first_t, self.powmod_multi_t(second_t, mods, (e_t, 32 * e_t.shape[1]), 1), mod)

    @staticmethod
    def _own_pair_index(count):
        own = np.arange(count, dtype=np.int32).reshape(-1, 1)
        return np.concatenate([own, own + count], axis=1)

    @staticmethod
    def _one_and(e_t):
        one_t = np.zeros_like(e_t)
        one_t[:, 0] = 1
        return np.stack([one_t, e_t], axis=1)

    def _one_plus_mn_t(self, m_t, n):
        count, limbs2 = m_t.shape[0], limbs.limbs_for(n * n)
        assert all(m < n for m in limbs.unpack(m_t))
        return self.shamir_fma_t(_wide(m_t, limbs2), np.tile(_rows([n], limbs2), (count, 1)), np.tile(_rows([1], limbs2), (count, 1)), n * n)

    def _reduce_wide_t(self, rows_t, n):
        ln = limbs.limbs_for(n)
        kw = (n.bit_length() - 1) // 32
        assert not rows_t[:, kw + 3 :].any()
        pow_t = np.tile(_rows([1 << (32 * kw)], ln), (rows_t.shape[0], 1))
        return self.shamir_fma_t(_wide(rows_t[:, kw : kw + 3], ln), pow_t, _wide(rows_t[:, :kw], ln), n)

    def _challenge_t(self, ctx, cts_t, s_t, a_t, c_t):
        return np.ascontiguousarray(self.sha256_rows_t(ctx, [cts_t, s_t, a_t, c_t])[:, 4:8])

    def range_prove_t(self, cts_t, messages_t, randomness_t, n, nh, s, t, bits, ctx, rng=None, draws=None, message_bits=None):
        sh = self.range_shape(n, nh, bits)
        message_bits = 32 * sh["z1_words"] if message_bits is None else int(message_bits)
        if not bits <= message_bits <= 32 * sh["z1_words"] or any(m >> message_bits for m in limbs.unpack(messages_t)):
            raise ValueError("message_bits in bits .. 32 z1_words that bounds every message expected")
        count = cts_t.shape[0]
        if (rng is None) == (draws is None):
            raise ValueError("exactly one of rng and draws expected")
        if cts_t.shape[1] != sh["limbs2"] or messages_t.shape != (count, sh["z1_words"]) or randomness_t.shape != (count, sh["limbs_n"]):
            raise ValueError("rows of the wrong shape")
        if draws is None:
            draws = (rng.rows_t(self, count, sh["alpha_bits"], sh["z1_words"]), rng.rows_t(self, count, sh["mu_bits"]),
                     rng.rows_t(self, count, sh["gamma_bits"], sh["z3_words"]), rng.rows_t(self, count, sh["rho_bits"], sh["limbs2"]))
        alpha_t, mu_t, gamma_t, rho_t = draws
        self.calls.append(("range_prove", count))
        s_t = self._shared_pair_t(s, t, messages_t, mu_t, nh, message_bits, sh["mu_bits"])
        c_t = self._shared_pair_t(s, t, alpha_t, gamma_t, nh, sh["alpha_bits"], sh["gamma_bits"])
        a_t = self.mulmod_t(self.powmod_nsquare_t(rho_t, n, n), self._one_plus_mn_t(alpha_t, n), n * n)
        e_t = self._challenge_t(ctx, cts_t, s_t, a_t, c_t)
        z1_t, _ = self.response_rows_t(alpha_t, e_t, messages_t)
        z3_t, _ = self.response_rows_t(gamma_t, e_t, mu_t)
        z2_t = self._own_pair_t(self._reduce_wide_t(rho_t, n), randomness_t, e_t, n)
        return s_t, a_t, c_t, z1_t, z2_t, z3_t

    def range_bounds_t(self, cts_t, s_t, a_t, c_t, z1_t, z2_t, z3_t, n, nh, bits):
        sh = self.range_shape(n, nh, bits)
        n2 = n * n
        ok = np.ones(cts_t.shape[0], dtype=bool)
        for r_t, bound in ((s_t, nh), (c_t, nh), (a_t, n2), (cts_t, n2), (z2_t, n), (z1_t, 1 << sh["z1_bits"]), (z3_t, 1 << sh["z3_bits"])):
            ok &= np.array([v < bound for v in limbs.unpack(r_t)], dtype=bool)
        return ok

    def range_verify_t(self, cts_t, s_t, a_t, c_t, z1_t, z2_t, z3_t, n, nh, s, t, bits, ctx):
        sh = self.range_shape(n, nh, bits)
        count = cts_t.shape[0]
        widths = (sh["limbs2"], sh["limbs_h"], sh["limbs2"], sh["limbs_h"], sh["z1_words"], sh["limbs_n"], sh["z3_words"])
        if any(r_t.shape != (count, w) for r_t, w in zip((cts_t, s_t, a_t, c_t, z1_t, z2_t, z3_t), widths)):
            raise ValueError("rows of the wrong shape")
        self.calls.append(("range_verify", count))
        n2 = n * n
        ok = self.range_bounds_t(cts_t, s_t, a_t, c_t, z1_t, z2_t, z3_t, n, nh, bits)

        def harmless(rows_t, value):
            return np.where(ok[:, None], rows_t, _rows([value], rows_t.shape[1])).astype(np.uint32)

        cts_t, s_t, a_t, c_t, z2_t = (harmless(r_t, 1) for r_t in (cts_t, s_t, a_t, c_t, z2_t))
        z1_t, z3_t = harmless(z1_t, 0), harmless(z3_t, 0)
        e_t = self._challenge_t(ctx, cts_t, s_t, a_t, c_t)
        left_t = self.mulmod_t(self.powmod_nsquare_t(_wide(z2_t, sh["limbs2"]), n, n), self._one_plus_mn_t(z1_t, n), n2)
        right_t = self.multiexp_nsquare_rows_t(np.concatenate([a_t, cts_t]), self._own_pair_index(count), self._one_and(e_t), 2, 128, n)
        left_h = self._shared_pair_t(s, t, z1_t, z3_t, nh, sh["z1_bits"], sh["z3_bits"])
        right_h = self._own_pair_t(c_t, s_t, e_t, nh)
        return ok & (left_t == right_t).all(axis=1) & (left_h == right_h).all(axis=1)


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
