"""A Python-int double of the engine methods multiplication.py and secure_product.py drive — the new
``response_mod_rows_t`` / ``mul_prove_t`` / ``mul_verify_t`` and the existing entry points they are composed with — on
numpy rows.  ``mul_prove_t`` and ``mul_verify_t`` are COMPOSED here the way the engine composes them (the wide draws cut
and reduced, c_b^a and c_b^x as ONE multi-exponentiation over the count inputs c_b, u^N, v^N and gamma^N as ONE launch
on 3 count rows, five row sets hashed, the response modulo N with its quotient, the quotient as the exponent of
c_b mod N), so widths, layouts and the draw order are exercised; every step is Python ints and hashlib.  The response
modulo N runs the model's STEP-WISE form (tools/mul_model.py: response_mod_steps — the kernel word for word) and checks
it against divmod on every row.  It extends the double of the membership proofs.  Lives in tests/ only; the product never
imports it."""

from __future__ import annotations

import numpy as np

import mul_model as mulm
from member_engine import MemberEngine
from proof_engine import _rows
from range_engine import _wide

from protocols.distributed_keygen_amd import limbs
from protocols.distributed_keygen_amd.engine import Engine


class MulEngine(MemberEngine):
    mul_shape = staticmethod(Engine.mul_shape)
    response_mod_constants = staticmethod(Engine.response_mod_constants)

    def response_mod_rows_t(self, rho_t, e_t, x_t, mod, out_t=None):
        count, wn = rho_t.shape
        ew = e_t.shape[1]
        if x_t.shape != (count, wn) or e_t.shape[0] != count:
            raise ValueError("one challenge row and one secret row per rho row expected")
        if mod < 1 or limbs.limbs_for(mod) != wn:
            raise ValueError("a modulus of exactly the width of the rows expected")
        if out_t is not None and any(out_t is t for t in (rho_t, e_t, x_t)):
            raise ValueError("the output must not alias an input")
        assert self.response_mod_constants(mod, wn) == mulm.response_mod_constants(mod, wn)
        self.calls.append(("response_mod", count, wn, ew))
        ws, ts, status = [], [], []
        for rho, e, x in zip(limbs.unpack(rho_t), limbs.unpack(np.ascontiguousarray(e_t)), limbs.unpack(x_t)):
            w, t, st = mulm.response_mod_steps(rho, e, x, mod, wn, ew)
            q, r = divmod(rho + e * x, mod)
            assert (w, t, st) == (r, q & ((1 << (32 * ew)) - 1), int(q >> (32 * ew) != 0))
            ws.append(w), ts.append(t), status.append(st)
        return _rows(ws, wn), _rows(ts, ew), np.array(status, dtype=np.uint8)

    def _mul_challenge_t(self, ctx, ca_t, cb_t, d_t, a_t, b_t):
        return np.ascontiguousarray(self.sha256_rows_t(ctx, [ca_t, cb_t, d_t, a_t, b_t])[:, 4:8])

    def _reduce_n2_t(self, rows_t, n):
        ln = limbs.limbs_for(n)
        count = rows_t.shape[0]
        lo_t = np.ascontiguousarray(rows_t[:, :ln])
        hi_t = _wide(rows_t[:, ln:], ln)
        return self.response_mod_rows_t(lo_t, np.tile(_rows([(1 << (32 * ln)) % n], ln), (count, 1)), hi_t, n)[0]

    def mul_prove_t(self, ca_t, cb_t, a_t, ra_t, gamma_t, n, ctx, rng=None, draws=None):
        sh = self.mul_shape(n)
        ln, limbs2 = sh["limbs_n"], sh["limbs2"]
        count = ca_t.shape[0]
        if n < 3 or n % 2 == 0 or sh["draw_bits"] > (n * n).bit_length() - 1:
            raise ValueError("an odd N with room for the wide draws expected")
        if any(t.shape != (count, w) for t, w in ((ca_t, limbs2), (cb_t, limbs2), (a_t, ln), (ra_t, ln), (gamma_t, ln))):
            raise ValueError("rows of the wrong shape")
        if (rng is None) == (draws is None):
            raise ValueError("exactly one of rng and draws expected")
        if draws is None:
            draws = (rng.rows_t(self, count, sh["draw_bits"], limbs2), rng.rows_t(self, 2 * count, sh["draw_bits"], limbs2))
        xd_t, uv_t = draws
        if xd_t.shape != (count, limbs2) or uv_t.shape != (2 * count, limbs2):
            raise ValueError("one x draw and two further draws per statement expected")
        if any(a >= n for a in limbs.unpack(a_t)):
            raise ValueError("a must be below n")
        self.calls.append(("mul_prove", count))
        n2 = n * n
        x_t = self._reduce_wide_t(xd_t, n)
        cbn_t = self._reduce_n2_t(cb_t, n)
        rn_t = self.powmod_nsquare_t(np.concatenate([uv_t, _wide(gamma_t, limbs2)]), n, n)
        index_t = np.tile(np.arange(count, dtype=np.int32), 2).reshape(-1, 1)
        pw_t = self.multiexp_nsquare_rows_t(cb_t, index_t, np.concatenate([a_t, x_t]), 1, 32 * ln, n)
        d_t = self.mulmod_t(pw_t[:count], rn_t[2 * count:], n2)
        bb_t = self.mulmod_t(pw_t[count:], rn_t[count : 2 * count], n2)
        aa_t = self.mulmod_t(rn_t[:count], self._one_plus_mn_t(x_t, n), n2)
        e_t = self._mul_challenge_t(ctx, ca_t, cb_t, d_t, aa_t, bb_t)
        w_t, t_t, status = self.response_mod_rows_t(x_t, e_t, a_t, n)
        assert not status.any()
        uvn_t = self._reduce_wide_t(uv_t, n)
        z_t = self._own_pair_t(uvn_t[:count], ra_t, e_t, n)
        y_t = self._own_pair_t(self._own_pair_t(uvn_t[count:], cbn_t, t_t, n), gamma_t, e_t, n)
        return d_t, aa_t, bb_t, w_t, z_t, y_t

    def mul_verify_t(self, ca_t, cb_t, d_t, a_t, b_t, w_t, z_t, y_t, n, ctx):
        sh = self.mul_shape(n)
        ln, limbs2 = sh["limbs_n"], sh["limbs2"]
        count = ca_t.shape[0]
        wide, narrow = (ca_t, cb_t, d_t, a_t, b_t), (w_t, z_t, y_t)
        if any(t.shape != (count, limbs2) for t in wide) or any(t.shape != (count, ln) for t in narrow):
            raise ValueError("rows of the wrong shape")
        self.calls.append(("mul_verify", count))
        n2 = n * n
        ok = np.array([w < n for w in limbs.unpack(w_t)], dtype=bool)
        for r_t, bound in [(t, n2) for t in wide] + [(z_t, n), (y_t, n)]:
            ok &= np.array([0 < v < bound for v in limbs.unpack(r_t)], dtype=bool)

        def harmless(rows_t, value):
            return np.where(ok[:, None], rows_t, _rows([value], rows_t.shape[1])).astype(np.uint32)

        ca_t, cb_t, d_t, a_t, b_t, z_t, y_t = (harmless(t, 1) for t in (ca_t, cb_t, d_t, a_t, b_t, z_t, y_t))
        w_t = harmless(w_t, 0)
        e_t = self._mul_challenge_t(ctx, ca_t, cb_t, d_t, a_t, b_t)
        rn_t = self.powmod_nsquare_t(_wide(np.concatenate([z_t, y_t]), limbs2), n, n)
        own = np.arange(count, dtype=np.int32).reshape(-1, 1)
        left1_t = self.mulmod_t(rn_t[:count], self._one_plus_mn_t(w_t, n), n2)
        left2_t = self.mulmod_t(self.multiexp_nsquare_rows_t(cb_t, own, w_t, 1, 32 * ln, n), rn_t[count:], n2)
        right_t = self.multiexp_nsquare_rows_t(np.concatenate([a_t, b_t, ca_t, d_t]), self._own_pair_index(2 * count),
                                               self._one_and(np.concatenate([e_t, e_t])), 2, 128, n)
        return ok & (left1_t == right_t[:count]).all(axis=1) & (left2_t == right_t[count:]).all(axis=1)


def equations_hold(n, label, ca, cb, d, proof):
    """The verifier's two equations and nothing else — no range check: what a forgery must satisfy."""
    a_, b_, w, z, y = proof
    n2 = n * n
    e = mulm.challenge(mulm.context(n, label), ca, cb, d, a_, b_, mulm.limbs_for(n2))
    return ((1 + w * n) * pow(z, n, n2) % n2 == a_ * pow(ca, e, n2) % n2, pow(cb, w, n2) * pow(y, n, n2) % n2 == b_ * pow(d, e, n2) % n2)


def zero_forgeries(n, label, ca, cb, a, ra, alpha, gamma, draws):
    """(name, (A, B, w, z, y)) against the statement (c_a, c_b, d = c_b^alpha gamma^N) with alpha != a — a d that does NOT
    hold a b —, each satisfying BOTH equations.  Each equation alone is a sound proof of its own half: the second that
    d = c_b^alpha' rho^N for SOME alpha', the first that c_a holds SOME a'; what ties alpha' to a' is the shared w.
    A = z = 0 satisfies the first equation for any w, so the second half is run honestly with alpha; B = y = 0
    satisfies the second, so the first half is run honestly with a; and all zeros satisfy both.  Only the check
    0 < A, B, z, y refuses them."""
    n2 = n * n
    ctx, limbs2 = mulm.context(n, label), mulm.limbs_for(n2)
    d = mulm.product(n, cb, alpha, gamma)
    x, u, v = draws[0] % n, draws[1], draws[2]
    out = []
    b_ = pow(cb, x, n2) * pow(v, n, n2) % n2
    w, t = mulm.response_mod(x, mulm.challenge(ctx, ca, cb, d, 0, b_, limbs2), alpha, n)
    e = mulm.challenge(ctx, ca, cb, d, 0, b_, limbs2)
    out.append(("A = z = 0", (0, b_, w, 0, v % n * pow(cb % n, t, n) % n * pow(gamma % n, e, n) % n)))
    a_ = (1 + x * n) % n2 * pow(u, n, n2) % n2
    e = mulm.challenge(ctx, ca, cb, d, a_, 0, limbs2)
    out.append(("B = y = 0", (a_, 0, (x + e * a) % n, u % n * pow(ra % n, e, n) % n, 0)))
    out.append(("A = z = 0 and B = y = 0", (0, 0, x, 0, 0)))
    for name, proof in out:
        assert equations_hold(n, label, ca, cb, d, proof) == (True, True), name          # it WOULD pass
    return d, out


def tamperings(n, cols, ca, cb, d):
    """(name, c_a, c_b, d, A, B, w, z, y) with row 1 — and only row 1 — spoiled; every column a list of ints."""
    a_, b_, w, z, y = cols
    n2 = n * n

    def at1(vals, v):
        return list(vals[:1]) + [v] + list(vals[2:])

    return [
        ("d (1 + N)", ca, cb, at1(d, d[1] * (1 + n) % n2), a_, b_, w, z, y),
        ("c_a (1 + N)", at1(ca, ca[1] * (1 + n) % n2), cb, d, a_, b_, w, z, y),
        ("c_b (1 + N)", ca, at1(cb, cb[1] * (1 + n) % n2), d, a_, b_, w, z, y),
        ("A", ca, cb, d, at1(a_, a_[1] * (1 + n) % n2), b_, w, z, y),
        ("B", ca, cb, d, a_, at1(b_, (b_[1] + 1) % n2), w, z, y),
        ("w", ca, cb, d, a_, b_, at1(w, (w[1] + 1) % n), z, y),
        ("z", ca, cb, d, a_, b_, w, at1(z, z[1] * 2 % n), y),
        ("y", ca, cb, d, a_, b_, w, z, at1(y, (y[1] + 1) % n)),
        ("w >= N", ca, cb, d, a_, b_, at1(w, w[1] + n), z, y),
        ("z >= N", ca, cb, d, a_, b_, w, at1(z, z[1] + n), y),
        ("y >= N", ca, cb, d, a_, b_, w, z, at1(y, y[1] + n)),
        ("A >= N^2", ca, cb, d, at1(a_, a_[1] + n2), b_, w, z, y),
        ("B >= N^2", ca, cb, d, a_, at1(b_, b_[1] + n2), w, z, y),
        ("d >= N^2", ca, cb, at1(d, d[1] + n2), a_, b_, w, z, y),
        ("c_a >= N^2", at1(ca, ca[1] + n2), cb, d, a_, b_, w, z, y),
        ("c_b >= N^2", ca, at1(cb, cb[1] + n2), d, a_, b_, w, z, y),
        ("z = 0", ca, cb, d, a_, b_, w, at1(z, 0), y),
        ("y = 0", ca, cb, d, a_, b_, w, z, at1(y, 0)),
        ("negative", ca, cb, d, at1(a_, -a_[1]), b_, w, z, y),
        ("w beyond its row", ca, cb, d, a_, b_, at1(w, w[1] + (1 << (32 * limbs.limbs_for(n)))), z, y),
        ("z beyond its row", ca, cb, d, a_, b_, w, at1(z, z[1] + (1 << 8192)), y),
        ("no integer", ca, cb, d, a_, b_, w, z, at1(y, None)),
    ]
