"""A Python-int double of the engine PRIMITIVE multiplication.py and secure_product.py add — ``response_mod_rows_t`` — on
CPU ``int32`` tensors.  ``mul_prove_t`` and ``mul_verify_t`` are NOT written again here: the double runs the shipped
composition it inherits (``ProofFlows``: the wide draws cut and reduced, c_b^a and c_b^x as ONE multi-exponentiation over
the count inputs c_b, u^N, v^N and gamma^N as ONE launch on 3 count rows, five row sets hashed, the response modulo N
with its quotient, the quotient as the exponent of c_b mod N) over the primitives, so widths, layouts, the draw order and
the screening are the engine's own.  The response modulo N runs the model's STEP-WISE form (tools/mul_model.py:
response_mod_steps — the kernel word for word) and checks it against divmod on every row; its refusals and constants are
the engine's (``Engine.response_mod_constants``).  It extends the double of the membership proofs.  Lives in tests/ only;
the product never imports it."""

from __future__ import annotations

import mul_model as mulm
from member_engine import MemberEngine
from proof_engine import _flags_t, _ints, _rows_t

from protocols.distributed_keygen_amd import limbs
from protocols.distributed_keygen_amd.engine import Engine


class MulEngine(MemberEngine):
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
        for rho, e, x in zip(_ints(rho_t), _ints(e_t), _ints(x_t)):
            w, t, st = mulm.response_mod_steps(rho, e, x, mod, wn, ew)
            q, r = divmod(rho + e * x, mod)
            assert (w, t, st) == (r, q & ((1 << (32 * ew)) - 1), int(q >> (32 * ew) != 0))
            ws.append(w), ts.append(t), status.append(st)
        self.statuses.append(_flags_t(status))
        return _rows_t(ws, wn), _rows_t(ts, ew), self.statuses[-1]

    # ---- the shipped compositions, recorded
    def mul_prove_t(self, ca_t, *args, **kwargs):
        return self._proved(("mul_prove", ca_t.shape[0]), super().mul_prove_t, ca_t, *args, **kwargs)

    def mul_verify_t(self, ca_t, *args, **kwargs):
        self.calls.append(("mul_verify", ca_t.shape[0]))
        return super().mul_verify_t(ca_t, *args, **kwargs)


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
