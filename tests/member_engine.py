"""A Python-int double of the engine PRIMITIVES membership.py drives — ``member_challenges_t`` (its three modes) and
``modinv_t`` — on CPU ``int32`` tensors; every step is Python ints.  ``member_prove_t`` and ``member_verify_t`` are NOT
written again here: the double runs the shipped composition it inherits (``ProofFlows``: the draws for every slot, the
real slot masked and split by the three challenge modes, the branch rows c^-1 (1 + s_j N) from one inverse per
ciphertext, N-th powers of the count k wide rows joined to ONE multi-exponentiation of 128-bit weights, the k commitments
hashed as one row set, the real response placed by a slot mask) over these primitives, so widths, layouts, the draw order
and the screening are the engine's own.  It extends the double of the range proofs.  Lives in tests/ only; the product
never imports it."""

from __future__ import annotations

from proof_engine import _flags_t, _ints, _rows_t
from range_engine import RangeEngine

M128 = (1 << 128) - 1


class MemberEngine(RangeEngine):
    # ---- existing entry points, in ints
    def modinv_t(self, x_t, mod):
        self.calls.append(("modinv", len(x_t)))
        return _rows_t([pow(v, -1, mod) for v in _ints(x_t)], x_t.shape[1])          # (ValueError for a non-unit, as the engine)

    # ---- the primitive of the membership proofs
    def member_challenges_t(self, e_t, sim_t, index_t, mode, out_t=None):
        if mode not in (0, 1, 2):
            raise ValueError("mode 0 (mask), 1 (split) or 2 (sum) expected")
        count, words = sim_t.shape
        k = words // 4
        if words % 4 or not 2 <= k <= 16:
            raise ValueError("rows of 2 .. 16 slots of four words expected")
        if mode != 0 and tuple(e_t.shape) != (count, 4):
            raise ValueError("one challenge row per row of slots expected")
        slots = _ints(sim_t.reshape(count * k, 4))
        self.calls.append(("member_challenges", mode, count, k))
        if mode == 2:
            es = _ints(e_t)
            return _flags_t(sum(slots[r * k : (r + 1) * k]) & M128 != es[r] for r in range(count))
        if tuple(index_t.shape) != (count,):
            raise ValueError("an index [count] expected")
        index = [int(i) for i in index_t]
        if any(not 0 <= i < k for i in index):
            raise ValueError("index out of range")
        es = _ints(e_t) if mode == 1 else []
        out = []
        for r in range(count):
            row = [0 if j == index[r] else slots[r * k + j] for j in range(k)]
            if mode == 1:
                row[index[r]] = (es[r] - sum(row)) & M128
            out.extend(row)
        return _rows_t(out, 4).reshape(count, 4 * k)

    # ---- the shipped compositions, recorded
    def member_prove_t(self, cts_t, index_t, randomness_t, n, values, *args, **kwargs):
        return self._proved(("member_prove", cts_t.shape[0], len(values)), super().member_prove_t,
                            cts_t, index_t, randomness_t, n, values, *args, **kwargs)

    def member_verify_t(self, cts_t, a_t, e_t, z_t, n, values, ctx):
        self.calls.append(("member_verify", cts_t.shape[0], len(values)))
        return super().member_verify_t(cts_t, a_t, e_t, z_t, n, values, ctx)


def forgeries(n, values, label, c, seed=3):
    """(name, (a, e, z)) for ANY ciphertext c, made without a witness: zero satisfies 0^N = 0 u_j^(e_j) whatever c and e_j
    are.  All slots zero with the challenge put into slot 0; and one zero slot (each of the first and the last in turn)
    beside k - 1 honestly SIMULATED slots — z_j and e_j chosen, a_j = z_j^N u_j^(-e_j) — with the challenge re-split into
    the zero slot.  Every equation and the sum hold; only the check 0 < a_j, 0 < z_j refuses them."""
    import random

    import member_model as mm

    k, n2 = len(values), n * n
    ctx, limbs2 = mm.context(n, values, label), mm.limbs_for(n * n)
    us = mm.branches(n, values, c)
    out = [("every slot zero", ([0] * k, [mm.challenge(ctx, c, [0] * k, limbs2)] + [0] * (k - 1), [0] * k))]
    for slot in (0, k - 1):
        rnd = random.Random(seed + slot)
        zs = [0 if j == slot else rnd.randrange(1, n) for j in range(k)]
        es = [0 if j == slot else rnd.getrandbits(128) for j in range(k)]
        a = [0 if j == slot else pow(zs[j], n, n2) * pow(us[j], -es[j], n2) % n2 for j in range(k)]
        es[slot] = (mm.challenge(ctx, c, a, limbs2) - sum(es)) & M128
        assert sum(es) & M128 == mm.challenge(ctx, c, a, limbs2)
        assert all(pow(z, n, n2) == aj * pow(u, e, n2) % n2 for z, aj, u, e in zip(zs, a, us, es))          # it WOULD pass
        out.append((f"slot {slot} zero, the others simulated", (a, es, zs)))
    return out


def tamperings(n, values, proofs_ints, cts):
    """(name, cts, a, e, z) with row 1 — and only row 1 — spoiled; a, e, z are lists of k ints per row."""
    a, e, z = proofs_ints
    n2 = n * n

    def at1(col, j, v):
        row = list(col[1])
        row[j] = v
        return [col[0], row] + list(col[2:])

    def row1(col, row):
        return [col[0], row] + list(col[2:])

    e1 = e[1]
    swapped = [e1[1], e1[0]] + list(e1[2:])
    shifted = [(e1[0] + 1) & M128, (e1[1] - 1) & M128] + list(e1[2:])
    last = len(values) - 1
    out = [
        ("c (1 + N)", [cts[0], cts[1] * (1 + n) % n2] + list(cts[2:]), a, e, z),
        ("a_0", cts, at1(a, 0, a[1][0] * (1 + n) % n2), e, z),
        ("a_last", cts, at1(a, last, (a[1][last] + 1) % n2), e, z),
        ("z_0", cts, a, e, at1(z, 0, z[1][0] * 2 % n)),
        ("z_last", cts, a, e, at1(z, last, (z[1][last] + 1) % n)),
        ("z_j >= N", cts, a, e, at1(z, last, z[1][last] + n)),
        ("z_j = 0", cts, a, e, at1(z, 0, 0)),
        ("a_j = 0 and z_j = 0", cts, at1(a, last, 0), e, at1(z, last, 0)),
        ("a_j >= N^2", cts, at1(a, 0, a[1][0] + n2), e, z),
        ("c >= N^2", [cts[0], cts[1] + n2] + list(cts[2:]), a, e, z),
        ("two e_j swapped", cts, a, row1(e, swapped), z),
        ("e_0 + 1 and e_1 - 1", cts, a, row1(e, shifted), z),
    ]
    for word in range(4):
        out.append((f"a bit of word {word} of e_last", cts, a, at1(e, last, e1[last] ^ (1 << (32 * word + 5))), z))
    out += [
        ("negative", cts, at1(a, 0, -a[1][0]), e, z),
        ("e_j beyond its row", cts, a, at1(e, 0, e1[0] + (1 << 128)), z),
        ("a row of k - 1 entries", cts, a, e, row1(z, list(z[1][:-1]))),
    ]
    return out
