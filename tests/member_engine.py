"""A Python-int double of the engine methods membership.py drives — the new ``member_challenges_t`` / ``member_prove_t`` /
``member_verify_t`` and the existing entry points they are composed with — on numpy rows.  ``member_prove_t`` and
``member_verify_t`` are COMPOSED here the way the engine composes them (the draws for every slot, the real slot masked
and split by the three challenge modes, the branch rows c^-1 (1 + s_j N) from one inverse per ciphertext, N-th powers of
the count k wide rows joined to ONE multi-exponentiation of 128-bit weights, the k commitments hashed as one row set,
the real response placed by a slot mask), so widths, layouts and the draw order are exercised; every step is Python
ints and hashlib.  The three challenge modes are Python ints.  It extends the double of the range proofs.  Lives in
tests/ only; the product never imports it."""

from __future__ import annotations

import numpy as np

from proof_engine import _rows
from range_engine import RangeEngine, _wide

from protocols.distributed_keygen_amd import limbs
from protocols.distributed_keygen_amd.engine import Engine

M128 = (1 << 128) - 1


class MemberEngine(RangeEngine):
    member_shape = staticmethod(Engine.member_shape)

    # ---- existing entry points, in ints
    def modinv_t(self, x_t, mod):
        self.calls.append(("modinv", len(x_t)))
        return _rows([pow(v, -1, mod) for v in limbs.unpack(x_t)], x_t.shape[1])          # (ValueError for a non-unit, as the engine)

    # ---- the new entry points
    def member_challenges_t(self, e_t, sim_t, index_t, mode, out_t=None):
        if mode not in (0, 1, 2):
            raise ValueError("mode 0 (mask), 1 (split) or 2 (sum) expected")
        count, words = sim_t.shape
        k = words // 4
        if words % 4 or not 2 <= k <= 16:
            raise ValueError("rows of 2 .. 16 slots of four words expected")
        if mode != 0 and tuple(e_t.shape) != (count, 4):
            raise ValueError("one challenge row per row of slots expected")
        slots = limbs.unpack(np.ascontiguousarray(sim_t).reshape(count * k, 4))
        self.calls.append(("member_challenges", mode, count, k))
        if mode == 2:
            es = limbs.unpack(e_t)
            return np.array([int(sum(slots[r * k : (r + 1) * k]) & M128 != es[r]) for r in range(count)], dtype=np.uint8)
        if tuple(index_t.shape) != (count,):
            raise ValueError("an index [count] expected")
        index = [int(i) for i in index_t]
        if any(not 0 <= i < k for i in index):
            raise ValueError("index out of range")
        out = []
        for r in range(count):
            row = [0 if j == index[r] else slots[r * k + j] for j in range(k)]
            if mode == 1:
                row[index[r]] = (limbs.unpack(e_t[r : r + 1])[0] - sum(row)) & M128
            out.extend(row)
        return _rows(out, 4).reshape(count, 4 * k)

    def _member_values(self, n, values):
        values = [int(s) for s in values]
        sh = self.member_shape(n, len(values))
        if n < 3 or n % 2 == 0 or len(set(values)) != len(values) or any(not 0 <= s < n for s in values):
            raise ValueError("an odd N and distinct values in [0, N) expected")
        return sh, values

    def _member_branches_t(self, rows_t, factors, n):
        k, count = len(factors), rows_t.shape[0]
        fac_t = self._one_plus_mn_t(_rows(factors, limbs.limbs_for(n)), n)
        return self.mulmod_t(np.repeat(rows_t, k, axis=0), np.tile(fac_t, (count, 1)), n * n)

    def _member_challenge_t(self, ctx, cts_t, a_t):
        return np.ascontiguousarray(self.sha256_rows_t(ctx, [cts_t, a_t])[:, 4:8])

    def member_prove_t(self, cts_t, index_t, randomness_t, n, values, ctx, rng=None, draws=None):
        sh, values = self._member_values(n, values)
        k, ln, limbs2 = sh["k"], sh["limbs_n"], sh["limbs2"]
        count = cts_t.shape[0]
        if cts_t.shape[1] != limbs2 or randomness_t.shape != (count, ln):
            raise ValueError("rows of the wrong shape")
        if (rng is None) == (draws is None):
            raise ValueError("exactly one of rng and draws expected")
        if draws is None:
            draws = (rng.rows_t(self, count * k, sh["draw_bits"], limbs2), rng.rows_t(self, count * k, 128))
        zt_t, et_t = draws
        if zt_t.shape != (count * k, limbs2) or et_t.shape != (count * k, 4):
            raise ValueError("k draws of each kind per ciphertext expected")
        self.calls.append(("member_prove", count, k))
        n2 = n * n
        sim_t = self.member_challenges_t(None, et_t.reshape(count, 4 * k), index_t, 0)
        ubar_t = self._member_branches_t(self.modinv_t(cts_t, n2), values, n)
        own = np.arange(count * k, dtype=np.int32).reshape(-1, 1)
        a_t = self.mulmod_t(self.powmod_nsquare_t(zt_t, n, n), self.multiexp_nsquare_rows_t(ubar_t, own, sim_t.reshape(count * k, 4), 1, 128, n), n2)
        a_t = a_t.reshape(count, k * limbs2)
        e_t = self.member_challenges_t(self._member_challenge_t(ctx, cts_t, a_t), sim_t, index_t, 1)
        real = (np.arange(k).reshape(1, k) == index_t.astype(np.int64).reshape(-1, 1)).reshape(count, k, 1)

        def own_slot(rows_t):
            return np.where(real, rows_t, 0).sum(axis=1).astype(np.uint32)

        zs_t = self._reduce_wide_t(zt_t, n).reshape(count, k, ln)
        zi_t = self._own_pair_t(own_slot(zs_t), randomness_t, own_slot(e_t.reshape(count, k, 4)), n)
        z_t = np.where(real, zi_t.reshape(count, 1, ln), zs_t).astype(np.uint32).reshape(count, k * ln)
        return a_t, e_t, z_t

    def member_verify_t(self, cts_t, a_t, e_t, z_t, n, values, ctx):
        sh, values = self._member_values(n, values)
        k, ln, limbs2 = sh["k"], sh["limbs_n"], sh["limbs2"]
        count = cts_t.shape[0]
        if any(r_t.shape != (count, w) for r_t, w in ((cts_t, limbs2), (a_t, k * limbs2), (e_t, 4 * k), (z_t, k * ln))):
            raise ValueError("rows of the wrong shape")
        self.calls.append(("member_verify", count, k))
        n2 = n * n

        def below(rows_t, words, bound):
            return np.array([v < bound for v in limbs.unpack(np.ascontiguousarray(rows_t).reshape(-1, words))], dtype=bool).reshape(count, -1).all(axis=1)

        ok = below(cts_t, limbs2, n2) & below(a_t, limbs2, n2) & below(z_t, ln, n)
        ok &= (a_t.reshape(count, k, limbs2) != 0).any(axis=2).all(axis=1) & (z_t.reshape(count, k, ln) != 0).any(axis=2).all(axis=1)

        def harmless(rows_t, slots, value):
            fill = _rows([value], rows_t.shape[1] // slots).reshape(1, 1, -1)
            return np.where(ok.reshape(-1, 1, 1), rows_t.reshape(count, slots, -1), fill).astype(np.uint32).reshape(count, -1)

        cts_t, a_t, z_t, e_t = harmless(cts_t, 1, 1), harmless(a_t, k, 1), harmless(z_t, k, 1), harmless(e_t, k, 0)
        split_ok = self.member_challenges_t(self._member_challenge_t(ctx, cts_t, a_t), e_t, None, 2) == 0
        u_t = self._member_branches_t(cts_t, [(n - s) % n for s in values], n)
        left_t = self.powmod_nsquare_t(_wide(z_t.reshape(count * k, ln), limbs2), n, n)
        right_t = self.multiexp_nsquare_rows_t(np.concatenate([a_t.reshape(count * k, limbs2), u_t]), self._own_pair_index(count * k),
                                               self._one_and(e_t.reshape(count * k, 4)), 2, 128, n)
        return ok & split_ok & (left_t == right_t).reshape(count, k * limbs2).all(axis=1)


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
