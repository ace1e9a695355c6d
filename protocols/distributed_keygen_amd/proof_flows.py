"""The compositions of the Sigma-protocols — decryption proofs (threshold.py), range proofs (range_proof.py), one-of-k
membership proofs (membership.py) and multiplication proofs (multiplication.py) — over the engine's primitive entry
points, written once: ``Engine`` inherits ``ProofFlows`` and runs them on the device; the Python-int doubles of the tests
inherit it too and run the SAME code over CPU tensors.

Nothing here launches anything itself or talks to the native library.  ``ProofFlows`` uses ``self.torch``,
``self.device``, ``self.to_device``, ``self._empty_rows`` and the public primitives (``powmod_nsquare_t``, ``mulmod_t``,
``multiexp_nsquare_rows_t``, ``multiexp_mod_t``, ``powmod_multi_t``, ``sha256_rows_t``, the three response kernels,
``member_challenges_t``, ``modinv_t``, ``shamir_fma_t``, the fixed-base tables) and joins them with plain torch calls.
The module itself imports neither torch nor the library (of ``_lib`` the constants only: nothing is loaded)."""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

from . import _lib, limbs as _limbs
from ._checks import RowChecks, _check_modulus, _check_rows_n2, _int_args

E_BITS = 128                     # challenge width
K_BITS = 128                     # statistical hiding margin


def range_shape(n: int, nh: int, bits: int) -> Dict[str, int]:
    """Bit lengths and row widths of a range proof (tools/range_model.py: shape).  ValueError unless
    1 <= bits and bits + 258 <= bits(n) - 1."""
    n, nh, bits = int(n), int(nh), int(bits)
    nb, hb = n.bit_length(), nh.bit_length()
    if bits < 1 or bits + E_BITS + K_BITS + 2 > nb - 1:
        raise ValueError(f"a claimed length of 1 .. bits(N) - 259 = {nb - 259} bits expected (l + E + K + 2 <= bits(N) - 1)")
    out = dict(alpha_bits=bits + E_BITS + K_BITS, mu_bits=hb + K_BITS, gamma_bits=hb + E_BITS + 2 * K_BITS, rho_bits=nb + 64)
    out.update(z1_bits=out["alpha_bits"] + 1, z3_bits=out["gamma_bits"] + 1)
    out.update(z1_words=(out["z1_bits"] + 31) // 32, z3_words=(out["z3_bits"] + 31) // 32, limbs_n=_limbs.limbs_for(n),
               limbs2=_limbs.limbs_for(n * n), limbs_h=_limbs.limbs_for(nh))
    return out


def member_shape(n: int, k: int) -> Dict[str, int]:
    """Bit lengths and row widths of a one-of-k proof (tools/member_model.py: shape).  ValueError unless 2 <= k <= 16."""
    n, k = int(n), int(k)
    if not _lib.MX_MEMBER_MIN_K <= k <= _lib.MX_MEMBER_MAX_K:
        raise ValueError(f"{_lib.MX_MEMBER_MIN_K} <= k <= {_lib.MX_MEMBER_MAX_K} expected")
    return dict(k=k, draw_bits=n.bit_length() + 64, e_bits=E_BITS, e_words=E_BITS // 32, limbs_n=_limbs.limbs_for(n),
                limbs2=_limbs.limbs_for(n * n))


def mul_shape(n: int) -> Dict[str, int]:
    """Bit lengths and row widths of a multiplication proof (tools/mul_model.py: shape)."""
    n = int(n)
    return dict(draw_bits=n.bit_length() + 64, e_bits=E_BITS, e_words=E_BITS // 32, limbs_n=_limbs.limbs_for(n),
                limbs2=_limbs.limbs_for(n * n))


class ProofFlows(RowChecks):
    """The prove and verify compositions of the four proofs and their helpers; see the module docstring for what a
    class that inherits them has to provide."""

    range_shape = staticmethod(range_shape)
    member_shape = staticmethod(member_shape)
    mul_shape = staticmethod(mul_shape)

    # ------------------------------------------------------------------ what the four proofs share
    def _expect_rows(self, expected, count: int, per: str = "ciphertext") -> None:
        """ValueError unless every (rows, what, words) of `expected` holds `count` rows of `words` words."""
        for rows_t, what, words in expected:
            if self._word_rows(rows_t, what, words)[0] != count:
                raise ValueError(f"one of the {what} per {per} expected")

    @staticmethod
    def _drawn(rng, draws, draw, what: str = "draws"):
        """The rows a test passed as `draws`, or what `draw()` takes from `rng`: exactly one of the two sources."""
        if (rng is None) == (draws is None):
            raise ValueError(f"exactly one of rng and {what} expected")
        return draw() if draws is None else draws

    def _event(self):
        ev = self.torch.cuda.Event(enable_timing=True)
        ev.record(self.torch.cuda.current_stream(self.device))
        return ev

    def _marker(self, stages: Optional[List[Any]]):
        """mark(name): appends (name, end event) to the list `stages` a probe passed; does nothing without one."""
        return (lambda name: None) if stages is None else (lambda name: stages.append((name, self._event())))

    def _challenge128_t(self, ctx: bytes, row_sets: Sequence[Any]):
        """The 128-bit challenge rows: the first 16 bytes of the digest are words 4 .. 7 of its row."""
        return self.sha256_rows_t(ctx, row_sets)[:, 4:8].contiguous()

    def _own_index(self, count: int):
        """index (r) as a column ``[count, 1]``: row r reads input r."""
        return self.torch.arange(count, device=self.device, dtype=self.torch.int32).view(-1, 1)

    def _harmless(self, ok, rows_t, value: int, slots: int = 1):
        """The rows of `rows_t` where the verdict `ok` (bool ``[count]``) holds and, where it does not, `value` (1, or 0 for
        an exponent) in each of the `slots` slots of the row: what a kernel may read whatever the prover sent."""
        torch = self.torch
        count = rows_t.shape[0]
        fill = torch.zeros((1, 1, rows_t.shape[1] // slots), dtype=torch.int32, device=self.device)
        fill[0, 0, 0] = value
        return torch.where(ok.view(-1, 1, 1), rows_t.view(count, slots, -1), fill).contiguous().view(count, -1)

    def _rows_below(self, rows_t, bound: int):
        """bool ``[count]``: the row, as a little-endian integer, is below `bound`."""
        torch = self.torch
        count, words = rows_t.shape
        if bound >> (32 * words):
            return torch.ones(count, dtype=torch.bool, device=self.device)
        vals = rows_t.to(torch.int64) & 0xFFFFFFFF
        lim = (self.to_device(_limbs.pack_one(bound, words).reshape(1, words)).to(torch.int64) & 0xFFFFFFFF)
        pos = torch.arange(1, words + 1, device=self.device, dtype=torch.int64)
        top = ((vals != lim) * pos).max(dim=1).values                  # 1 + the highest word that differs, 0 = equal
        return (top > 0) & torch.gather(vals < lim, 1, (top - 1).clamp(min=0).view(-1, 1)).view(-1)

    def _widened(self, rows_t, words: int):
        """The rows zero-extended to `words` words (a copy only when they are narrower)."""
        have = rows_t.shape[1]
        if have == words:
            return rows_t
        out_t = self.torch.zeros((rows_t.shape[0], words), dtype=self.torch.int32, device=self.device)
        out_t[:, :have] = rows_t
        return out_t

    def _term_weights(self, parts, ww: int):
        """[count, len(parts), ww] weights from one row tensor per term, each zero-extended to ww words."""
        return self.torch.stack([self._widened(p, ww) for p in parts], dim=1).contiguous()

    def _const_rows(self, values: Sequence[int], words: int):
        return self.to_device(_limbs.pack([int(v) for v in values], words).reshape(len(values), words))

    def _repeated_row(self, value: int, words: int, count: int):
        return self._const_rows([value], words).repeat(count, 1).contiguous()

    # ------------------------------------------------------------------ decryption proofs of a dealt threshold key (threshold.py)
    def _dleq_bases_t(self, cts_t, n: int, pieces: int, kw: int):
        """[chat^(2^(32 kw j)) for j < pieces], chat = c^4: squarings on the pair kernel, each from the one before."""
        out = [self.powmod_nsquare_t(cts_t, n, 4)]
        for _ in range(pieces - 1):
            out.append(self.powmod_nsquare_t(out[-1], n, 1 << (32 * kw)))
        return out

    def _dleq_powers_t(self, bases, exps_t, n: int, kw: int):
        """prod_j bases[j][r] ^ (piece j of exps[r]): chat^(exps[r]) in ONE multi-exponentiation launch whose weight block
        is the exponent rows themselves, read as [count][pieces][kw]."""
        torch = self.torch
        pieces, count = len(bases), exps_t.shape[0]
        index_t = (self._own_index(count) + count * torch.arange(pieces, device=self.device, dtype=torch.int32).view(1, -1)).contiguous()
        return self.multiexp_nsquare_rows_t(torch.cat(bases), index_t, exps_t, pieces, 32 * kw, n, _checked=True)

    def _dleq_fixed_t(self, v_bases: Sequence[int], exps_t, n: int, kw: int):
        """prod_j v_bases[j] ^ (piece j of exps[r]) through the fixed-base tables of the bases v^(2^(32 kw j))."""
        out_t = None
        for j, base in enumerate(v_bases):
            table = self.fixed_base_table(n, base, 32 * kw)
            piece_t = exps_t[:, j * kw : (j + 1) * kw].contiguous()
            out_t = self.fixed_base_power_t(table, piece_t) if out_t is None else self.fixed_base_randomize_t(table, piece_t, out_t)
        return out_t

    def _dleq_challenge_t(self, ctx: bytes, chat_t, ci2_t, a_t, b_t):
        """The 128-bit challenge rows: the first 16 bytes of the digest are words 4 .. 7 of its row."""
        return self._challenge128_t(ctx, [chat_t, ci2_t, a_t, b_t])

    @_int_args
    def dleq_prove_t(self, cts_t, partials_t, n: int, v_bases: Sequence[int], ctx: bytes, x_t, rho_bits: int, kw: int,
                     rng=None, rho_t=None, _stages: Optional[List[Any]] = None):
        """The proofs (a, b, z) that ``partials_t`` = c^(2x) were made with the exponent x behind w = v^x (threshold.py;
        tools/proof_model.py is the model): a = chat^rho, b = v^rho, e = H(ctx, chat, c_i^2, a, b), z = rho + e x, for
        chat = c^4 and one draw rho of ``rho_bits`` bits per row — from ``rng`` (a ``DeviceRng``), or the rows ``rho_t``
        a test passes.  Rows of rho and z are ``pieces = len(v_bases)`` pieces of ``kw`` words; ``v_bases`` are the public
        v^(2^(32 kw j)) mod n^2; ``x_t`` is the secret exponent as ONE device row.  Nothing per row leaves the device.
        Returns ``(a_t, b_t, z_t)``.  `_stages`, a list, receives (name, end event) pairs for tools/proof_probe.py."""
        count, limbs2 = self._word_rows(cts_t, "ciphertext rows")
        _check_modulus(n)
        _check_rows_n2(n, limbs2)
        if self._word_rows(partials_t, "partial rows", limbs2)[0] != count:
            raise ValueError("one partial decryption per ciphertext expected")
        pieces = len(v_bases)
        zw = pieces * kw
        if pieces < 1 or kw < 1 or 32 * kw > 2 * n.bit_length() + 64 or not 1 <= rho_bits < 32 * zw:
            raise ValueError("pieces of 1 .. (2 bits(n) + 64) / 32 words that hold rho_bits + 1 bits expected")
        rho_t = self._drawn(rng, rho_t, lambda: rng.rows_t(self, count, rho_bits, zw), "rho_t")
        if self._word_rows(rho_t, "rho rows", zw)[0] != count:
            raise ValueError("one rho row per ciphertext expected")
        mark = self._marker(_stages)
        mark("start")
        bases = self._dleq_bases_t(cts_t, n, pieces, kw)
        ci2_t = self.mulmod_t(partials_t, partials_t, n * n)
        mark("squarings")
        a_t = self._dleq_powers_t(bases, rho_t, n, kw)
        mark("multiexp")
        b_t = self._dleq_fixed_t(v_bases, rho_t, n, kw)
        mark("fixed_base")
        e_t = self._dleq_challenge_t(ctx, bases[0], ci2_t, a_t, b_t)
        mark("hash")
        z_t, _ = self.dleq_response_t(rho_t, e_t, x_t)        # (rho_bits + 1 <= 32 zw and e x < 2^rho_bits: it fits)
        mark("response")
        return a_t, b_t, z_t

    @_int_args
    def dleq_verify_t(self, cts_t, partials_t, a_t, b_t, z_t, n: int, v_bases: Sequence[int], w: int, ctx: bytes, z_bits: int,
                      kw: int, _stages: Optional[List[Any]] = None):
        """bool ``[count]``: row r is True iff a, b, c_i (and c) are below n^2, z below 2^z_bits, chat^z = a (c_i^2)^e and
        v^z = b w^e with e recomputed from the hash — the verdicts of the proofs of ``dleq_prove_t``, one per row; a bad
        row never raises.  Out-of-range rows are replaced by 1 (z by 0) before anything is computed from them.  No
        inverse of anything the prover sent is taken."""
        torch = self.torch
        count, limbs2 = self._word_rows(cts_t, "ciphertext rows")
        _check_modulus(n)
        _check_rows_n2(n, limbs2)
        pieces = len(v_bases)
        zw = pieces * kw
        if pieces < 1 or kw < 1 or 32 * kw > 2 * n.bit_length() + 64 or not 1 <= z_bits <= 32 * zw:
            raise ValueError("pieces of 1 .. (2 bits(n) + 64) / 32 words that hold z_bits bits expected")
        self._expect_rows(((partials_t, "partial rows", limbs2), (a_t, "a rows", limbs2), (b_t, "b rows", limbs2)), count)
        if self._word_rows(z_t, "z rows", zw)[0] != count:
            raise ValueError("one z row per ciphertext expected")
        if count == 0:
            return torch.ones(0, dtype=torch.bool, device=self.device)
        n2 = n * n
        ok = self._rows_below(z_t, 1 << z_bits)
        for t in (cts_t, partials_t, a_t, b_t):
            ok = ok & self._rows_below(t, n2)
        cts_t, partials_t, a_t, b_t = (self._harmless(ok, t, 1) for t in (cts_t, partials_t, a_t, b_t))
        z_t = self._harmless(ok, z_t, 0)
        mark = self._marker(_stages)
        mark("start")
        bases = self._dleq_bases_t(cts_t, n, pieces, kw)
        ci2_t = self.mulmod_t(partials_t, partials_t, n2)
        mark("squarings")
        e_t = self._dleq_challenge_t(ctx, bases[0], ci2_t, a_t, b_t)
        mark("hash")
        left_t = self._dleq_powers_t(bases, z_t, n, kw)
        right_t = self.mulmod_t(a_t, self.multiexp_nsquare_rows_t(ci2_t, self._own_index(count), e_t, 1, 128, n, _checked=True), n2)
        mark("multiexp")
        left_v = self._dleq_fixed_t(v_bases, z_t, n, kw)
        right_v = self.fixed_base_randomize_t(self.fixed_base_table(n, w, 128), e_t, b_t)
        mark("fixed_base")
        verdict = ok & (left_t == right_t).all(dim=1) & (left_v == right_v).all(dim=1)
        mark("compare")
        return verdict

    # ------------------------------------------------------------------ range proofs of ciphertexts (range_proof.py)
    # Which route a product of two powers of the range proofs takes (measured at 10 000 rows).  With SHARED
    # bases multiexp_kernel beats one modexp per term joined by a product from the 16-lane instances on (moduli above 2084
    # bits: 87.8 against 89.9 ms at 4096) and loses below (17.2 against 14.5 ms at 2048); with per-row bases and a 128-bit
    # exponent it loses at both lengths, so those products never take it.
    RANGE_MULTIEXP_MIN_BITS = 2085

    @classmethod
    def range_uses_multiexp(cls, mod: int) -> bool:
        """True iff the shared-base products modulo `mod` of the range proofs run through ``multiexp_mod_t``."""
        return int(mod).bit_length() >= cls.RANGE_MULTIEXP_MIN_BITS

    def _shared_pair_t(self, base0: int, base1: int, w0_t, w1_t, mod: int, bits0: int, bits1: int, route: Optional[str] = None):
        """base0^(w0[r]) * base1^(w1[r]) mod `mod` for weights below 2^bits0 and 2^bits1.  Route "multiexp": ONE
        ``multiexp_mod_t`` launch whose two tables every row shares, the longer term first and the windows above the shorter
        one skipping it.  Route "modexps": one ``powmod_multi_t`` per term — a group per row, the modulus row repeated — and
        ``mulmod_t`` to join them.  None: whichever measured faster at this length (``range_uses_multiexp``)."""
        if bits1 > bits0:
            base0, base1, w0_t, w1_t, bits0, bits1 = base1, base0, w1_t, w0_t, bits1, bits0
        count = w0_t.shape[0]
        lm = _limbs.limbs_for(mod)
        if route is None:
            route = "multiexp" if self.range_uses_multiexp(mod) else "modexps"
        if route == "modexps":
            mods = (self._repeated_row(mod, lm, count), mod.bit_length())
            out_t = self.powmod_multi_t(self._repeated_row(base0 % mod, lm, count), mods, (w0_t, bits0), 1)
            return self.mulmod_t(out_t, self.powmod_multi_t(self._repeated_row(base1 % mod, lm, count), mods, (w1_t, bits1), 1), mod, out_t=out_t)
        ww = max(w0_t.shape[1], w1_t.shape[1])
        index_t = self.torch.tensor([[0, 1]], dtype=self.torch.int32, device=self.device).repeat(count, 1).contiguous()
        return self.multiexp_mod_t(self._const_rows([base0 % mod, base1 % mod], lm), index_t, self._term_weights([w0_t, w1_t], ww), 2, 32 * ww,
                                   mod, term_bits=(bits0, bits1), _checked=True)

    def _own_pair_index(self, count: int):
        """index (r, count + r): row r of the first and of the second block of a two-block input tensor."""
        own = self._own_index(count)
        return self.torch.cat([own, own + count], dim=1).contiguous()

    def _one_and(self, e_t):
        """[count, 2, ew] weights (1, e[r])."""
        one_t = self.torch.zeros_like(e_t)
        one_t[:, 0] = 1
        return self._term_weights([one_t, e_t], e_t.shape[1])

    def _own_pair_t(self, first_t, second_t, e_t, mod: int, route: str = "modexps"):
        """first[r] * second[r]^(e[r]) mod `mod`, per-row bases.  Route "modexps" (what the proofs take: it measured faster
        at every length): ``powmod_multi_t`` with a group per row and ``mulmod_t``.  Route "multiexp": ONE ``multiexp_mod_t``
        launch, the 128-bit term first and the term of weight 1 confined to the lowest window."""
        torch = self.torch
        count, ew = e_t.shape
        if route == "modexps":
            mods = (self._repeated_row(mod, first_t.shape[1], count), mod.bit_length())
            return self.mulmod_t(first_t, self.powmod_multi_t(second_t, mods, (e_t, 32 * ew), 1), mod)
        one_t = torch.zeros_like(e_t)
        one_t[:, 0] = 1
        own = self._own_index(count)
        index_t = torch.cat([own + count, own], dim=1).contiguous()
        return self.multiexp_mod_t(torch.cat([first_t, second_t]), index_t, self._term_weights([e_t, one_t], ew), 2, 32 * ew,
                                   mod, term_bits=(32 * ew, 1), _checked=True)

    def _one_plus_mn_t(self, m_t, n: int):
        """1 + m[r] n as rows of the width of n^2, for m[r] below n — (1 + n)^m mod n^2 without an exponentiation: one
        multiply-add modulo n^2 (mx_fma_mod)."""
        count = m_t.shape[0]
        limbs2 = _limbs.limbs_for(n * n)
        return self.shamir_fma_t(self._widened(m_t, limbs2), self._repeated_row(n, limbs2, count), self._repeated_row(1, limbs2, count), n * n)

    def _reduce_wide_t(self, rows_t, n: int):
        """rows below 2^(bits(n) + 64) -> their residues modulo n as ``[count, limbs(n)]`` rows: the row is cut at the
        highest word boundary k below bits(n) (lo < 2^k < n, hi < 2^96) and hi * 2^k + lo goes through mx_fma_mod."""
        ln = _limbs.limbs_for(n)
        kw = (n.bit_length() - 1) // 32
        if kw < 1 or ln < 3 or rows_t.shape[1] < kw + 3:
            raise ValueError("a modulus of at least 96 bits expected")
        lo_t = self._widened(rows_t[:, :kw].contiguous(), ln)
        hi_t = self._widened(rows_t[:, kw : kw + 3].contiguous(), ln)
        pow_t = self._const_rows([1 << (32 * kw)], ln).repeat(rows_t.shape[0], 1).contiguous()
        return self.shamir_fma_t(hi_t, pow_t, lo_t, n)

    def _range_challenge_t(self, ctx: bytes, cts_t, s_t, a_t, c_t):
        """The 128-bit challenge rows over four row sets of two widths."""
        return self._challenge128_t(ctx, [cts_t, s_t, a_t, c_t])

    @_int_args
    def range_prove_t(self, cts_t, messages_t, randomness_t, n: int, nh: int, s: int, t: int, bits: int, ctx: bytes, rng=None,
                      draws=None, message_bits: Optional[int] = None, _stages: Optional[List[Any]] = None):
        """The proofs (S, A, C, z1, z2, z3) that the ciphertexts ``cts_t`` = (1 + n)^m r^n hold messages of ``bits``
        bits (range_proof.py; tools/range_model.py is the model): ``messages_t`` ``[count, z1_words]`` rows of m,
        ``randomness_t`` ``[count, limbs(n)]`` rows of r below n, (nh, s, t) the verifier's parameters.  The four
        draws alpha, mu, gamma, rho' come from ``rng`` (a ``DeviceRng``: four consecutive calls in this order) or are the
        rows ``draws`` a test passes.  ``message_bits``: a bound on the length of every message, ``bits`` .. 32 z1_words
        (default: the row width — the rows may hold messages beyond 2^bits, which the proof's slack admits); the modexp
        of the message term is as long as it says, and a message beyond it is a ValueError.  Nothing per row leaves the
        device.  `_stages`, a list, receives (name, end event) pairs for tools/range_proof_probe.py."""
        sh = self.range_shape(n, nh, bits)
        _check_modulus(nh)
        message_bits = 32 * sh["z1_words"] if message_bits is None else int(message_bits)
        if not bits <= message_bits <= 32 * sh["z1_words"]:
            raise ValueError("message_bits in bits .. 32 z1_words expected")
        count, _ = self._word_rows(cts_t, "ciphertext rows", sh["limbs2"])
        if self._word_rows(messages_t, "message rows", sh["z1_words"])[0] != count:
            raise ValueError("one message row per ciphertext expected")
        if self._word_rows(randomness_t, "randomness rows", sh["limbs_n"])[0] != count:
            raise ValueError("one randomness row per ciphertext expected")
        alpha_t, mu_t, gamma_t, rho_t = self._drawn(rng, draws, lambda: (
            rng.rows_t(self, count, sh["alpha_bits"], sh["z1_words"]), rng.rows_t(self, count, sh["mu_bits"]),
            rng.rows_t(self, count, sh["gamma_bits"], sh["z3_words"]), rng.rows_t(self, count, sh["rho_bits"], sh["limbs2"])))
        if count and message_bits < 32 * sh["z1_words"] and not bool(self._rows_below(messages_t, 1 << message_bits).all()):
            raise ValueError("a message is longer than message_bits")
        self._expect_rows(((alpha_t, "alpha rows", sh["z1_words"]), (mu_t, "mu rows", (sh["mu_bits"] + 31) // 32),
                           (gamma_t, "gamma rows", sh["z3_words"]), (rho_t, "rho rows", sh["limbs2"])), count)
        mark = self._marker(_stages)
        mark("start")
        s_t = self._shared_pair_t(s, t, messages_t, mu_t, nh, message_bits, sh["mu_bits"])
        c_t = self._shared_pair_t(s, t, alpha_t, gamma_t, nh, sh["alpha_bits"], sh["gamma_bits"])
        mark("multiexp_aux")
        a_t = self.powmod_nsquare_t(rho_t, n, n)
        mark("r_pow_n")
        a_t = self.mulmod_t(a_t, self._one_plus_mn_t(alpha_t, n), n * n, out_t=a_t)          # (alpha < 2^(bits + 256) < n)
        mark("multiexp_n2")
        e_t = self._range_challenge_t(ctx, cts_t, s_t, a_t, c_t)
        mark("hash")
        z1_t, _ = self.response_rows_t(alpha_t, e_t, messages_t)
        z3_t, _ = self.response_rows_t(gamma_t, e_t, mu_t)
        mark("response")
        z2_t = self._own_pair_t(self._reduce_wide_t(rho_t, n), randomness_t, e_t, n)
        mark("multiexp_n")
        return s_t, a_t, c_t, z1_t, z2_t, z3_t

    @_int_args
    def range_bounds_t(self, cts_t, s_t, a_t, c_t, z1_t, z2_t, z3_t, n: int, nh: int, bits: int):
        """bool ``[count]``: the range checks of ``range_verify_t`` — S, C < nh, A, c < n^2, z2 < n, z1 < 2^(bits + 257),
        z3 < 2^(bits(nh) + 385) — as row compares in torch; what fails them is never read by a kernel."""
        sh = self.range_shape(n, nh, bits)
        n2 = n * n
        return (self._rows_below(s_t, nh) & self._rows_below(c_t, nh) & self._rows_below(a_t, n2) & self._rows_below(cts_t, n2)
                & self._rows_below(z2_t, n) & self._rows_below(z1_t, 1 << sh["z1_bits"]) & self._rows_below(z3_t, 1 << sh["z3_bits"]))

    @_int_args
    def range_verify_t(self, cts_t, s_t, a_t, c_t, z1_t, z2_t, z3_t, n: int, nh: int, s: int, t: int, bits: int, ctx: bytes,
                       _stages: Optional[List[Any]] = None):
        """bool ``[count]``: row r is True iff S, C < nh, A, c < n^2, z2 < n, z1 < 2^(bits + 257), z3 < 2^(bits(nh) + 385),
        (1 + n)^z1 z2^n = A c^e (mod n^2) and s^z1 t^z3 = C S^e (mod nh) with e recomputed from the hash — the verdicts
        of the proofs of ``range_prove_t``, one per row; a bad row never raises.  Out-of-range rows are replaced by 1
        (z1 and z3 by 0) before anything is computed from them.  No inverse of anything the prover sent is taken."""
        torch = self.torch
        sh = self.range_shape(n, nh, bits)
        _check_modulus(nh)
        count, _ = self._word_rows(cts_t, "ciphertext rows", sh["limbs2"])
        self._expect_rows(((s_t, "S rows", sh["limbs_h"]), (a_t, "A rows", sh["limbs2"]), (c_t, "C rows", sh["limbs_h"]),
                           (z1_t, "z1 rows", sh["z1_words"]), (z2_t, "z2 rows", sh["limbs_n"]), (z3_t, "z3 rows", sh["z3_words"])), count)
        if count == 0:
            return torch.ones(0, dtype=torch.bool, device=self.device)
        n2 = n * n
        ok = self.range_bounds_t(cts_t, s_t, a_t, c_t, z1_t, z2_t, z3_t, n, nh, bits)
        cts_t, s_t, a_t, c_t, z2_t = (self._harmless(ok, r_t, 1) for r_t in (cts_t, s_t, a_t, c_t, z2_t))
        z1_t, z3_t = self._harmless(ok, z1_t, 0), self._harmless(ok, z3_t, 0)
        mark = self._marker(_stages)
        mark("start")
        e_t = self._range_challenge_t(ctx, cts_t, s_t, a_t, c_t)
        mark("hash")
        left_t = self.powmod_nsquare_t(self._widened(z2_t, sh["limbs2"]), n, n)
        mark("r_pow_n")
        left_t = self.mulmod_t(left_t, self._one_plus_mn_t(z1_t, n), n2, out_t=left_t)          # (z1 < 2^(bits + 257) < n past the range check)
        right_t = self.multiexp_nsquare_rows_t(torch.cat([a_t, cts_t]), self._own_pair_index(count), self._one_and(e_t), 2, 128, n, _checked=True)
        mark("multiexp_n2")
        left_h = self._shared_pair_t(s, t, z1_t, z3_t, nh, sh["z1_bits"], sh["z3_bits"])
        right_h = self._own_pair_t(c_t, s_t, e_t, nh)
        mark("multiexp_aux")
        verdict = ok & (left_t == right_t).all(dim=1) & (left_h == right_h).all(dim=1)
        mark("compare")
        return verdict

    # ------------------------------------------------------------------ one-of-k membership proofs (membership.py)
    def _member_values(self, n: int, values: Sequence[int]) -> Tuple[Dict[str, int], List[int]]:
        values = [int(s) for s in values]
        sh = self.member_shape(n, len(values))
        _check_modulus(n)
        if len(set(values)) != len(values) or any(not 0 <= s < n for s in values):
            raise ValueError("distinct values in [0, N) expected")
        return sh, values

    def _member_branches_t(self, rows_t, factors: Sequence[int], n: int):
        """rows[r] * (1 + factors[j] n) mod n^2 as ``[count k, limbs2]`` rows, row r k + j: the k branch rows of every
        ciphertext (or of its inverse) — the public factors through mx_fma_mod, the products through mx_mulmod."""
        k, count = len(factors), rows_t.shape[0]
        fac_t = self._one_plus_mn_t(self._const_rows(factors, _limbs.limbs_for(n)), n)
        return self.mulmod_t(rows_t.repeat_interleave(k, dim=0).contiguous(), fac_t.repeat(count, 1).contiguous(), n * n)

    def _member_challenge_t(self, ctx: bytes, cts_t, a_t):
        """The 128-bit challenge rows: c and the k commitments of a row as ONE row set of k limbs2 words."""
        return self._challenge128_t(ctx, [cts_t, a_t])

    @_int_args
    def member_prove_t(self, cts_t, index_t, randomness_t, n: int, values: Sequence[int], ctx: bytes, rng=None, draws=None,
                       _stages: Optional[List[Any]] = None):
        """The proofs (a, e, z) that the ciphertexts ``cts_t`` = (1 + n)^(values[index[r]]) r^n hold one of ``values``
        (membership.py; tools/member_model.py is the model): ``index_t`` int32 ``[count]`` in [0, k) — which value, the
        secret —, ``randomness_t`` ``[count, limbs(n)]`` rows of r below n.  The two draws — ``[count k, limbs(n^2)]``
        rows of bits(n) + 64 bits, then ``[count k, 4]`` rows of 128 bits, for EVERY slot — come from ``rng`` (a
        ``DeviceRng``: two consecutive calls in this order) or are the rows ``draws`` a test passes.  Returns
        ``(a_t [count, k limbs(n^2)], e_t [count, 4 k], z_t [count, k limbs(n)])``.  Every slot is treated alike: the
        real one is masked, split and placed by compare-and-select arithmetic (csrc/mx_member.hpp, ``torch.where`` over a
        slot mask), never by an address or a branch.  Nothing per row leaves the device.  ValueError if a ciphertext
        is no unit modulo n^2.  `_stages`, a list, receives (name, end event) pairs for tools/member_probe.py."""
        torch = self.torch
        sh, values = self._member_values(n, values)
        k, ln, limbs2 = sh["k"], sh["limbs_n"], sh["limbs2"]
        count, _ = self._word_rows(cts_t, "ciphertext rows", limbs2)
        if self._word_rows(randomness_t, "randomness rows", ln)[0] != count:
            raise ValueError("one randomness row per ciphertext expected")
        zt_t, et_t = self._drawn(rng, draws, lambda: (rng.rows_t(self, count * k, sh["draw_bits"], limbs2), rng.rows_t(self, count * k, 128)))
        if self._word_rows(zt_t, "z draws", limbs2)[0] != count * k or self._word_rows(et_t, "e draws", 4)[0] != count * k:
            raise ValueError("k draws of each kind per ciphertext expected")
        n2 = n * n
        mark = self._marker(_stages)
        mark("start")
        sim_t = self.member_challenges_t(None, et_t.view(count, 4 * k), index_t, _lib.MX_MEMBER_MASK)      # (the range of the index is checked here)
        if count == 0:
            return self._empty_rows(k * limbs2, 0), sim_t, self._empty_rows(k * ln, 0)
        mark("mask")
        ubar_t = self._member_branches_t(self.modinv_t(cts_t, n2), values, n)
        mark("branches")
        a_t = self.powmod_nsquare_t(zt_t, n, n)
        mark("r_pow_n")
        a_t = self.mulmod_t(a_t, self.multiexp_nsquare_rows_t(ubar_t, self._own_index(count * k), sim_t.view(count * k, 4), 1, 128, n, _checked=True),
                            n2, out_t=a_t)
        a_t = a_t.view(count, k * limbs2)
        mark("multiexp_n2")
        e_t = self.member_challenges_t(self._member_challenge_t(ctx, cts_t, a_t), sim_t, index_t, _lib.MX_MEMBER_SPLIT, out_t=sim_t)
        mark("hash_split")
        real = (torch.arange(k, device=self.device, dtype=torch.int32).view(1, k) == index_t.view(-1, 1)).view(count, k, 1)
        zero = torch.zeros((), dtype=torch.int32, device=self.device)

        def own_slot(rows_t):          # the real slot of every row, by mask and sum: no address depends on the index
            return torch.where(real, rows_t, zero).sum(dim=1, dtype=torch.int32).contiguous()

        zs_t = self._reduce_wide_t(zt_t, n).view(count, k, ln)
        zi_t = self._own_pair_t(own_slot(zs_t), randomness_t, own_slot(e_t.view(count, k, 4)), n)
        z_t = torch.where(real, zi_t.view(count, 1, ln), zs_t).contiguous().view(count, k * ln)
        mark("response")
        return a_t, e_t, z_t

    @_int_args
    def member_verify_t(self, cts_t, a_t, e_t, z_t, n: int, values: Sequence[int], ctx: bytes, _stages: Optional[List[Any]] = None):
        """bool ``[count]``: row r is True iff c < n^2, every 0 < a_j < n^2 and 0 < z_j < n, sum_j e_j = e (mod 2^128)
        with e recomputed from the hash, and z_j^n = a_j u_j^(e_j) (mod n^2) for every j, u_j = c (1 + (n - s_j) n) —
        the verdicts of the proofs of ``member_prove_t``, one per row; a bad row never raises.  ZERO is refused because
        a_j = z_j = 0 satisfies the equation for any c (a forgery without a witness); it is the only non-unit that needs
        a check when every prime factor of n exceeds 2^128 — any other would factor n.  Rows with a value out of range
        are replaced by 1 (their challenges by 0) before any kernel reads them.  No inverse of anything the prover sent
        is taken."""
        torch = self.torch
        sh, values = self._member_values(n, values)
        k, ln, limbs2 = sh["k"], sh["limbs_n"], sh["limbs2"]
        count, _ = self._word_rows(cts_t, "ciphertext rows", limbs2)
        self._expect_rows(((a_t, "a rows", k * limbs2), (e_t, "e rows", 4 * k), (z_t, "z rows", k * ln)), count)
        if count == 0:
            return torch.ones(0, dtype=torch.bool, device=self.device)
        n2 = n * n
        ok = (self._rows_below(cts_t, n2) & self._rows_below(a_t.view(count * k, limbs2), n2).view(count, k).all(dim=1)
              & self._rows_below(z_t.view(count * k, ln), n).view(count, k).all(dim=1))
        # zero is refused: a_j = z_j = 0 satisfies 0^n = 0 u_j^(e_j) for ANY c — a forgery without a witness
        ok = ok & (a_t.view(count, k, limbs2) != 0).any(dim=2).all(dim=1) & (z_t.view(count, k, ln) != 0).any(dim=2).all(dim=1)
        cts_t, a_t, z_t, e_t = self._harmless(ok, cts_t, 1), self._harmless(ok, a_t, 1, k), self._harmless(ok, z_t, 1, k), self._harmless(ok, e_t, 0, k)
        mark = self._marker(_stages)
        mark("start")
        split_ok = self.member_challenges_t(self._member_challenge_t(ctx, cts_t, a_t), e_t, None, _lib.MX_MEMBER_SUM) == 0
        mark("hash_sum")
        u_t = self._member_branches_t(cts_t, [(n - s) % n for s in values], n)
        mark("branches")
        left_t = self.powmod_nsquare_t(self._widened(z_t.view(count * k, ln), limbs2), n, n)
        mark("r_pow_n")
        right_t = self.multiexp_nsquare_rows_t(torch.cat([a_t.view(count * k, limbs2), u_t]), self._own_pair_index(count * k),
                                               self._one_and(e_t.view(count * k, 4)), 2, 128, n, _checked=True)
        mark("multiexp_n2")
        verdict = ok & split_ok & (left_t == right_t).view(count, k * limbs2).all(dim=1)
        mark("compare")
        return verdict

    # ------------------------------------------------------------------ multiplication proofs (multiplication.py)
    def _mul_shape_checked(self, n: int) -> Dict[str, int]:
        _check_modulus(n)
        sh = self.mul_shape(n)
        if sh["draw_bits"] > (n * n).bit_length() - 1 or n.bit_length() < 96:
            raise ValueError(f"a modulus of {n.bit_length()} bits leaves no room for 64 extra bits of randomness below n^2")
        return sh

    def _mul_challenge_t(self, ctx: bytes, ca_t, cb_t, d_t, a_t, b_t):
        """The 128-bit challenge rows over the five rows of the width of n^2."""
        return self._challenge128_t(ctx, [ca_t, cb_t, d_t, a_t, b_t])

    def _reduce_n2_t(self, rows_t, n: int):
        """rows below n^2 -> their residues modulo n, ``[count, limbs(n)]``: lo + 2^(32 limbs(n)) hi through the
        response modulo n — rho = lo, x = hi, e = 2^(32 limbs(n)) mod n — whose residue is right whatever lo and hi are."""
        ln = _limbs.limbs_for(n)
        count = rows_t.shape[0]
        lo_t = rows_t[:, :ln].contiguous()
        hi_t = self._widened(rows_t[:, ln:].contiguous(), ln) if rows_t.shape[1] > ln else self.torch.zeros_like(lo_t)
        return self.response_mod_rows_t(lo_t, self._repeated_row((1 << (32 * ln)) % n, ln, count), hi_t, n)[0]

    @_int_args
    def mul_prove_t(self, ca_t, cb_t, a_t, ra_t, gamma_t, n: int, ctx: bytes, rng=None, draws=None, _stages: Optional[List[Any]] = None):
        """(d, A, B, w, z, y): d = c_b^a gamma^n mod n^2 and the proof that it holds a b for the a inside
        c_a = (1 + n)^a r_a^n (multiplication.py; tools/mul_model.py is the model).  ``ca_t`` and ``cb_t``
        ``[count, limbs(n^2)]``, ``a_t`` (below n), ``ra_t`` and ``gamma_t`` ``[count, limbs(n)]``.  The draws — count rows
        of bits(n) + 64 bits at the width of n^2 for x, then 2 count such rows for u and v (all u first) — come from
        ``rng`` (a ``DeviceRng``: two consecutive calls in this order) or are the two row sets ``draws`` a test passes.
        c_b^a and c_b^x are ONE multi-exponentiation launch over the count inputs c_b (2 count rows, one table per
        input); u^n, v^n and gamma^n ONE launch of the r^n route on 3 count rows; (w, t) = divmod(x + e a, n) is the
        response kernel modulo n.  Nothing per row leaves the device.  ValueError for an a that is not below n.
        `_stages`, a list, receives (name, end event) pairs for tools/mul_probe.py."""
        torch = self.torch
        sh = self._mul_shape_checked(n)
        ln, limbs2 = sh["limbs_n"], sh["limbs2"]
        count, _ = self._word_rows(ca_t, "c_a rows", limbs2)
        self._expect_rows(((cb_t, "c_b rows", limbs2), (a_t, "a rows", ln), (ra_t, "r_a rows", ln), (gamma_t, "gamma rows", ln)), count, "statement")
        xd_t, uv_t = self._drawn(rng, draws, lambda: (rng.rows_t(self, count, sh["draw_bits"], limbs2),
                                                      rng.rows_t(self, 2 * count, sh["draw_bits"], limbs2)))
        if self._word_rows(xd_t, "x draws", limbs2)[0] != count or self._word_rows(uv_t, "u and v draws", limbs2)[0] != 2 * count:
            raise ValueError("one x draw and two further draws per statement expected")
        if count == 0:
            return (self._empty_rows(limbs2),) * 3 + (self._empty_rows(ln),) * 3
        if not bool(self._rows_below(a_t, n).all()):
            raise ValueError("a must be below n")
        n2 = n * n
        mark = self._marker(_stages)
        mark("start")
        x_t = self._reduce_wide_t(xd_t, n)
        cbn_t = self._reduce_n2_t(cb_t, n)
        mark("reduce")
        rn_t = self.powmod_nsquare_t(torch.cat([uv_t, self._widened(gamma_t, limbs2)]), n, n)          # u^n | v^n | gamma^n
        mark("r_pow_n")
        index_t = self._own_index(count).repeat(2, 1).contiguous()
        pw_t = self.multiexp_nsquare_rows_t(cb_t, index_t, torch.cat([a_t, x_t]), 1, 32 * ln, n, _checked=True)          # c_b^a | c_b^x
        d_t = self.mulmod_t(pw_t[:count], rn_t[2 * count:], n2)
        bb_t = self.mulmod_t(pw_t[count:], rn_t[count : 2 * count], n2)
        aa_t = self.mulmod_t(rn_t[:count], self._one_plus_mn_t(x_t, n), n2)
        mark("multiexp_n2")
        e_t = self._mul_challenge_t(ctx, ca_t, cb_t, d_t, aa_t, bb_t)
        mark("hash")
        w_t, t_t, _ = self.response_mod_rows_t(x_t, e_t, a_t, n)          # (x, a < n: the quotient fits the four words)
        mark("response")
        uvn_t = self._reduce_wide_t(uv_t, n)
        z_t = self._own_pair_t(uvn_t[:count], ra_t, e_t, n)
        y_t = self._own_pair_t(self._own_pair_t(uvn_t[count:], cbn_t, t_t, n), gamma_t, e_t, n)
        mark("multiexp_n")
        return d_t, aa_t, bb_t, w_t, z_t, y_t

    @_int_args
    def mul_verify_t(self, ca_t, cb_t, d_t, a_t, b_t, w_t, z_t, y_t, n: int, ctx: bytes, _stages: Optional[List[Any]] = None):
        """bool ``[count]``: row r is True iff 0 < c_a, c_b, d, A, B < n^2, w < n, 0 < z, y < n,
        (1 + w n) z^n = A c_a^e and c_b^w y^n = B d^e (mod n^2) with e recomputed from the hash — the verdicts of the
        proofs of ``mul_prove_t``, one per row; a bad row never raises.  ZERO is refused: A = z = 0 satisfies the first
        equation and B = y = 0 the second for any statement.  Rows with a value out of range are replaced by 1 (w by 0)
        before any kernel reads them.  No inverse of anything the prover sent is taken."""
        torch = self.torch
        sh = self._mul_shape_checked(n)
        ln, limbs2 = sh["limbs_n"], sh["limbs2"]
        count, _ = self._word_rows(ca_t, "c_a rows", limbs2)
        self._expect_rows(((cb_t, "c_b rows", limbs2), (d_t, "d rows", limbs2), (a_t, "A rows", limbs2), (b_t, "B rows", limbs2),
                           (w_t, "w rows", ln), (z_t, "z rows", ln), (y_t, "y rows", ln)), count, "statement")
        if count == 0:
            return torch.ones(0, dtype=torch.bool, device=self.device)
        n2 = n * n
        ok = self._rows_below(w_t, n)
        for r_t, bound in ((ca_t, n2), (cb_t, n2), (d_t, n2), (a_t, n2), (b_t, n2), (z_t, n), (y_t, n)):
            ok = ok & self._rows_below(r_t, bound) & (r_t != 0).any(dim=1)          # zero is refused
        ca_t, cb_t, d_t, a_t, b_t, z_t, y_t = (self._harmless(ok, r_t, 1) for r_t in (ca_t, cb_t, d_t, a_t, b_t, z_t, y_t))
        w_t = self._harmless(ok, w_t, 0)
        mark = self._marker(_stages)
        mark("start")
        e_t = self._mul_challenge_t(ctx, ca_t, cb_t, d_t, a_t, b_t)
        mark("hash")
        rn_t = self.powmod_nsquare_t(self._widened(torch.cat([z_t, y_t]), limbs2), n, n)          # z^n | y^n
        mark("r_pow_n")
        left1_t = self.mulmod_t(rn_t[:count], self._one_plus_mn_t(w_t, n), n2)
        left2_t = self.mulmod_t(self.multiexp_nsquare_rows_t(cb_t, self._own_index(count), w_t, 1, 32 * ln, n, _checked=True), rn_t[count:], n2)
        right_t = self.multiexp_nsquare_rows_t(torch.cat([a_t, b_t, ca_t, d_t]), self._own_pair_index(2 * count),
                                               self._one_and(torch.cat([e_t, e_t])), 2, 128, n, _checked=True)          # A c_a^e | B d^e
        mark("multiexp_n2")
        verdict = ok & (left1_t == right_t[:count]).all(dim=1) & (left2_t == right_t[count:]).all(dim=1)
        mark("compare")
        return verdict
