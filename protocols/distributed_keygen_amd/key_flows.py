"""The compositions of the private-key side — CRT decryption and encryption with the primes of N (private_key.py), the
prime search and the safe-prime search (primes.py) — over the engine's primitive entry points, written once: ``Engine``
inherits ``PrivateKeyFlows`` and runs them on the device; the Python-int doubles of the tests inherit it too and run the
SAME code over CPU tensors.

Nothing here launches anything itself or talks to the native library.  ``PrivateKeyFlows`` uses of ``self``:

  * ``torch``, ``device``, ``to_device``, ``_empty_rows`` and the flag ``_fixed_window``;
  * staging between ints and rows: ``_staged_rows``, ``_fetched_ints``, ``_download_ints``;
  * ``nsquare_plan`` (a plan prepared before the fan-out) and ``_crt_pair`` (the chains modulo p^2 and q^2, side by side
    or one after the other);
  * the primitives ``crt_split_t``, ``crt_recombine_t``, ``crt_prime_split_t``, ``crt_lift_t``, ``powmod_nsquare_t``,
    ``powmod_shared_t``, ``powmod_multi_t``, ``random_rows_t``, ``sieve_t``, ``safe_sieve_t``, ``safe_double_t``,
    ``miller_rabin_base2_t``, ``miller_rabin_t`` and ``generator_shares_t``

and joins them with plain torch calls.  The module itself imports neither torch nor the library."""

from __future__ import annotations

from typing import Any, List, Optional, Sequence, Tuple

from . import limbs as _limbs
from ._checks import RowChecks, _int_args, _nsquare


class PrivateKeyFlows(RowChecks):
    """The private-key compositions; see the module docstring for what a class that inherits them has to provide."""

    # ------------------------------------------------------------------ private-key (CRT) decryption
    @_int_args
    def private_decrypt_t(self, cts_t, p: int, q: int, packed: bool = False, side_by_side: bool = True):
        """Decryption with the primes of N: cts_t int32 [batch, limbs2] -> (plaintext rows, status) as crt_recombine_t
        returns them.  The split, ``powmod_nsquare_t(half[0], p, p - 1)`` and ``powmod_nsquare_t(half[1], q, q - 1)``
        — half-length exponents over half-width moduli, with this engine's plan cache, launch shapes and
        set_fixed_window — and the recombination.  `side_by_side`: the modexp modulo q^2 on a companion stream beside the
        one modulo p^2 — never slower than one after the other from 1 to 40 000 rows, 1.9 x faster for a lone ciphertext
        (DESIGN.md §4.21); False keeps everything on the caller's stream."""
        batch, limbs2 = cts_t.shape
        half_t = self.crt_split_t(cts_t, p, q)
        if batch == 0:
            return self.crt_recombine_t(half_t[0], half_t[1], p, q, packed=packed, limbs2=limbs2)
        self.nsquare_plan(p, p - 1)                # both prepared on the caller's stream, before the fan-out
        self.nsquare_plan(q, q - 1)
        xp_t, xq_t = self._crt_pair(lambda: self.powmod_nsquare_t(half_t[0], p, p - 1),
                                    lambda: self.powmod_nsquare_t(half_t[1], q, q - 1), side_by_side)
        return self.crt_recombine_t(xp_t, xq_t, p, q, packed=packed, limbs2=limbs2)

    @_int_args
    def private_decrypt_batch(self, cts: Sequence[int], p: int, q: int) -> Tuple[List[int], List[bool]]:
        """(messages, ok) of the ciphertexts `cts` (ints, taken modulo N^2) under the private key (p, q); ok[e] is False
        where c^(p-1) is not 1 modulo p or c^(q-1) not 1 modulo q — no valid ciphertext — and the message is 0 there.
        Page-locked staging both ways, as powmod_nsquare_batch."""
        if len(cts) == 0:
            return [], []
        n2, limbs2 = _nsquare(p * q)
        rows_t, status_t = self.private_decrypt_t(self._staged_rows("in", cts, limbs2, n2), p, q)
        status = status_t.cpu().numpy()
        return self._fetched_ints("messages", rows_t), [not bool(s) for s in status]

    # ------------------------------------------------------------------ private-key (CRT) encryption
    def _powmod_prime_t(self, rows_t, prime: int, exp: int):
        """rows^exp mod `prime` for a SECRET exponent (q mod (p-1) or p mod (q-1): whoever learns one factors N).
        ``powmod_shared_t`` follows a sliding-window schedule built on the host from the exponent's bits — the number and
        order of squarings and multiplications is a function of the exponent, in the class of the pair kernel's default
        tape.  With set_fixed_window(True) the launch goes through ``powmod_multi_t`` with one group instead: the generic
        kernel's fixed-window ladder, one multiplication behind every `window` squarings whatever the digit, so that the
        sequence of operations depends on the exponent's bit length only (the table row a window reads is still chosen
        by its digit).  Same results bit for bit."""
        if self._fixed_window:
            return self.powmod_multi_t(rows_t, [prime], [exp], rows_t.shape[0])
        return self.powmod_shared_t(rows_t, prime, exp)

    def _private_noise_halves(self, count: int, p: int, q: int, randomness_t, rng, draws_t, side_by_side: bool):
        """(rho_p rows, rho_q rows, the randomness rows they came from) for `count` ciphertexts: from the caller's r
        (``randomness_t``: prime split, a modexp modulo each prime, one modulo each square with the prime as exponent) or
        from fresh draws D of bits(N) + 64 bits (``rng``, or ``draws_t`` given: crt_split_t and the second modexp only)."""
        if (randomness_t is not None) + (rng is not None) + (draws_t is not None) != 1:
            raise ValueError("exactly one of randomness_t, rng and draws_t expected")
        self.nsquare_plan(p, p)                    # both prepared on the caller's stream, before the fan-out
        self.nsquare_plan(q, q)
        if randomness_t is not None:
            if randomness_t.dim() != 2 or randomness_t.shape[0] != count:
                raise ValueError("one randomness row per ciphertext expected")
            kept_t = randomness_t
            mod_t = self.crt_prime_split_t(randomness_t, p, q)
            e_p, e_q = q % (p - 1), p % (q - 1)
            run_p = lambda: self.powmod_nsquare_t(self._powmod_prime_t(mod_t[0], p, e_p), p, p)
            run_q = lambda: self.powmod_nsquare_t(self._powmod_prime_t(mod_t[1], q, e_q), q, q)
        else:
            if draws_t is None:
                n = p * q
                bits = n.bit_length() + 64
                draws_t = self.random_rows_t(rng, count, bits, max(_limbs.limbs_for(n * n), (bits + 31) // 32))
            elif draws_t.dim() != 2 or draws_t.shape[0] != count:
                raise ValueError("one draw per ciphertext expected")
            kept_t = draws_t
            mod_t = self.crt_split_t(draws_t, p, q)
            run_p = lambda: self.powmod_nsquare_t(mod_t[0], p, p)
            run_q = lambda: self.powmod_nsquare_t(mod_t[1], q, q)
        if count == 0:
            return mod_t[0], mod_t[1], kept_t
        rho_p_t, rho_q_t = self._crt_pair(run_p, run_q, side_by_side)
        return rho_p_t, rho_q_t, kept_t

    @_int_args
    def private_noise_t(self, count: int, p: int, q: int, randomness_t=None, rng=None, draws_t=None, side_by_side: bool = True,
                        packed: bool = False):
        """`count` rows of noise rho = r^N mod N^2 under the key with the primes p, q, and their status, as crt_lift_t
        returns them — for callers who keep a pool and multiply it in later (mulmod_t).  The randomness as in
        private_encrypt_t."""
        rho_p_t, rho_q_t, _ = self._private_noise_halves(count, p, q, randomness_t, rng, draws_t, side_by_side)
        return self.crt_lift_t(rho_p_t, rho_q_t, p, q, packed=packed)

    @_int_args
    def private_encrypt_t(self, messages_t, p: int, q: int, randomness_t=None, rng=None, draws_t=None, side_by_side: bool = True,
                          packed: bool = False, return_randomness: bool = False):
        """Paillier encryption by the holder of the primes of N: messages_t int32 [batch, >= limbs(N)] (m below N) ->
        (ciphertext rows [batch, limbs(N^2)], status) as crt_lift_t returns them, c = (1 + m N) r^N mod N^2.  Exactly one
        source of randomness:

        ``randomness_t`` [batch, any width]: the caller's r (only r mod N matters).  r^N modulo p^2 is
            ((r mod p)^(q mod (p-1)) mod p)^p — crt_prime_split_t, ``powmod_shared_t(.., p, q mod (p-1))`` (with
            set_fixed_window: ``powmod_multi_t`` with one group, _powmod_prime_t) and ``powmod_nsquare_t(.., p, p)`` — and
            likewise modulo q^2: bit for bit the ciphertext of ``encrypt_batch``.
        ``rng`` (device_rng.DeviceRng): one draw D of bits(N) + 64 bits per ciphertext; rho_p = (D mod p^2)^p and
            rho_q = (D mod q^2)^q are a uniform N-th residue (up to 2^-64) — the reference's distribution — at the cost
            of the second modexp alone.
        ``draws_t`` [batch, >= limbs(N^2)]: the draws D given, for reproducible runs.

        A row whose randomness shares a factor with N has a non-zero status and is zero.  `side_by_side`: the chain
        modulo q^2 on the companion stream of private_decrypt_t beside the one modulo p^2; False keeps everything on the
        caller's stream — 1.9 x slower for a lone ciphertext, and the faster call at ONE measured point: the caller's r at
        key_length 4096 and 10 000 rows (67.6 against 85.6 ms).  Both modes beat ``encrypt_batch``'s route at every
        measured point (1.3-2.4 x with the caller's r, 1.9-3.9 x fresh).  ``return_randomness``: a third result, the rows of r or D.  The modexps use this engine's plan
        cache and launch shapes.  All four exponents — p, q, q mod (p-1), p mod (q-1) — are secrets: by default every
        modexp follows a sliding-window schedule that is a function of its exponent's bits; set_fixed_window(True)
        reaches all four (the pair kernel's fixed-window tape and the generic kernel's fixed-window ladder), after which
        the sequence of operations depends on the exponents' bit lengths only, the table rows read still on their
        digits."""
        batch = messages_t.shape[0]
        rho_p_t, rho_q_t, kept_t = self._private_noise_halves(batch, p, q, randomness_t, rng, draws_t, side_by_side)
        out = self.crt_lift_t(rho_p_t, rho_q_t, p, q, messages_t=messages_t, packed=packed)
        if not return_randomness:
            return out
        return (out, kept_t) if packed else (*out, kept_t)

    @_int_args
    def private_randomize_t(self, cts_t, p: int, q: int, randomness_t=None, rng=None, draws_t=None, side_by_side: bool = True,
                            packed: bool = False, return_randomness: bool = False):
        """Re-randomisation c r^N mod N^2 by the holder of the primes: cts_t int32 [batch, >= limbs(N^2)] (any value of
        that width) -> (rows, status); the ciphertext enters through its halves (crt_split_t), everything else as
        private_encrypt_t."""
        batch = cts_t.shape[0]
        halves_t = self.crt_split_t(cts_t, p, q)
        rho_p_t, rho_q_t, kept_t = self._private_noise_halves(batch, p, q, randomness_t, rng, draws_t, side_by_side)
        out = self.crt_lift_t(rho_p_t, rho_q_t, p, q, halves_t=halves_t, packed=packed)
        if not return_randomness:
            return out
        return (out, kept_t) if packed else (*out, kept_t)

    def _private_batch(self, run_t, rows_t, count: int, p: int, q: int, randomness, rng, return_randomness: bool):
        if (randomness is None) == (rng is None):
            raise ValueError("exactly one of randomness and rng expected")
        if randomness is not None and len(randomness) != count:
            raise ValueError("one randomness per value expected")
        if count == 0:
            return ([], [], []) if return_randomness else ([], [])
        n = p * q
        r_t = None if randomness is None else self._staged_rows("randomness", randomness, _limbs.limbs_for(n), n)
        out_t, status_t, kept_t = run_t(rows_t(), p, q, randomness_t=r_t, rng=rng, return_randomness=True)
        status = status_t.cpu().numpy()
        out = self._fetched_ints("out", out_t), [not bool(s) for s in status]
        if not return_randomness:
            return out
        return (*out, list(randomness) if randomness is not None else self._download_ints(kept_t))

    @_int_args
    def private_encrypt_batch(self, messages: Sequence[int], p: int, q: int, randomness: Optional[Sequence[int]] = None, rng=None,
                              return_randomness: bool = False):
        """(ciphertexts, ok) of the `messages` (ints, taken modulo N: negative ones are their residues) under the key with
        the primes p, q — private_encrypt_t with page-locked staging both ways.  Exactly one of ``randomness`` (one r per
        message, taken modulo N) and ``rng``; ok[e] is False, and the ciphertext 0, where the randomness shares a factor
        with N.  ``return_randomness``: a third result, the r given or the draws D of the fresh mode."""
        n = p * q
        return self._private_batch(self.private_encrypt_t, lambda: self._staged_rows("in", messages, _limbs.limbs_for(n), n),
                                   len(messages), p, q, randomness, rng, return_randomness)

    @_int_args
    def private_randomize_batch(self, ciphertexts: Sequence[int], p: int, q: int, randomness: Optional[Sequence[int]] = None,
                                rng=None, return_randomness: bool = False):
        """(c r^N mod N^2 for every ciphertext, ok) — private_randomize_t at the int level; ciphertexts are taken modulo
        N^2, everything else as private_encrypt_batch."""
        n2, limbs2 = _nsquare(p * q)
        return self._private_batch(self.private_randomize_t, lambda: self._staged_rows("in", ciphertexts, limbs2, n2),
                                   len(ciphertexts), p, q, randomness, rng, return_randomness)

    # ------------------------------------------------------------------ Miller-Rabin and the prime search (primes.py)
    def _mr_candidates(self, cands_t, bits: Optional[int] = None, above: int = 3, checked: bool = False) -> Tuple[int, int, int]:
        """(rows, limbs, bits) of candidate rows for the strong-pseudoprime kernels.  ValueError — before anything of this
        library is launched — for rows of another shape, `bits` outside [2, 32 * limbs], an even candidate or one below
        `above` (a small host constant); device rows are read for that with two reductions unless the caller made the
        rows itself (`checked`)."""
        torch = self.torch
        rows, limbs = self._word_rows(cands_t, "candidates")
        bits = 32 * limbs if bits is None else int(bits)
        if not 2 <= bits <= 32 * limbs:
            raise ValueError("bits must lie in [2, 32 * limbs]")
        if rows and not checked:
            low = cands_t[:, 0]
            small = (low >= 0) & (low < above)
            if limbs > 1:
                small &= ~(cands_t[:, 1:] != 0).any(dim=1)
            word, rest = bits >> 5, bits & 31
            wide = torch.zeros_like(small)
            if rest:                                     # the bits of the top word above `bits`, then the words above it
                wide |= ((cands_t[:, word].to(torch.int64) & 0xFFFFFFFF) >> rest) != 0
                word += 1
            if word < limbs:
                wide |= (cands_t[:, word:] != 0).any(dim=1)
            if bool(((low & 1) == 0).any()) or bool(small.any()) or bool(wide.any()):
                raise ValueError(f"candidates must be odd, at least {above} and of at most `bits` bits")
        return rows, limbs, bits

    def probable_prime_t(self, cands_t, bits: int, rounds: int, rng, _checked: bool = False):
        """uint8 ``[S]``: 1 where the odd candidate (above primes.SIEVE_BOUND, at most `bits` bits) is a probable prime.
        Three stages, each on the rows the one before left, compacted by indexing in between: the sieve by the odd
        primes below primes.SIEVE_BOUND (it flags such a prime itself as well — ``primes.is_probable_prime_batch``
        decides small values on the host), the base 2 (miller_rabin_base2_t), and `rounds` rounds to random bases drawn
        by `rng` (ONE ``generator_shares_t`` draw of survivors * rounds rows, none when nothing is left), ANDed per
        candidate.  A prime always passes; a composite passes with probability at most 4^-rounds.  ValueError —
        nothing launched — for rounds < 1, an even or too small candidate or rows of another shape."""
        from . import primes as _primes

        rounds = int(rounds)
        if rounds < 1:
            raise ValueError("rounds must be at least 1")
        rows, limbs, bits = self._mr_candidates(cands_t, bits, above=_primes.SIEVE_BOUND, checked=_checked)
        torch = self.torch
        out_t = torch.zeros(rows, dtype=torch.uint8, device=self.device)
        if not rows:
            return out_t
        left = torch.nonzero(self.sieve_t(cands_t, _primes.sieve_primes()) == 0).flatten()
        if left.numel():
            left = left[self.miller_rabin_base2_t(cands_t[left].contiguous(), bits, _checked=True) != 0]
        if left.numel():
            self._random_rounds(cands_t, left, bits, rounds, rng, out_t)
        return out_t

    def _random_rounds(self, rows_t, left, bits: int, rounds: int, rng, out_t) -> None:
        """out_t[left] = the AND of `rounds` rounds to random bases on the candidates rows_t[left], at least one of them:
        ONE generator_shares_t draw of survivors * rounds rows, then miller_rabin_t."""
        kept_t = rows_t[left].contiguous()
        bases_t = self.generator_shares_t((kept_t, bits), rounds, rng=rng)
        passed = self.miller_rabin_t(kept_t, bases_t, rounds, bits=bits, _checked=True)
        out_t[left] = passed.view(-1, rounds).min(dim=1).values

    def _search(self, count: int, bits: int, rounds: int, batch: Optional[int], default_batch, draw, keep):
        """`count` rows ``[count, limbs]`` in draw order: ``keep(draw(batch, limbs))`` — the rows that a fresh batch
        yields — batch after batch while there are fewer.  `rounds` is only checked here.  ValueError — nothing
        launched — for count < 0, bits < 16, rounds < 1 or batch < 1."""
        count = int(count)
        if count < 0 or bits < 16 or rounds < 1:
            raise ValueError("count >= 0, bits >= 16 and rounds >= 1 expected")
        limbs = _limbs.limbs_for_bits(bits)
        if count == 0:
            return self._empty_rows(limbs)
        batch = default_batch(count, bits) if batch is None else int(batch)
        if batch < 1:
            raise ValueError("batch must be at least 1")
        found: List[Any] = []
        have = 0
        while have < count:
            found.append(keep(draw(batch, limbs)))
            have += int(found[-1].shape[0])
        return self.torch.cat(found)[:count].contiguous()

    @staticmethod
    def _force_bits(rows_t, bit_positions: Sequence[int]):
        for b in bit_positions:
            rows_t[:, b >> 5] |= (1 << (b & 31)) - ((1 << 32) if (b & 31) == 31 else 0)      # the bit as an int32
        return rows_t

    def prime_search_t(self, count: int, bits: int, rng, rounds: int = 64, batch: Optional[int] = None):
        """`count` random probable primes of exactly `bits` bits as rows ``[count, limbs]``: draw `batch` rows of `bits`
        bits from `rng`, set the two top bits and bit 0 (the product of two such primes has exactly 2 * bits bits), run
        probable_prime_t, keep the primes in draw order, and draw again while there are fewer than `count`.

        The default `batch` (primes.default_batch): primes have a share of at least 2 / (bits ln 2) among such odd
        numbers, so a batch holds about batch * 2 / (bits ln 2) of them, Poisson distributed; the default is the
        smallest multiple of 64 for which a batch falls short of `count` with probability at most 2 %.  ValueError —
        nothing launched — for count < 0, bits < 16 or rounds < 1."""
        from . import primes as _primes

        bits, rounds = int(bits), int(rounds)
        return self._search(
            count, bits, rounds, batch, _primes.default_batch,
            lambda batch, limbs: self._force_bits(rng.rows_t(self, batch, bits), (bits - 1, bits - 2, 0)),
            lambda rows_t: rows_t[self.probable_prime_t(rows_t, bits, rounds, rng, _checked=True) != 0])

    # ------------------------------------------------------------------ safe primes p = 2h + 1 (primes.py)
    def safe_prime_t(self, halves_t, bits: int, rounds: int, rng, _checked: bool = False, _stages: Optional[List[Any]] = None):
        """uint8 ``[S]``: 1 where p = 2h + 1 is a safe prime — h and p both prime — for rows of odd h above
        primes.SIEVE_BOUND of at most `bits` - 1 bits; `bits` is the width of p.  Four stages, each on the rows the one
        before left, compacted by indexing in between: the joint sieve by the odd primes below primes.SIEVE_BOUND
        (safe_sieve_t), the base 2 on h (miller_rabin_base2_t, bits - 1), safe_double_t and the base 2 on p (bits), and
        `rounds` rounds to random bases on h (ONE ``generator_shares_t`` draw of survivors * rounds rows, none when
        nothing is left), ANDed per candidate.

        The random rounds run on h only.  With h an odd prime, p = 2h + 1, 3 not dividing p (the sieve saw to it) and
        2^(p-1) = 1 mod p, Pocklington's theorem makes p prime: the proven factor F = h of p - 1 exceeds sqrt(p) and
        gcd(2^((p-1)/h) - 1, p) = gcd(3, p) = 1.  The round to the base 2 on p, with s = 1 and d = h, is that test
        (2^h = 1 or -1 implies 2^(p-1) = 1).  So a safe prime always passes, and any other input — one chosen to fool
        the test included — passes with probability at most 4^-rounds: a composite h survives the rounds with at most
        that probability, and a prime h makes the verdict on p exact.  `_stages`, a list, receives the indices each
        stage left.  ValueError — nothing launched — for rounds < 1, `bits` outside [3, 32 * limbs], an even or too
        small h, one of more than bits - 1 bits, or rows of another shape."""
        from . import primes as _primes

        rounds, bits = int(rounds), int(bits)
        if rounds < 1:
            raise ValueError("rounds must be at least 1")
        rows, limbs = self._word_rows(halves_t, "halves")
        if not 3 <= bits <= 32 * limbs:
            raise ValueError("bits must lie in [3, 32 * limbs]")
        self._mr_candidates(halves_t, bits - 1, above=_primes.SIEVE_BOUND, checked=_checked)
        torch = self.torch
        out_t = torch.zeros(rows, dtype=torch.uint8, device=self.device)
        left = torch.arange(0, device=self.device)
        if rows:
            left = torch.nonzero(self.safe_sieve_t(halves_t, _primes.sieve_primes()) == 0).flatten()
        stages = [left]
        if left.numel():
            left = left[self.miller_rabin_base2_t(halves_t[left].contiguous(), bits - 1, _checked=True) != 0]
        stages.append(left)
        if left.numel():
            full_t = self.safe_double_t(halves_t[left].contiguous(), _checked=True)
            left = left[self.miller_rabin_base2_t(full_t, bits, _checked=True) != 0]
        stages.append(left)
        if left.numel():
            self._random_rounds(halves_t, left, bits - 1, rounds, rng, out_t)
            left = left[out_t[left] != 0]
        stages.append(left)
        if _stages is not None:
            _stages.extend(stages)
        return out_t

    def safe_prime_search_t(self, count: int, bits: int, rng, rounds: int = 64, batch: Optional[int] = None):
        """`count` random safe primes p = 2h + 1 of exactly `bits` bits as rows ``[count, limbs]``, in draw order: draw
        `batch` rows h of bits - 1 bits from `rng`, set bits bits - 2, bits - 3 and 0 (p then has exactly `bits` bits
        with its two top bits set — the product of two such primes has exactly 2 * bits bits — and p = 3 mod 4), run
        safe_prime_t, keep 2h + 1 of what passes, and draw again while there are fewer than `count`.

        Safe primes are rare (primes.safe_prime_density: one odd h in about 190 000 at 1024 bits), so the default
        `batch` (primes.default_safe_batch) is NOT sized to hold `count` of them: it is the Poisson batch of
        primes.default_batch's rule from the safe-prime density, capped at primes.SAFE_BATCH_BYTES of rows per draw,
        and the search loops over batches until one completes `count`.  ValueError — nothing launched — for count < 0,
        bits < 16 or rounds < 1."""
        from . import primes as _primes

        bits, rounds = int(bits), int(rounds)
        return self._search(
            count, bits, rounds, batch, _primes.default_safe_batch,
            lambda batch, limbs: self._force_bits(rng.rows_t(self, batch, bits - 1, limbs), (bits - 2, bits - 3, 0)),
            lambda halves_t: self.safe_double_t(
                halves_t[self.safe_prime_t(halves_t, bits, rounds, rng, _checked=True) != 0].contiguous(), _checked=True))
