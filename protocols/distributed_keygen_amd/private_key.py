"""Decryption and encryption with an ordinary Paillier private key — the primes p and q of N — on the GPU engine.

The decrypting party of gradient-boosted trees, vertical logistic regression or encrypted scoring usually holds a plain
key, not a threshold share.  Knowing p and q allows the CRT decryption of Paillier 1999, section 7:

    x_p = (c mod p^2)^(p-1) mod p^2      m_p = L_p(x_p) h_p mod p       L_p(x) = (x - 1) / p
    x_q = (c mod q^2)^(q-1) mod q^2      m_q = L_q(x_q) h_q mod q
    m   = m_p + p ((m_q - m_p) p^-1 mod q)
    h_p = L_p((N + 1)^(p-1) mod p^2)^-1 mod p,  h_q likewise

two modexps with half-length exponents over half-width moduli (``Engine.private_decrypt_t``: both moduli are squares,
so they run on the pair kernel of the partial decryption) instead of one full-width modexp with an exponent as long as N.
The plaintext rows have the format of ``Engine.combine_t``: ``slots.decode_t`` and ``packing.unpack`` take them as they
are.

The status.  A row's status is non-zero when c^(p-1) is not 1 modulo p (bit 0) or c^(q-1) not 1 modulo q (bit 1).  For a
prime p that happens exactly when p divides c: the status detects ciphertexts that share a factor with N (0, multiples of
p or q) and nothing else.  Every c coprime to N is a valid ciphertext of SOME plaintext, so a corrupted or foreign
ciphertext decrypts, without a status, to a wrong plaintext — as it does in every Paillier implementation.  With a
composite "prime" the status fires for most ciphertexts.  Neither decryption nor the constructor tests primality:
``PaillierPrivateKey.check_primes`` does (a batched Miller-Rabin test on the device, primes.py), and
``PaillierPrivateKey.generate`` makes a key from primes found by it.

Side channels.  The exponents p - 1 and q - 1 are the secret.  By default the modexps follow a sliding-window tape
that is a function of the exponent's bits, and the table row a window reads is chosen by its digits: timing and table
addresses depend on p and q, in the same class as gmpy2's ``mpz_powm``.  ``Engine.set_fixed_window(True)`` makes the
sequence of operations depend on the bit lengths only (the table rows read still depend on the digits); it applies to
both plans.  The plan cache of the engine holds constants derived from p and q in device memory for as long as the
engine keeps the plan.

Encryption.  The same party encrypts far more often than it decrypts (the label holder of gradient-boosted trees
encrypts (g, h) of every sample in every round), and the factors shorten that too.  Z*_{p^2} = C_{p-1} x C_p, and
x -> x^p mod p^2 depends on x mod p only and is multiplicative in it, so the reference's noise r^N mod N^2 is, modulo p^2,

    s_p   = (r mod p)^(q mod (p-1)) mod p                 one modexp modulo p, half-length exponent
    rho_p = s_p^p mod p^2                                 one modexp modulo p^2 with the exponent p (the decryption's shape)

and likewise modulo q^2; with v = 1 + m N (encryption), v = c (re-randomisation) or v = 1 (noise alone)

    c_p = v rho_p mod p^2,   c_q = v rho_q mod q^2,   c = c_p + p^2 ((c_q - c_p) (p^2)^-1 mod q^2)

is bit for bit the ciphertext ``Engine.encrypt_batch`` computes from the same (m, r) with one full-width modexp
(``encrypt_batch(.., randomness=..)``).  With randomness of its own the key holder skips the step modulo p: the N-th
residues modulo N^2 are C_{p-1} x C_{q-1} under the CRT and y -> y^p mod p^2 maps Z*_p onto C_{p-1} bijectively, so
rho_p = (D mod p^2)^p, rho_q = (D mod q^2)^q of ONE draw D of bits(N) + 64 bits per ciphertext (``rng``: a
``device_rng.DeviceRng``; D mod p and D mod q are jointly uniform up to 2^-64) is a uniform N-th residue — the reference's
distribution, no further assumption, no table.  The r of such a ciphertext, should anybody ask for it, is
rho^(N^-1 mod lambda) mod N with lambda = (p-1)(q-1).  DESIGN.md §4.22 has the measurements and says which route to take
where.  A randomness that shares a factor with N (r = 0, a multiple of p or q) gives rho_p = 0 or rho_q = 0: the row has
a status (bit 0: p, bit 1: q) and is zero, and the int-level functions raise ValueError as the reference's scheme rejects
such an r.

Side channels of the encryption.  The exponents p, q, q mod (p-1) and p mod (q-1) are secrets in the same class as the
decryption's — whoever learns e_p = q mod (p-1) = N mod (p-1) factors N through gcd(a^(N - e_p) - 1, N).  By default all
four modexps follow sliding-window schedules that are functions of their exponents' bits: the two modulo the squares the
pair kernel's tape, the two modulo the primes the generic kernel's shared-exponent schedule (``powmod_shared_t``).
``Engine.set_fixed_window(True)`` reaches all four: new plans of the pair kernel get the fixed-window tape, and the two
modexps modulo the primes are launched through ``powmod_multi_t`` with one group, the generic kernel's fixed-window
ladder.  The number and order of squarings and multiplications then depends on the bit lengths of the exponents only;
the table row a window reads is still chosen by its digit, and the bit length of q mod (p-1) itself (how many leading
zero bits it has) still shows in the length of its ladder.  Measured cost: 7-8 % of a caller's-r encryption at key_length
2048, 3-4 % at 4096.  The fresh mode has no modexp modulo the primes.

This path is for a plain key.  Neither direction ever applies to the distributed key of this package
(``GpuPaillierSharedKey``), whose primes nobody knows: there the threshold route — partial decryptions and their
recombination — is the only one.
"""

from __future__ import annotations

import math
from typing import Any, Iterable, List, Sequence, Tuple


def crt_constants(p: int, q: int) -> Tuple[int, int, int]:
    """(h_p, h_q, p^-1 mod q) of the key with the primes p and q; ValueError for an even or too small prime, p == q, or
    gcd(pq, (p-1)(q-1)) != 1 (then N + 1 does not generate what decryption needs and h_p or h_q does not exist)."""
    if p < 3 or q < 3 or p % 2 == 0 or q % 2 == 0:
        raise ValueError("p and q must be odd primes")
    if p == q:
        raise ValueError("p and q must differ")
    n = p * q
    if math.gcd(n, (p - 1) * (q - 1)) != 1:
        raise ValueError("gcd(pq, (p-1)(q-1)) must be 1")
    try:
        h_p = pow((pow(n + 1, p - 1, p * p) - 1) // p, -1, p)
        h_q = pow((pow(n + 1, q - 1, q * q) - 1) // q, -1, q)
    except ValueError:
        raise ValueError("p and q are no Paillier key: L((N+1)^(p-1)) is not invertible") from None
    return h_p, h_q, pow(p, -1, q)


_BAD_RANDOMNESS = "Randomness that shares a factor with N (0, or a multiple of p or q): no valid Paillier randomness"

_NOT_VALID = ("Not a valid ciphertext under this key: c^(p-1) is not 1 modulo p or c^(q-1) not 1 modulo q "
              "(the ciphertext shares a factor with N)")


class PaillierPrivateKey:
    """The private key (p, q) of the public key N = p q with generator N + 1, decrypting and encrypting batches on the GPU.

    The constructor refuses an even "prime", p == q and gcd(pq, (p-1)(q-1)) != 1, and tests nothing else — two odd
    composites that pass these checks give a key that decrypts wrongly.  ``check_primes()`` vets a key received from
    elsewhere; ``generate`` / ``generate_batch`` make keys from primes searched on the device.  ``engine`` is injected
    so that the host logic is testable without a GPU; the default is the process-wide HIP engine."""

    def __init__(self, p: int, q: int, engine: Any = None) -> None:
        p, q = int(p), int(q)
        self.h_p, self.h_q, self.p_inv = crt_constants(p, q)
        self.p, self.q = p, q
        self.n = p * q
        self.n_square = self.n * self.n
        self._engine = engine
        self._own_rng: Any = None                 # the device generator of fresh encryptions, made on first use

    # ------------------------------------------------------------------ key generation and vetting (primes.py)
    @classmethod
    def generate(cls, key_length: int, rng: Any = None, rounds: int = 64, engine: Any = None, safe: bool = False) -> "PaillierPrivateKey":
        """A fresh key whose N has exactly `key_length` bits: two distinct random probable primes of key_length / 2 bits
        each, found on the device (``primes.random_primes``: `rounds` Miller-Rabin rounds to random bases behind a sieve
        and the base 2).  ``rng``: a ``device_rng.DeviceRng`` (default: a fresh one, keyed from the operating
        system).  ``safe=True``: both primes are safe primes, p = 2 p' + 1 with p' prime (``primes.random_safe_primes``)
        — what threshold Paillier with a dealer and the auxiliary moduli of range proofs ask for; such primes are rare
        (one candidate in about 190 000 at key_length 2048), so the search takes correspondingly longer.  For two
        distinct safe primes of equal length gcd(N, phi(N)) = 1 holds by itself.  ValueError for an odd key_length or
        one below 64."""
        return cls.generate_batch(1, key_length, rng=rng, rounds=rounds, engine=engine, safe=safe)[0]

    @classmethod
    def generate_batch(cls, count: int, key_length: int, rng: Any = None, rounds: int = 64, engine: Any = None,
                       safe: bool = False) -> List["PaillierPrivateKey"]:
        """`count` fresh keys — one per client or per session — from ONE search for 2 * count primes: key i takes primes
        2 i and 2 i + 1 of the search's draw order.  A prime that came up twice (probability about 2^-(key_length / 2))
        is searched again.  Everything else as ``generate``."""
        count, key_length = int(count), int(key_length)
        if count < 0:
            raise ValueError("count must not be negative")
        if key_length < 64 or key_length % 2:
            raise ValueError("key_length must be even and at least 64")
        if int(rounds) < 1:
            raise ValueError("rounds must be at least 1")
        if count == 0:
            return []
        from . import primes
        from .device_rng import DeviceRng

        rng = DeviceRng() if rng is None else rng
        search = primes.random_safe_primes if safe else primes.random_primes
        found: List[int] = []
        while len(found) < 2 * count:
            for prime in search(2 * count - len(found), key_length // 2, rng=rng, rounds=rounds, engine=engine):
                if prime not in found:
                    found.append(prime)
        return [cls(found[2 * i], found[2 * i + 1], engine=engine) for i in range(count)]

    def check_primes(self, rounds: int = 64, rng: Any = None, engine: Any = None, safe: bool = False) -> bool:
        """True iff p and q both pass ``primes.is_probable_prime_batch`` with `rounds` random bases: wrong for a key with
        a composite "prime" with probability at most 4^-rounds, whoever chose it.  What to run on a key received from
        elsewhere before trusting its decryptions.  ``safe=True``: true iff p and q are both SAFE primes
        (``primes.is_safe_prime_batch``, the same error bound)."""
        from . import primes

        if safe:
            return all(primes.is_safe_prime_batch([self.p, self.q], rounds=rounds, rng=rng, engine=self._eng(engine)))
        return all(primes.is_probable_prime_batch([self.p, self.q], rounds=rounds, rng=rng, engine=self._eng(engine)))

    def _eng(self, engine: Any = None) -> Any:
        if engine is not None:
            return engine
        if self._engine is None:
            from .engine import default_engine

            self._engine = default_engine()
        return self._engine

    def decrypt_t(self, cts_t, engine: Any = None):
        """Device rows [batch, limbs(N^2)] of ciphertexts -> (plaintext rows [batch, limbs(N)], status uint8 [batch]) on
        the device, nothing fetched: ``Engine.private_decrypt_t``.  The caller reads the status (module docstring)."""
        return self._eng(engine).private_decrypt_t(cts_t, self.p, self.q)

    def decrypt_batch(self, cts: Sequence[int], signed: bool = False, engine: Any = None, return_ok: bool = False):
        """[decrypt(c) for c in cts] as one GPU batch.  ``signed=True`` maps m > N/2 to m - N.  A ciphertext with a
        non-zero status raises ValueError — like ``GpuPaillierSharedKey.decrypt_batch`` for a combination that is not 1
        modulo N — unless ``return_ok=True``: then the result is ``(messages, ok)`` and the message is 0 where ok is
        False."""
        vals = cts if isinstance(cts, list) else list(cts)
        if not vals:
            return ([], []) if return_ok else []
        msgs, ok = self._eng(engine).private_decrypt_batch(vals, self.p, self.q)
        if not return_ok and not all(ok):
            raise ValueError(_NOT_VALID)
        if signed:
            half, n = self.n // 2, self.n
            msgs = [m - n if m > half and good else m for m, good in zip(msgs, ok)]
        return (msgs, ok) if return_ok else msgs

    def decrypt(self, ciphertext: int, signed: bool = False) -> int:
        return self.decrypt_batch([ciphertext], signed=signed)[0]

    def decrypt_sequence(self, objs: Iterable[Any], signed: bool = False, engine: Any = None, return_ok: bool = False):
        """decrypt_batch over ciphertext OBJECTS: anything with ``get_value()`` (the reference's PaillierCiphertext,
        ``PlainCiphertext``), read the way ``homomorphic`` reads its operands; plain ints pass through."""
        vals: List[int] = [int(o.get_value()) if hasattr(o, "get_value") else int(o) for o in objs]
        return self.decrypt_batch(vals, signed=signed, engine=engine, return_ok=return_ok)

    # ------------------------------------------------------------------ encryption (module docstring)
    def _rng(self, randomness: Any, rng: Any) -> Any:
        """The source of fresh randomness when the caller names none: a device generator the key keeps."""
        if randomness is not None or rng is not None:
            return rng
        if self._own_rng is None:
            from .device_rng import DeviceRng

            self._own_rng = DeviceRng()
        return self._own_rng

    def noise_t(self, count: int, randomness_t=None, rng: Any = None, engine: Any = None, **options: Any):
        """``count`` rows of noise rho = r^N mod N^2 and their status on the device (``Engine.private_noise_t``): a pool to
        multiply into ciphertexts later.  Fresh draws from ``rng`` (default: the key's own generator) unless
        ``randomness_t`` holds the r or ``draws_t`` the draws.  ``options``: ``draws_t``, ``side_by_side``, ``packed``, as
        the engine takes them."""
        return self._eng(engine).private_noise_t(count, self.p, self.q, **self._sources(randomness_t, rng, options))

    def encrypt_t(self, messages_t, randomness_t=None, rng: Any = None, engine: Any = None, **options: Any):
        """Device rows [batch, >= limbs(N)] of messages below N -> (ciphertext rows [batch, limbs(N^2)], status uint8
        [batch]) on the device, nothing fetched: ``Engine.private_encrypt_t``.  The caller reads the status.
        ``options``: ``draws_t``, ``side_by_side``, ``packed``, ``return_randomness``, as the engine takes them."""
        return self._eng(engine).private_encrypt_t(messages_t, self.p, self.q, **self._sources(randomness_t, rng, options))

    def randomize_t(self, cts_t, randomness_t=None, rng: Any = None, engine: Any = None, **options: Any):
        """Device rows of ciphertexts -> (c r^N mod N^2, status) on the device: ``Engine.private_randomize_t``;
        ``options`` as ``encrypt_t``."""
        return self._eng(engine).private_randomize_t(cts_t, self.p, self.q, **self._sources(randomness_t, rng, options))

    def _sources(self, randomness_t: Any, rng: Any, options: dict) -> dict:
        """The keywords of the engine's tensor-level functions: the key's own generator where the caller names no source
        of randomness (``randomness_t``, ``rng`` or ``draws_t``)."""
        if randomness_t is None and rng is None and options.get("draws_t") is None:
            rng = self._rng(None, None)
        return dict(options, randomness_t=randomness_t, rng=rng)

    def _checked(self, result, return_ok: bool):
        values, ok = result
        if return_ok:
            return values, ok
        if not all(ok):
            raise ValueError(_BAD_RANDOMNESS)
        return values

    def encrypt_batch(self, messages: Sequence[int], randomness: Any = None, rng: Any = None, return_ok: bool = False, engine: Any = None):
        """[(1 + m N) r^N mod N^2 for m, r] as one GPU batch; messages are taken modulo N, so negative ones are allowed.
        ``randomness``: one r per message — the ciphertexts of ``Engine.encrypt_batch`` bit for bit; else fresh draws
        from ``rng`` (default: the key's own generator).  A randomness that shares a factor with N raises ValueError
        unless ``return_ok=True``: then the result is ``(ciphertexts, ok)`` and the ciphertext is 0 where ok is False."""
        vals = messages if isinstance(messages, list) else list(messages)
        if randomness is not None:
            randomness = randomness if isinstance(randomness, list) else list(randomness)
            if len(randomness) != len(vals):
                raise ValueError("one randomness per message expected")
        if not vals:
            return ([], []) if return_ok else []
        return self._checked(self._eng(engine).private_encrypt_batch(vals, self.p, self.q, randomness=randomness,
                                                                     rng=self._rng(randomness, rng)), return_ok)

    def encrypt(self, message: int, randomness: Any = None, rng: Any = None) -> int:
        return self.encrypt_batch([message], None if randomness is None else [randomness], rng)[0]

    def randomize_batch(self, cts: Sequence[int], randomness: Any = None, rng: Any = None, return_ok: bool = False, engine: Any = None):
        """[c r^N mod N^2 for c, r]: re-randomisation, everything as ``encrypt_batch``."""
        vals = cts if isinstance(cts, list) else list(cts)
        if randomness is not None:
            randomness = randomness if isinstance(randomness, list) else list(randomness)
            if len(randomness) != len(vals):
                raise ValueError("one randomness per ciphertext expected")
        if not vals:
            return ([], []) if return_ok else []
        return self._checked(self._eng(engine).private_randomize_batch(vals, self.p, self.q, randomness=randomness,
                                                                       rng=self._rng(randomness, rng)), return_ok)

    def encrypt_slots_t(self, values: Any, slot_bits: int, signed: bool = True, rng: Any = None, engine: Any = None, **options: Any):
        """Slot-packed encryption that leaves its result on the device: ``Engine.slots_encode_t`` followed by
        ``encrypt_t`` — ceil(count / k) ciphertext rows of the packed plaintexts of ``values`` (slots.py's layout) and
        their status; the plaintext rows never leave the device.  What ``slots.encrypt_t`` is for a ``FastRandomizer``,
        with the reference's randomiser."""
        eng = self._eng(engine)
        if not hasattr(values, "is_cuda") and not hasattr(values, "dtype"):      # Python ints: slots_encode_t takes arrays
            import numpy as np

            vals = [int(v) for v in values]
            for idx, v in enumerate(vals):
                if not -(1 << 63) <= v < 1 << 63:
                    raise ValueError(f"value {idx} ({v}) lies outside int64")
            values = np.array(vals, dtype=np.int64)
        rows_t = eng.slots_encode_t(values, self.n, int(slot_bits), bool(signed))
        return self.encrypt_t(rows_t, rng=rng, engine=eng, **options)

    def encrypt_slots(self, values: Any, slot_bits: int, signed: bool = True, rng: Any = None, engine: Any = None) -> List[int]:
        """``encrypt_slots_t`` fetched as ints; ValueError for a draw that shares a factor with N."""
        eng = self._eng(engine)
        rows_t, status_t = self.encrypt_slots_t(values, slot_bits, signed, rng=rng, engine=eng)
        if bool(status_t.any()):
            raise ValueError(_BAD_RANDOMNESS)
        from . import limbs

        return limbs.unpack(eng.to_host(rows_t))
