"""Host-side mirror of the Shamir-field steps of a key-generation round, batched over candidates.

Reference: the candidate moduli of a round are formed from Shamir shares modulo a prime P
(distributed_keygen.py:647-651) by

    candidate_n = prime_candidate_p * prime_candidate_q         DK:1274   share-wise product modulo P
    candidate_n += zero                                         DK:1277   share-wise sum modulo P
    await exchange_reconstruct(candidate_n, ...)                DK:1281   every party learns all shares
    candidate_n_plaintext = candidate_n.reconstruct()           DK:1284   Lagrange interpolation at 0

through ``Batched[ShamirVariable]`` (utils.py:205-270, 404-471), whose arithmetic lives in the
un-vendored tno.mpc.encryption_schemes.shamir (``ShamirShares.__mul__/__add__/reconstruct_secret``:
the textbook prime-field operations).  Here the same values are computed for the whole batch at
once: ``mul_add_shares_batch`` = this party's share of every candidate, ``reconstruct_batch`` = the
candidate moduli; the tensor-level forms (``Engine.shamir_fma_t`` / ``shamir_lincomb_t``) keep them
on the device for the sieve that follows (DK:1288-1292).

The step in front of that — `_generate_pq`, DK:718-853: this party's additive shares p_i, q_i of the round's prime
candidates (DK:874-875) and the Shamir sharings of p_i, q_i (degree t) and of 0 (degree 2t) that it sends out — is
``generate_pq_t`` / ``generate_pq_batch``: five rows calls on a ``device_rng.DeviceRng`` and five kernels on their rows for the whole
round instead of a Python loop per candidate, coefficient and party.  ``sum_shares_*`` are the sums p = sum_j p_j of the
received shares (DK:840-847).  What a caller must know before using it:

  * A coefficient of a sharing polynomial is D mod P for a draw D of bits(P) + 64 bits: uniform on [0, P) up to a bias
    below 2^-64 (the draw ``Engine.encrypt_fresh_batch`` makes for its randomness, for the same reason).
  * Candidates and coefficients are a DETERMINISTIC EXPANSION of the ``DeviceRng`` key: who knows the key knows every
    share of every round.  Read the module docstring of ``device_rng`` — what the key is, where it lives, what a fork
    does to it — before use.
  * Opt-in.  Nothing draws on the device unless a caller passes a ``DeviceRng`` here or as ``share_rng=`` to
    ``patch.install``; the reference's own ``secrets``-based sampling stays the default.

Draw order (the contract tools/share_model.py and the tests rebuild): with c = ``rng.next_call`` on entry,
    call c      p candidates     rows_t(batch, L - 3)
    call c + 1  q candidates     rows_t(batch, L - 3)
    call c + 2  p coefficients   rows_t(t * batch, bits(P) + 64, cw)      row (k - 1) * batch + e: coefficient k of candidate e
    call c + 3  q coefficients   rows_t(t * batch, bits(P) + 64, cw)
    call c + 4  zero coefficients rows_t(2t * batch, bits(P) + 64, cw)
"""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

MAX_SHARE_DEGREE = 24          # include/mxpaillier.h: MX_SHARE_MAX_DEGREE (an element's coefficients are kept in LDS)


def _engine(engine: Any) -> Any:
    if engine is not None:
        return engine
    from .engine import default_engine

    return default_engine()


def lagrange_coefficients_at_zero(points: Sequence[int], prime: int, engine: Any = None) -> List[int]:
    """lambda_i = prod_{j != i} x_j / (x_j - x_i) mod prime for the evaluation points x (party indices):
    products of a handful of word-sized values on the host, as in the reference; the modular inverses
    of the denominators go through the engine's device inverse when an engine is given (so that the
    batched path has no host big-integer inversion at all), else through ``pow(den, -1, prime)``."""
    if len(set(points)) != len(points):
        raise ValueError("evaluation points must be distinct")
    nums, dens = [], []
    for i in points:
        num = den = 1
        for j in points:
            if j != i:
                num = num * j % prime
                den = den * (j - i) % prime
        nums.append(num)
        dens.append(den)
    invs = engine.modinv_batch(dens, prime) if engine is not None else [pow(d, -1, prime) for d in dens]
    return [n * v % prime for n, v in zip(nums, invs)]


def mul_add_shares_batch(p_shares: Sequence[int], q_shares: Sequence[int], zero_shares: Sequence[int], prime: int,
                         engine: Any = None) -> List[int]:
    """[(p * q + z) % prime ...]: this party's share of every candidate modulus (DK:1274-1277)."""
    return _engine(engine).shamir_fma_batch(list(p_shares), list(q_shares), list(zero_shares), prime)


def _points(shares_by_party: Dict[int, Sequence[int]], degree: int, points: Optional[Sequence[int]]) -> List[int]:
    """The degree+1 evaluation points the interpolation runs through.  The un-vendored
    ``ShamirShares.reconstruct_secret`` takes the first degree+1 entries of its shares dictionary in
    INSERTION order; a caller that has that dictionary passes its key order as `points` (patch.py does).
    Without it the parties are taken in index order — the same value whenever the shares are consistent
    (any degree+1 points of a degree-`degree` polynomial interpolate to the same secret)."""
    if points is None:
        pts = sorted(shares_by_party)[: degree + 1]
    else:
        pts = [int(i) for i in points][: degree + 1]
        if any(i not in shares_by_party for i in pts):
            raise KeyError(next(i for i in pts if i not in shares_by_party))
    if len(pts) < degree + 1:
        raise ValueError("not enough shares to reconstruct")
    return pts


def reconstruct_batch(shares_by_party: Dict[int, Sequence[int]], prime: int, degree: int, engine: Any = None,
                      points: Optional[Sequence[int]] = None) -> List[int]:
    """Candidate moduli of a round from every party's shares (DK:1284): per candidate the value at 0 of
    the degree-`degree` polynomial through the shares of degree+1 parties (`points`, see _points).
    Raises ValueError with fewer shares than that."""
    points = _points(shares_by_party, degree, points)
    count = len(shares_by_party[points[0]])
    if any(len(shares_by_party[i]) != count for i in points):
        raise ValueError("every party needs one share per candidate")
    if count == 0:
        return []
    eng = _engine(engine)
    coeffs = lagrange_coefficients_at_zero(points, prime, eng)
    return eng.shamir_lincomb_batch([shares_by_party[i] for i in points], coeffs, prime)


def reconstruct_and_sieve_batch(shares_by_party: Dict[int, Sequence[int]], prime: int, degree: int,
                                prime_list: Sequence[int], engine: Any = None, points: Optional[Sequence[int]] = None):
    """DK:1284 and the filter DK:1288-1292 for a whole round without the moduli leaving the device in
    between: returns (has_small_divisor per candidate, {candidate index: modulus} of the survivors)."""
    points = _points(shares_by_party, degree, points)
    count = len(shares_by_party[points[0]])
    if any(len(shares_by_party[i]) != count for i in points):
        raise ValueError("every party needs one share per candidate")
    if count == 0:
        return [], {}
    eng = _engine(engine)
    coeffs = lagrange_coefficients_at_zero(points, prime, eng)
    return eng.shamir_reconstruct_sieve_batch([shares_by_party[i] for i in points], coeffs, prime, list(prime_list))


# ------------------------------------------------------------------ candidates and their sharings (DK:718-853)
def coefficient_bits(prime: int) -> int:
    """Bits of the draw behind one coefficient of a sharing polynomial: 64 more than the prime has."""
    return int(prime).bit_length() + 64


def check_candidate_args(count: int, prime_length: int, row_words: Optional[int] = None) -> Tuple[int, int]:
    """(words of a random row, words of a candidate row) for candidates of `prime_length` bits, or ValueError."""
    if prime_length < 8:
        raise ValueError("prime_length must be at least 8")
    if count < 0:
        raise ValueError("count must not be negative")
    words = (prime_length + 31) // 32
    row_words = words if row_words is None else int(row_words)
    if row_words < words:
        raise ValueError("rows narrower than prime_length bits")
    return (prime_length - 3 + 31) // 32, row_words


def check_share_args(prime: int, degree: int, points: Sequence[int]) -> List[int]:
    """The evaluation points as a list of ints, or the ValueError of a sharing the engine refuses."""
    if prime < 3 or prime % 2 == 0:
        raise ValueError("the Shamir modulus must be odd and >= 3")
    if degree < 1:
        raise ValueError("the polynomial degree must be at least 1")
    if degree > MAX_SHARE_DEGREE:
        raise ValueError(f"the polynomial degree must not exceed {MAX_SHARE_DEGREE}")
    pts = []
    for x in points:
        if isinstance(x, bool) or not hasattr(x, "__index__"):
            raise ValueError("evaluation points must be integers")
        pts.append(int(x))
    if any(not 1 <= x < 1 << 16 for x in pts) or len(set(pts)) != len(pts):
        raise ValueError("evaluation points must be distinct integers in [1, 2^16)")
    if len(pts) < degree + 1:
        raise ValueError("a sharing of this degree needs at least degree + 1 points")
    return pts


def _check_round(index: int, prime_length: int, prime: int, n_parties: int, t: int, batch_size: int) -> List[int]:
    if not 1 <= index <= n_parties:
        raise ValueError("index must lie in 1 .. n_parties")
    if batch_size < 0:
        raise ValueError("batch_size must not be negative")
    check_candidate_args(batch_size, prime_length)
    if prime_length >= prime.bit_length():
        raise ValueError("candidates of prime_length bits must lie below the Shamir modulus")
    points = list(range(1, n_parties + 1))
    check_share_args(prime, t, points)
    check_share_args(prime, 2 * t, points)
    return points


def generate_pq_t(index: int, prime_length: int, prime: int, n_parties: int, t: int, batch_size: int, rng: Any,
                  engine: Any = None):
    """`_generate_pq` up to the exchange (DK:784-831) on the device: ``(p_t, q_t, shares_t)`` with this party's additive
    shares of the round's candidates as rows ``[batch_size, limbs]`` (limbs = the width of `prime`) and
    ``shares_t = {"p": ..., "q": ..., "zero": ...}``, each ``[n_parties, batch_size, limbs]``: row block j - 1 is what
    party j receives.  Degrees t, t and 2t; points 1 .. n_parties; five calls on `rng` in the order of the module
    docstring.  Every refusal (engine docstrings) comes before the first of them."""
    index, prime_length, prime, n_parties, t, batch_size = (int(v) for v in (index, prime_length, prime, n_parties, t, batch_size))
    points = _check_round(index, prime_length, prime, n_parties, t, batch_size)
    if rng is None:
        raise ValueError("a DeviceRng is needed")
    eng = _engine(engine)
    from . import limbs as _limbs

    limbs = _limbs.limbs_for(prime)
    p_t = eng.prime_candidates_t(batch_size, prime_length, index == 1, rng=rng, row_words=limbs)
    q_t = eng.prime_candidates_t(batch_size, prime_length, index == 1, rng=rng, row_words=limbs)
    shares_t = {
        "p": eng.shamir_share_t(p_t, prime, t, points, rng=rng),
        "q": eng.shamir_share_t(q_t, prime, t, points, rng=rng),
        "zero": eng.shamir_share_t(None, prime, 2 * t, points, batch=batch_size, rng=rng),
    }
    return p_t, q_t, shares_t


def generate_pq_batch(index: int, prime_length: int, prime: int, n_parties: int, t: int, batch_size: int, rng: Any,
                      engine: Any = None):
    """generate_pq_t as Python ints: ``(p_additive, q_additive, shares)`` with
    ``shares = {"p": {j: [...]}, "q": {...}, "zero": {...}}`` for j = 1 .. n_parties — what `_generate_pq` holds after
    its three ``.share(index)`` calls (DK:829-831)."""
    eng = _engine(engine)
    p_t, q_t, shares_t = generate_pq_t(index, prime_length, prime, n_parties, t, batch_size, rng, eng)
    batch = int(batch_size)
    shares: Dict[str, Dict[int, List[int]]] = {}
    for name, rows_t in shares_t.items():
        vals = eng._download_ints(rows_t.reshape(int(n_parties) * batch, -1)) if batch else []
        shares[name] = {j: vals[(j - 1) * batch : j * batch] for j in range(1, int(n_parties) + 1)}
    return (eng._download_ints(p_t) if batch else []), (eng._download_ints(q_t) if batch else []), shares


def sum_shares_t(x_t, prime: int, engine: Any = None):
    """p = sum_j p_j per candidate (DK:840-847) for shares ``[terms, batch, limbs]`` on the device: the linear
    combination with coefficients 1."""
    return _engine(engine).shamir_lincomb_t(x_t, [1] * int(x_t.shape[0]), prime)


def sum_shares_batch(columns: Sequence[Sequence[int]], prime: int, engine: Any = None) -> List[int]:
    """The same over Python ints: one column of shares per party, one sum per candidate."""
    return _engine(engine).shamir_lincomb_batch([list(c) for c in columns], [1] * len(columns), prime)
