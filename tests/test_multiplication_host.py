"""Host logic of the multiplication proofs (multiplication.py) and of the product of two ciphertexts under a dealt
threshold key (secure_product.py) over the Python-int double of the engine (mul_engine.py), bit-exact against the model
(tools/mul_model.py).  No GPU."""

from __future__ import annotations

import random

import numpy as np
import pytest

import mul_cases as mc
from mul_cases import mulm
from mul_engine import MulEngine, equations_hold, tamperings, zero_forgeries

from protocols.distributed_keygen_amd import limbs, multiplication, secure_product, threshold
from protocols.distributed_keygen_amd.device_rng import DeviceRng
from protocols.distributed_keygen_amd.multiplication import MultiplicationProofs

N128, N1K, N2K = mc.modulus(128), mc.modulus(1024), mc.modulus(2048)


def proven(n, count, call=40, label=mc.LABEL):
    eng = MulEngine()
    a, ra, gamma, b, ca, cb = mc.statements(n, count)
    d, proofs = multiplication.prove_batch(n, a, ra, gamma, cb, label, rng=DeviceRng(key=mc.KEY, first_call=call), c_a=ca, engine=eng)
    return eng, (a, ra, gamma, b, ca, cb), d, proofs


def row_of(cols, r):
    return [col[r] for col in cols]


# ---- the response modulo M: the kernel's steps against divmod --------------------------------------------------------------
def test_the_estimate_never_falls_short_by_more_than_the_kernel_corrects_exhaustively_at_4_bit_words():
    """Every M of two 4-bit words with a non-zero top word, odd and even, and EVERY window below 16 M: the estimate is
    never above the digit and at most MAX_ESTIMATE_ERROR below it."""
    worst = 0
    for mod in range(16, 256):
        recip, shift = mulm.response_mod_constants(mod, 2, 4)
        for window in range(16 * mod):
            short = window // mod - mulm.response_mod_estimate(window >> 8, (window >> 4) & 15, window & 15, recip, shift, 4)
            assert 0 <= short <= mulm.MAX_ESTIMATE_ERROR, (mod, window)
            worst = max(worst, short)
    assert worst >= 1                      # (the corrections are not idle)


def test_the_step_wise_division_equals_divmod_exhaustively_at_4_bit_words():
    """wn = 2, ew = 1: every M and EVERY s a row can form (s <= 16 * 255); and pass 1 for every (rho, e, x), which does not
    depend on M — the two halves of response_mod_steps, each over its whole domain."""
    for mod in range(16, 256):
        for s in range(16 * 255 + 1):
            q, r = divmod(s, mod)
            assert mulm.response_mod_divide([s & 15, (s >> 4) & 15, s >> 8], mod, 2, 1, 4) == (r, q & 15, int(q > 15)), (mod, s)
    for rho in range(256):
        for x in range(256):
            for e in range(16):
                words = mulm.response_mod_form(rho, e, x, 2, 1, 4)
                assert words[0] | words[1] << 4 | words[2] << 8 == rho + e * x
    rnd = random.Random(4)
    for _ in range(2000):                  # and the two together
        mod, rho, e, x = rnd.randrange(16, 256), rnd.randrange(256), rnd.randrange(16), rnd.randrange(256)
        q, r = divmod(rho + e * x, mod)
        assert mulm.response_mod_steps(rho, e, x, mod, 2, 1, 4) == (r, q & 15, int(q > 15)) and mulm.response_mod(rho, e, x, mod) == (r, q)


@pytest.mark.parametrize("wn", [1, 2, 4, 9, 32])
def test_the_step_wise_form_on_the_directed_rows_at_32_bit_words(wn):
    errors = []
    for name, mod in mc.moduli(wn) if wn > 1 else [("one word", 0xFFFFFFFB), ("one word, top bit clear", 0x10001)]:
        rows = mc.response_rows(mod, wn, 64)
        want = mc.expected(rows, mod)
        got = [mulm.response_mod_steps(rho, e, x, mod, wn, 4, 32, errors) for rho, e, x in rows]
        assert [g[0] for g in got] == want[0] and [g[1] for g in got] == want[1] and [g[2] for g in got] == want[2], name
        if wn >= 2 and mod < (1 << (32 * wn)) - 1:
            assert want[2][-4] == 1 and sum(want[2][:-4]) == 0, name          # rho, x below M never raise the status
        if wn >= 5:          # every directed multiple is there: s = k M - 1, k M, k M + 1
            assert {(k, dl) for k in mc.DIRECTED_K for dl in (-1, 0, 1)} <= {(k, rho + e * x - k * mod) for rho, e, x in rows for k in mc.DIRECTED_K}, name
    assert 0 <= min(errors) and max(errors) <= mulm.MAX_ESTIMATE_ERROR


def test_the_quotient_of_in_range_rows_fits_the_challenge_width():
    for mod in (N128, N1K, (1 << 96) + 1, (1 << 128) - 1):
        w, t = mulm.response_mod(mod - 1, mc.E_MAX, mod - 1, mod)
        assert t <= mc.E_MAX and w + t * mod == (mod - 1) * (mc.E_MAX + 1)


def test_the_engines_double_refuses_what_the_engine_refuses():
    eng = MulEngine()
    rows = eng.to_device(np.zeros((2, 4), dtype=np.uint32))
    for bad in (lambda: eng.response_mod_rows_t(rows, rows, rows[:, :3], N128), lambda: eng.response_mod_rows_t(rows, rows[:1], rows, N128),
                lambda: eng.response_mod_rows_t(rows, rows, rows, N128 >> 40), lambda: eng.response_mod_rows_t(rows, rows, rows, N128 << 8),
                lambda: eng.response_mod_rows_t(rows, rows, rows, N128, out_t=rows), lambda: eng.response_mod_constants(1 << 128, 4),
                lambda: eng.response_mod_constants(0, 1)):
        with pytest.raises(ValueError):
            bad()
    assert eng.response_mod_constants(1, 1) == ((1 << 96) // ((1 << 63) + 1), 31) and eng.response_mod_constants((1 << 64) - 1, 2) == (1 << 32, 0)


# ---- the proofs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_length", [128, 1024, 2048])
def test_the_model_is_complete_at_the_extremes(key_length):
    n = mc.modulus(key_length)
    n2 = n * n
    a, ra, gamma, b, ca, cb = mc.statements(n, 4)
    xs, us, vs = mulm.device_draws(mc.KEY, 9, 4, n)
    xs[1] += (n - 1) - xs[1] % n                   # x = N - 1 beside a = N - 1
    assert xs[1] % n == n - 1 and a[1] == n - 1 and a[0] == 0 and xs[1] >> (n.bit_length() + 64) == 0
    for r in range(4):
        d = mulm.product(n, cb[r], a[r], gamma[r])
        proof = mulm.prove(n, mc.LABEL, ca[r], cb[r], a[r], ra[r], gamma[r], xs[r], us[r], vs[r])
        assert mulm.verify(n, mc.LABEL, ca[r], cb[r], d, proof) and equations_hold(n, mc.LABEL, ca[r], cb[r], d, proof) == (True, True)
        assert mc.decrypt(key_length, d) == a[r] * b[r] % n if key_length == 128 else True
        wrong = d * (1 + n) % n2                   # a d that holds a b + 1
        assert not mulm.verify(n, mc.LABEL, ca[r], cb[r], wrong, proof) and equations_hold(n, mc.LABEL, ca[r], cb[r], wrong, proof) != (True, True)
    # e = 2^128 - 1 with x = a = N - 1: the largest response, written out with the challenge forced
    x = a_ = n - 1
    w, t = mulm.response_mod(x, mc.E_MAX, a_, n)
    assert (w, t) == ((x + mc.E_MAX * a_) % n, (x + mc.E_MAX * a_) // n) and t < 1 << 128
    u, v, g, rr = us[0], vs[0], gamma[1], ra[1]
    z, y = u % n * pow(rr, mc.E_MAX, n) % n, v % n * pow(cb[1] % n, t, n) % n * pow(g, mc.E_MAX, n) % n
    aa, bb = (1 + x * n) * pow(u, n, n2) % n2, pow(cb[1], x, n2) * pow(v, n, n2) % n2
    d = mulm.product(n, cb[1], a_, g)
    assert (1 + w * n) * pow(z, n, n2) % n2 == aa * pow(ca[1], mc.E_MAX, n2) % n2
    assert pow(cb[1], w, n2) * pow(y, n, n2) % n2 == bb * pow(d, mc.E_MAX, n2) % n2


@pytest.mark.parametrize("key_length,count", [(1024, 5), (2048, 3)])
def test_proofs_equal_the_model_bit_for_bit_and_verify(key_length, count):
    n = mc.modulus(key_length)
    eng, (a, ra, gamma, b, ca, cb), d, proofs = proven(n, count)
    want_d, want = mc.model_proofs(n, mc.LABEL, a, ra, gamma, ca, cb, 40)
    assert d == want_d and proofs.to_ints() == want
    assert multiplication.context(n, mc.LABEL) == mulm.context(n, mc.LABEL)
    assert multiplication.shape(n) == mulm.shape(n) == eng.mul_shape(n)
    assert multiplication.verify_batch(n, ca, cb, d, proofs, mc.LABEL, engine=eng) == [True] * count
    again = MultiplicationProofs.from_ints(*proofs.to_ints(), n)
    assert again.unfit == [False] * count and all((x == eng.to_host(y)).all() for x, y in zip(again.rows(), proofs.rows()))
    assert multiplication.verify_batch(n, ca, cb, d, again, mc.LABEL, engine=eng) == [True] * count
    # the composition: c_b^a and c_b^x are ONE multi-exponentiation over the count inputs; u^N, v^N, gamma^N ONE launch on
    # 3 count rows; the prover's response modulo N twice (the reduction of c_b, then (w, t))
    ln = limbs.limbs_for(n)
    calls = eng.calls[: eng.calls.index(("mul_verify", count))]
    assert [c[1:] for c in calls if c[0] == "multiexp_rows"] == [(count, 2 * count, 1, 32 * ln)]
    assert [c for c in calls if c[0] == "powmod_nsquare"] == [("powmod_nsquare", 3 * count)]
    assert [c for c in calls if c[0] == "response_mod"] == [("response_mod", count, ln, ln), ("response_mod", count, ln, 4)]
    after = eng.calls[eng.calls.index(("mul_verify", count)) + 1 : eng.calls.index(("mul_verify", count), eng.calls.index(("mul_verify", count)) + 1)]
    assert [c for c in after if c[0] == "powmod_nsquare"] == [("powmod_nsquare", 2 * count)]
    assert [c[1:] for c in after if c[0] == "multiexp_rows"] == [(count, count, 1, 32 * ln), (4 * count, 2 * count, 2, 128)]


def test_the_double_takes_the_smallest_key_and_equals_the_model():
    """The engine entries take any N the wide draws fit under (the 260-bit refusal is the module's): the 128-bit golden
    key, with a = 0 and a = N - 1 and b = 0 and b = N - 1 among the rows."""
    eng = MulEngine()
    count = 9
    a, ra, gamma, b, ca, cb = mc.statements(N128, count)
    sh = eng.mul_shape(N128)

    def up(vals, words):
        return eng.to_device(limbs.pack(vals, words).reshape(count, words))

    ctx = mulm.context(N128, mc.LABEL)
    rows = eng.mul_prove_t(up(ca, sh["limbs2"]), up(cb, sh["limbs2"]), up(a, sh["limbs_n"]), up(ra, sh["limbs_n"]), up(gamma, sh["limbs_n"]),
                           N128, ctx, rng=DeviceRng(key=mc.KEY, first_call=7))
    want_d, want = mc.model_proofs(N128, mc.LABEL, a, ra, gamma, ca, cb, 7)
    assert limbs.unpack(eng.to_host(rows[0])) == want_d and MultiplicationProofs(*rows[1:]).to_ints() == want
    assert [mc.decrypt(128, d) for d in want_d] == [x * y % N128 for x, y in zip(a, b)]
    assert list(eng.mul_verify_t(up(ca, sh["limbs2"]), up(cb, sh["limbs2"]), *rows, N128, ctx)) == [True] * count


def test_every_tampering_is_false_for_its_row_only():
    n = N1K
    eng, (a, ra, gamma, b, ca, cb), d, proofs = proven(n, 3)
    cols = proofs.to_ints()
    for what, tca, tcb, td, *tcols in tamperings(n, cols, ca, cb, d):
        spoiled = MultiplicationProofs.from_ints(*tcols, n)
        assert multiplication.verify_batch(n, tca, tcb, td, spoiled, mc.LABEL, engine=eng) == [True, False, True], what
        if what != "no integer":
            assert not mulm.verify(n, mc.LABEL, tca[1], tcb[1], td[1], row_of(tcols, 1)), what
            assert mulm.verify(n, mc.LABEL, tca[0], tcb[0], td[0], row_of(tcols, 0)) and mulm.verify(n, mc.LABEL, tca[2], tcb[2], td[2], row_of(tcols, 2))
    # a short row: a column with one entry too few is the caller's mistake
    with pytest.raises(ValueError):
        MultiplicationProofs.from_ints(cols[0], cols[1], cols[2], cols[3], cols[4][:-1], n)
    # the label and N are bound by ctx (and by the equations): every row fails
    assert multiplication.verify_batch(n, ca, cb, d, proofs, b"another session", engine=eng) == [False] * 3
    other_n = n + 2
    moved = MultiplicationProofs.from_ints(*cols, other_n)
    assert multiplication.verify_batch(other_n, ca, cb, d, moved, mc.LABEL, engine=eng) == [False] * 3
    assert not any(mulm.verify(other_n, mc.LABEL, ca[r], cb[r], d[r], row_of(cols, r)) for r in range(3))


def test_the_zero_forgeries_are_refused():
    """A d that holds a b + 1 — alpha = a + b^-1 — with proofs that satisfy BOTH equations and need no witness for the
    half they zero: only the refusal of zero stops them."""
    n = N1K
    eng, (a, ra, gamma, b, ca, cb), d, proofs = proven(n, 3)
    cols = proofs.to_ints()
    alpha = (a[1] + pow(b[1], -1, n)) % n
    draws = [col[0] for col in mulm.device_draws(mc.KEY, 3, 1, n)]
    wrong_d, forged = zero_forgeries(n, mc.LABEL, ca[1], cb[1], a[1], ra[1], alpha, gamma[1], draws)
    assert wrong_d == d[1] * pow(cb[1], alpha - a[1], n * n) % (n * n) != d[1]
    small = N128                                   # (that such a d holds a b + 1, seen by decrypting at the small key)
    sa, sra, sg, sb, sca, scb = mc.statements(small, 1)
    assert mc.decrypt(128, mulm.product(small, scb[0], (sa[0] + pow(sb[0], -1, small)) % small, sg[0])) == (sa[0] * sb[0] + 1) % small
    assert [name for name, _ in forged] == ["A = z = 0", "B = y = 0", "A = z = 0 and B = y = 0"]
    for what, proof in forged:
        assert not mulm.verify(n, mc.LABEL, ca[1], cb[1], wrong_d, proof) and not mulm.in_range(n, ca[1], cb[1], wrong_d, proof), what
        got = MultiplicationProofs.from_ints(*([cols[j][0], proof[j], cols[j][2]] for j in range(5)), n)
        assert multiplication.verify_batch(n, ca, cb, [d[0], wrong_d, d[2]], got, mc.LABEL, engine=eng) == [True, False, True], what


def test_multiply_with_proof_round_trip():
    eng = MulEngine()
    n = N1K
    a, ra, gamma, b, ca, cb = mc.statements(n, 3)
    c_a, d, proofs = multiplication.multiply_with_proof(n, a, cb, mc.LABEL, rng=DeviceRng(key=mc.KEY, first_call=1), engine=eng)
    assert multiplication.verify_batch(n, c_a, cb, d, proofs, mc.LABEL, engine=eng) == [True] * 3
    cols = proofs.to_ints()
    assert all(mulm.verify(n, mc.LABEL, c_a[r], cb[r], d[r], row_of(cols, r)) for r in range(3))
    assert multiplication.verify_batch(n, c_a, cb, [d[0], d[1] * (1 + n) % (n * n), d[2]], proofs, mc.LABEL, engine=eng) == [True, False, True]
    assert multiplication.verify_batch(n, [c_a[0], c_a[1] * (1 + n) % (n * n), c_a[2]], cb, d, proofs, mc.LABEL, engine=eng) == [True, False, True]


def test_every_refusal_happens_without_an_engine_call():
    eng = MulEngine()
    n = N1K
    a, ra, gamma, b, ca, cb = mc.statements(n, 2)
    d0, empty = multiplication.prove_batch(n, [], [], [], [], mc.LABEL, engine=eng)
    assert d0 == [] and len(empty) == 0 and multiplication.verify_batch(n, [], [], [], empty, mc.LABEL, engine=eng) == []
    assert multiplication.multiply_with_proof(n, [], [], mc.LABEL, engine=eng)[:2] == ([], [])
    d, good = multiplication.prove_batch(n, a, ra, gamma, cb, mc.LABEL, rng=DeviceRng(key=mc.KEY), c_a=ca, engine=eng)
    pk, shares = dealt(128, 3, 1)
    eng.calls.clear()
    n259 = (1 << 258) | 1
    for bad in (lambda: multiplication.prove_batch(N128, a, ra, gamma, cb, mc.LABEL, engine=eng),                 # bits(N) < 260
                lambda: multiplication.prove_batch(n259, a, ra, gamma, cb, mc.LABEL, engine=eng),
                lambda: multiplication.prove_batch(n - 1, a, ra, gamma, cb, mc.LABEL, engine=eng),                # an even N
                lambda: multiplication.prove_batch(n, [0, n], ra, gamma, cb, mc.LABEL, engine=eng),              # a >= N
                lambda: multiplication.prove_batch(n, [0, -1], ra, gamma, cb, mc.LABEL, engine=eng),
                lambda: multiplication.prove_batch(n, a, ra[:1], gamma, cb, mc.LABEL, engine=eng),
                lambda: multiplication.prove_batch(n, a, ra, gamma, cb[:1], mc.LABEL, engine=eng),
                lambda: multiplication.prove_batch(n, a, ra, gamma, [cb[0], 0], mc.LABEL, engine=eng),           # c_b = 0
                lambda: multiplication.prove_batch(n, a, ra, gamma, [cb[0], n * n], mc.LABEL, engine=eng),
                lambda: multiplication.prove_batch(n, a, ra, gamma, cb, mc.LABEL, c_a=ca[:1], engine=eng),
                lambda: multiplication.prove_batch(n, a, ra, gamma, cb, "a str label", engine=eng),
                lambda: multiplication.multiply_with_proof(N128, a, cb, mc.LABEL, engine=eng),
                lambda: multiplication.multiply_with_proof(n, [n], cb[:1], mc.LABEL, engine=eng),
                lambda: multiplication.multiply_with_proof(n, a, cb[:1], mc.LABEL, engine=eng),
                lambda: multiplication.verify_batch(N128, ca, cb, d, good, mc.LABEL, engine=eng),
                lambda: multiplication.verify_batch(n, ca[:1], cb, d, good, mc.LABEL, engine=eng),
                lambda: multiplication.verify_batch(n, ca, cb, d[:1], good, mc.LABEL, engine=eng),
                lambda: multiplication.verify_batch(n, ca, cb, d, good.to_ints(), mc.LABEL, engine=eng),
                lambda: MultiplicationProofs.from_ints([1], [1], [1], [1], [], n),
                lambda: secure_product.mask_batch(pk, 1, [5], mc.LABEL, engine=eng),                               # the 128-bit key
                lambda: secure_product.mask_batch(pk, 4, [5], mc.LABEL, engine=eng),                               # no such party
                lambda: secure_product.mask_batch(pk, 1, [0], mc.LABEL, engine=eng),
                lambda: secure_product.mask_batch(pk, 1, [5], "a str label", engine=eng),
                lambda: secure_product.masked_batch(pk, [5], [5, 6], [], mc.LABEL, engine=eng),
                lambda: secure_product.masked_batch(pk, [5], [5], [], mc.LABEL, engine=eng),                       # nobody contributed
                lambda: secure_product.finish_batch(pk, [5], [pk.n], [secure_product.MaskContribution(1, [5], [5], empty)], engine=eng),
                lambda: secure_product.finish_batch(pk, [5], [1], [], engine=eng)):
        with pytest.raises(ValueError):
            bad()
    assert eng.calls == []
    assert multiplication.shape((1 << 259) | 1)["draw_bits"] == 260 + 64          # the shortest modulus the module takes


# ---- the product of two ciphertexts under a dealt key -----------------------------------------------------------------------
class _Key:
    def __init__(self, p, q):
        self.p, self.q = p, q


def dealt(key_length, parties, thr):
    p, q = mc.primes(key_length)
    return threshold.deal(_Key(p, q), parties, thr, rng=random.Random(11), check=False, engine=MulEngine())


@pytest.fixture
def small_keys_allowed(monkeypatch):
    """The 128-bit golden key carries no soundness (its prime factors are 64 bits long) and the module refuses it; the
    PROTOCOL is the same at any length, so these tests lower the module's bound for their duration."""
    monkeypatch.setattr(multiplication, "MIN_BITS", 128)


@pytest.mark.parametrize("parties,thr", [(3, 1), (5, 2)])
def test_the_product_of_two_ciphertexts_decrypts_to_the_product(small_keys_allowed, parties, thr):
    pk, shares = dealt(128, parties, thr)
    n = pk.n
    rnd = random.Random(parties)
    a = [rnd.randrange(n), rnd.randrange(n)] + [x for x in (0, 1, n - 1) for _ in range(3)]
    b = [rnd.randrange(n), rnd.randrange(n)] + [0, 1, n - 1] * 3
    ca = [mulm.encrypt(n, m, rnd.randrange(1, n)) for m in a]
    cb = [mulm.encrypt(n, m, rnd.randrange(1, n)) for m in b]
    rng = DeviceRng(key=mc.KEY, first_call=100)
    c_ab, cheaters = secure_product.multiply(pk, shares, ca, cb, mc.LABEL, rng=rng)
    assert cheaters == [] and [mc.decrypt(128, c) for c in c_ab] == [x * y % n for x, y in zip(a, b)]
    sq, cheaters = secure_product.square(pk, shares, ca[:3], mc.LABEL + b"/sq", rng=rng)
    assert cheaters == [] and [mc.decrypt(128, c) for c in sq] == [x * x % n for x in a[:3]]


def cheating_contribution(pk, index, cb, label, rng):
    """Party `index` with an E_i that holds (d_i + 1) b: honest D_i and proofs, E_i times c_b."""
    good = secure_product.mask_batch(pk, index, cb, label, rng=rng)
    return secure_product.MaskContribution(index, good.D, [e * c % pk.n_square for e, c in zip(good.E, cb)], good.proofs)


def test_a_cheating_party_is_named_and_left_out_and_too_few_is_an_error(small_keys_allowed):
    pk, shares = dealt(128, 3, 1)
    n = pk.n
    rnd = random.Random(8)
    a, b = [rnd.randrange(n) for _ in range(3)], [rnd.randrange(n) for _ in range(3)]
    ca = [mulm.encrypt(n, m, rnd.randrange(1, n)) for m in a]
    cb = [mulm.encrypt(n, m, rnd.randrange(1, n)) for m in b]
    rng = DeviceRng(key=mc.KEY, first_call=300)
    bad2 = cheating_contribution(pk, 2, cb, mc.LABEL, rng)
    c_ab, cheaters = secure_product.multiply(pk, shares, ca, cb, mc.LABEL, rng=rng, contributions={2: bad2})
    assert cheaters == [2] and [mc.decrypt(128, c) for c in c_ab] == [x * y % n for x, y in zip(a, b)]
    # taken in all the same, the cheater's E would shift the product by b
    honest = [secure_product.mask_batch(pk, i, cb, mc.LABEL, rng=rng) for i in (1, 3)]
    c_m, accepted, named = secure_product.masked_batch(pk, ca, cb, honest + [bad2], mc.LABEL)
    assert named == [2] and [c.index for c in accepted] == [1, 3]
    m = [mc.decrypt(128, c) for c in c_m]
    assert [mc.decrypt(128, c) for c in secure_product.finish_batch(pk, cb, m, accepted)] == [x * y % n for x, y in zip(a, b)]
    # a contribution under another party's name, for another label or of another length is its sender's fault alone
    stolen = secure_product.MaskContribution(3, honest[0].D, honest[0].E, honest[0].proofs)
    assert secure_product.masked_batch(pk, ca, cb, honest + [bad2, secure_product.mask_batch(pk, 2, cb, mc.LABEL, rng=rng)], mc.LABEL)[2] == [2]
    with pytest.raises(ValueError, match=r"invalid: \[2, 3\]"):
        secure_product.masked_batch(pk, ca, cb, [honest[0], bad2, stolen], mc.LABEL)
    with pytest.raises(ValueError, match=r"invalid: \[3\]"):          # (a second contribution under a name discards both)
        secure_product.masked_batch(pk, ca, cb, [honest[0], honest[1], stolen], mc.LABEL)
    # fewer than threshold + 1 valid contributions: an error that names the others
    with pytest.raises(ValueError, match=r"invalid: \[2, 3\]"):
        secure_product.masked_batch(pk, ca, cb, [honest[0], bad2, cheating_contribution(pk, 3, cb, mc.LABEL, rng)], mc.LABEL)
    with pytest.raises(ValueError, match=r"invalid: \[1, 3\]"):
        secure_product.masked_batch(pk, ca, cb, honest, b"another product")
    # an E that has no inverse stops the last step
    with pytest.raises(ValueError):
        secure_product.finish_batch(pk, cb, m, [secure_product.MaskContribution(1, honest[0].D, [n] * 3, honest[0].proofs)])


def test_the_header_declares_what_the_library_exports():
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    header = (mc.HERE.parent / "include" / "mxpaillier.h").read_text()
    assert "mx_response_mod_rows" in header
    assert hasattr(lib, "mx_response_mod_rows") and "mx_response_mod_rows" in _lib.SYMBOLS
    recip, shift = mulm.response_mod_constants(N128, 4)
    # the refusals need no GPU: they come back before anything is launched
    good = (8, 8, 8, 8, recip, shift, 8, 8, 8, 4, 4, 1)
    for k in (0, 1, 2, 3, 6, 7, 8):                # a null pointer, each in turn
        assert lib.mx_response_mod_rows(*(None if j == k else v for j, v in enumerate(good)), None) == -1, k
    for k, v in ((9, 0), (10, 0), (9, -1), (11, -1), (5, 32), (5, -1), (4, recip & 0xFFFFFFFF), (4, 1 << 33), (4, 0)):
        assert lib.mx_response_mod_rows(*(v if j == k else g for j, g in enumerate(good)), None) == -1, (k, v)
    for k, v in ((9, (1 << 20) + 1), (10, (1 << 20) + 1), (11, (256 << 31) + 1)):
        assert lib.mx_response_mod_rows(*(v if j == k else g for j, g in enumerate(good)), None) == -2, (k, v)
    assert lib.mx_response_mod_rows(*good[:11], 0, None) == 0          # a count of 0: nothing to launch
    assert lib.mx_version() == 404
