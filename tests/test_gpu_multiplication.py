"""The response kernel modulo M (csrc/mx_response_mod.hpp) and the multiplication proofs over it on the GPU —
Engine.response_mod_rows_t / mul_prove_t / mul_verify_t, multiplication.py and secure_product.py — bit for bit against
Python divmod and tools/mul_model.py.

The engine entries take any N the wide draws fit under, so the row-by-row comparison runs at the 128-bit golden key (the
module itself refuses moduli below 260 bits); the end-to-end cases run at 1024 and 2048 bits."""

from __future__ import annotations

import random

import pytest

pytestmark = pytest.mark.gpu

import mul_cases as mc  # noqa: E402
from mul_cases import mulm  # noqa: E402
from mul_engine import tamperings, zero_forgeries  # noqa: E402

N128 = mc.modulus(128)


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def rows_of(eng, values, width):
    from protocols.distributed_keygen_amd import limbs

    return eng.to_device(limbs.pack(list(values), width).reshape(len(values), width))


def ints_of(eng, rows_t):
    from protocols.distributed_keygen_amd import limbs

    return limbs.unpack(eng.to_host(rows_t.contiguous()))


# ------------------------------------------------------------------ the response kernel
@pytest.mark.parametrize("wn", [4, 9, 32, 64, 128])
def test_response_mod_rows_equal_python_divmod(eng, wn):
    """Every kind of modulus of wn words; the directed rows (s on and beside multiples of M, the largest row) placed among
    257 rows of a launch of two workgroups; rows with rho or x at or above M raise the status and keep the residue."""
    for name, mod in mc.moduli(wn):
        rows = mc.response_rows(mod, wn, 257)
        rnd = random.Random(wn)
        rnd.shuffle(rows)                                           # (the directed rows spread over both workgroups)
        for count in (1, 63, 64, 65, 257) if name == "random odd" else (257,):
            part = rows[:count] if count > 1 else rows[-1:]
            rho_t, e_t, x_t = (rows_of(eng, [r[j] for r in part], w) for j, w in ((0, wn), (1, 4), (2, wn)))
            w_t, t_t, status_t = eng.response_mod_rows_t(rho_t, e_t, x_t, mod)
            want = mc.expected(part, mod)
            assert ints_of(eng, w_t) == want[0], (name, count)
            assert ints_of(eng, t_t) == want[1], (name, count)
            assert [int(s) for s in status_t.cpu()] == want[2], (name, count)
            assert (ints_of(eng, rho_t), ints_of(eng, e_t), ints_of(eng, x_t)) == tuple([r[j] for r in part] for j in range(3))      # inputs untouched
        if mod < (1 << (32 * wn)) - 1:
            assert sum(want[2]) >= 1                                # (the rows at or above M are there and raise it)
        assert [s for (rho, e, x), s in zip(rows, want[2]) if rho < mod and x < mod] == [0] * sum(1 for rho, e, x in rows if rho < mod and x < mod)


def test_response_mod_other_challenge_widths(eng):
    """ew = 1, 3 and ew = wn (the width the reduction of c_b modulo N uses), with operands anywhere in their rows."""
    rnd = random.Random(6)
    for wn, ew in ((4, 1), (9, 3), (4, 4), (9, 9), (32, 32)):
        for name, mod in mc.moduli(wn)[:4]:
            rows = [(rnd.getrandbits(32 * wn), rnd.getrandbits(32 * ew), rnd.getrandbits(32 * wn)) for _ in range(65)]
            rows[0] = ((1 << (32 * wn)) - 1, (1 << (32 * ew)) - 1, (1 << (32 * wn)) - 1)
            w_t, t_t, status_t = eng.response_mod_rows_t(*(rows_of(eng, [r[j] for r in rows], w) for j, w in ((0, wn), (1, ew), (2, wn))), mod)
            want = mc.expected(rows, mod, ew)
            assert (ints_of(eng, w_t), ints_of(eng, t_t), [int(s) for s in status_t.cpu()]) == want, (wn, ew, name)


def test_response_mod_refusals_launch_nothing(eng):
    import torch

    wn, mod = 4, N128
    rows = mc.response_rows(mod, wn, 4)
    rho_t, e_t, x_t = (rows_of(eng, [r[j] for r in rows], 4) for j in range(3))
    out_t = torch.zeros_like(rho_t)
    for bad in (lambda: eng.response_mod_rows_t(rho_t, e_t, x_t, mod, out_t=rho_t),                    # an aliased output
                lambda: eng.response_mod_rows_t(rho_t, e_t, x_t, mod, out_t=x_t),
                lambda: eng.response_mod_rows_t(rho_t, e_t, x_t, mod, out_t=e_t),
                lambda: eng.response_mod_rows_t(rho_t, e_t, x_t, mod, out_t=x_t.view(4, 4)),                   # ... through a view
                lambda: eng.response_mod_rows_t(rho_t, e_t, x_t, mod, out_t=out_t[:2].contiguous()),
                lambda: eng.response_mod_rows_t(rho_t, e_t[:2].contiguous(), x_t, mod),
                lambda: eng.response_mod_rows_t(rho_t, e_t, x_t[:, :3].contiguous(), mod),
                lambda: eng.response_mod_rows_t(rho_t, e_t, x_t, mod >> 32),                             # a modulus narrower than the rows
                lambda: eng.response_mod_rows_t(rho_t, e_t, x_t, mod << 32),
                lambda: eng.response_mod_rows_t(rho_t, e_t, x_t, 0),
                lambda: eng.response_mod_rows_t(rho_t.to(torch.int64), e_t, x_t, mod)):
        with pytest.raises(ValueError):
            bad()
    empty = eng.response_mod_rows_t(rho_t[:0].contiguous(), e_t[:0].contiguous(), x_t[:0].contiguous(), mod)
    assert [tuple(t.shape) for t in empty] == [(0, 4), (0, 4), (0,)]
    # the C entry itself: bad arguments come back as a status, before anything is launched
    lib = eng.lib
    recip, shift = eng.response_mod_constants(mod, wn)
    assert (recip, shift) == mulm.response_mod_constants(mod, wn)
    mod_t = rows_of(eng, [mod], wn)
    t_t = torch.zeros_like(e_t)
    st = torch.full((4,), 7, dtype=torch.uint8, device=eng.device)
    names = ("rho", "e", "x", "mod", "recip", "shift", "w", "t", "status", "wn", "ew", "count", "stream")
    good = [rho_t.data_ptr(), e_t.data_ptr(), x_t.data_ptr(), mod_t.data_ptr(), recip, shift, out_t.data_ptr(), t_t.data_ptr(), st.data_ptr(), wn, 4, 4, None]

    def run(**change):
        args = list(good)
        for key, v in change.items():
            args[names.index(key)] = v
        return lib.mx_response_mod_rows(*args)

    for change in (dict(rho=None), dict(e=None), dict(x=None), dict(mod=None), dict(w=None), dict(t=None), dict(status=None), dict(wn=0), dict(ew=0),
                   dict(wn=-1), dict(count=-1), dict(shift=32), dict(shift=-1), dict(recip=0), dict(recip=recip - (1 << 32)), dict(recip=1 << 33)):
        assert run(**change) == -1, change
    for change in (dict(wn=(1 << 20) + 1), dict(ew=(1 << 20) + 1), dict(count=(256 << 31) + 1)):
        assert run(**change) == -2, change
    assert run(count=0) == 0
    eng.synchronize()
    assert not bool(out_t.any()) and not bool(t_t.any()) and [int(s) for s in st.cpu()] == [7] * 4


# ------------------------------------------------------------------ the proofs
def verdicts(eng, n, ca, cb, d, cols, label):
    """multiplication.verify_batch without the module's refusal of short moduli: received ints -> rows -> mul_verify_t."""
    from protocols.distributed_keygen_amd import multiplication

    proofs = multiplication.MultiplicationProofs.from_ints(*cols, n)
    sh = multiplication.shape(n)
    wide = [multiplication._rows_of(col, sh["limbs2"]) for col in (ca, cb, d)]
    got = eng.mul_verify_t(*(eng.to_device(rows) for rows, _ in wide), *(eng.to_device(t) for t in proofs.rows()), n, multiplication.context(n, label))
    return [bool(g) and not u and all(fit[r] for _, fit in wide) for r, (g, u) in enumerate(zip(got.cpu(), proofs.unfit))]


def test_proofs_at_the_smallest_key_equal_the_model_row_for_row(eng):
    from protocols.distributed_keygen_amd import DeviceRng, multiplication

    n, count = N128, 65
    sh = eng.mul_shape(n)
    a, ra, gamma, b, ca, cb = mc.statements(n, count)
    ctx = multiplication.context(n, mc.LABEL)
    assert ctx == mulm.context(n, mc.LABEL) and sh == mulm.shape(n) == multiplication.shape(n)
    ca_t, cb_t = rows_of(eng, ca, sh["limbs2"]), rows_of(eng, cb, sh["limbs2"])
    rows = eng.mul_prove_t(ca_t, cb_t, rows_of(eng, a, sh["limbs_n"]), rows_of(eng, ra, sh["limbs_n"]), rows_of(eng, gamma, sh["limbs_n"]), n, ctx,
                           rng=DeviceRng(key=mc.KEY, first_call=40))
    assert [tuple(t.shape) for t in rows] == [(count, sh["limbs2"])] * 3 + [(count, sh["limbs_n"])] * 3
    want_d, want = mc.model_proofs(n, mc.LABEL, a, ra, gamma, ca, cb, 40)
    d = ints_of(eng, rows[0])
    got = multiplication.MultiplicationProofs(*rows[1:]).to_ints()
    assert d == want_d
    for field, g, w in zip(multiplication.MultiplicationProofs.FIELDS, got, want):
        assert g == w, field
    assert [mc.decrypt(128, v) for v in d] == [x * y % n for x, y in zip(a, b)]
    assert [bool(v) for v in eng.mul_verify_t(ca_t, cb_t, *rows, n, ctx).cpu()] == [True] * count
    # the same rows with the draws passed in: bit for bit again
    xs, us, vs = mulm.device_draws(mc.KEY, 40, count, n)
    again = eng.mul_prove_t(ca_t, cb_t, rows_of(eng, a, sh["limbs_n"]), rows_of(eng, ra, sh["limbs_n"]), rows_of(eng, gamma, sh["limbs_n"]), n, ctx,
                            draws=(rows_of(eng, xs, sh["limbs2"]), rows_of(eng, us + vs, sh["limbs2"])))
    assert all(bool((x == y).all()) for x, y in zip(again, rows))
    # verdicts per row: every tampering spoils row 1 of the first three rows and nothing else
    cols = tuple(list(col[:3]) for col in got)
    for what, tca, tcb, td, *tcols in tamperings(n, cols, ca[:3], cb[:3], d[:3]):
        assert verdicts(eng, n, tca, tcb, td, tcols, mc.LABEL) == [True, False, True], what
    # the zero forgeries against a d that holds a b + 1: both equations hold, only the refusal of zero stops them
    alpha = (a[1] + pow(b[1], -1, n)) % n
    wrong_d, forged = zero_forgeries(n, mc.LABEL, ca[1], cb[1], a[1], ra[1], alpha, gamma[1], [xs[3], us[3], vs[3]])
    assert mc.decrypt(128, wrong_d) == (a[1] * b[1] + 1) % n
    for what, proof in forged:
        fcols = [[cols[j][0], proof[j], cols[j][2]] for j in range(5)]
        assert verdicts(eng, n, ca[:3], cb[:3], [d[0], wrong_d, d[2]], fcols, mc.LABEL) == [True, False, True], what
    assert verdicts(eng, n, ca[:3], cb[:3], d[:3], cols, b"another session") == [False] * 3
    assert verdicts(eng, n + 2, ca[:3], cb[:3], d[:3], cols, mc.LABEL) == [False] * 3
    with pytest.raises(ValueError):                                                  # an a that is not below n
        eng.mul_prove_t(ca_t, cb_t, rows_of(eng, [n] * count, sh["limbs_n"]), rows_of(eng, ra, sh["limbs_n"]), rows_of(eng, gamma, sh["limbs_n"]),
                        n, ctx, rng=DeviceRng())
    with pytest.raises(ValueError):                                                  # and the module refuses a modulus this short
        multiplication.prove_batch(n, a, ra, gamma, cb, mc.LABEL, engine=eng)


@pytest.mark.parametrize("key_length", [1024, 2048])
def test_multiply_with_proof_end_to_end_with_cheating_rows(eng, key_length):
    from protocols.distributed_keygen_amd import DeviceRng, multiplication

    n = mc.modulus(key_length)
    n2 = n * n
    a, ra, gamma, b, ca, cb = mc.statements(n, 9)
    c_a, d, proofs = multiplication.multiply_with_proof(n, a, cb, mc.LABEL, rng=DeviceRng(key=mc.KEY, first_call=5), engine=eng)
    assert multiplication.verify_batch(n, c_a, cb, d, proofs, mc.LABEL, engine=eng) == [True] * 9
    cols = proofs.to_ints()
    assert mulm.verify(n, mc.LABEL, c_a[4], cb[4], d[4], [col[4] for col in cols])          # the model accepts one of the engine's proofs
    cheat_d, cheat_a, cheat_b = list(d), list(c_a), list(cb)
    cheat_d[5] = d[5] * (1 + n) % n2                                                    # a b + 1
    cheat_a[6] = c_a[6] * (1 + n) % n2                                                  # the proof is for another a
    cheat_b[7] = cb[7] * (1 + n) % n2                                                   # and for another b
    received = multiplication.MultiplicationProofs.from_ints(*cols, n)
    assert multiplication.verify_batch(n, cheat_a, cheat_b, cheat_d, received, mc.LABEL, engine=eng) == [True] * 5 + [False] * 3 + [True]
    assert multiplication.verify_batch(n, c_a, cb, d, received, b"another session", engine=eng) == [False] * 9


def test_the_product_of_two_ciphertexts_with_one_cheater(eng):
    from protocols.distributed_keygen_amd import DeviceRng, secure_product, threshold

    class Key:
        p, q = mc.primes(1024)

    pk, shares = threshold.deal(Key, 3, 1, rng=random.Random(11), check=False, engine=eng)
    n = pk.n
    rnd = random.Random(2)
    a = [0, 1, n - 1] + [rnd.randrange(n) for _ in range(5)]
    b = [rnd.randrange(n) for _ in range(5)] + [0, 1, n - 1]
    ca = [mulm.encrypt(n, m, rnd.randrange(1, n)) for m in a]
    cb = [mulm.encrypt(n, m, rnd.randrange(1, n)) for m in b]
    rng = DeviceRng(key=mc.KEY, first_call=200)
    good = secure_product.mask_batch(pk, 2, cb, mc.LABEL, rng=rng)
    bad2 = secure_product.MaskContribution(2, good.D, [e * c % pk.n_square for e, c in zip(good.E, cb)], good.proofs)          # E holds (d + 1) b
    c_ab, cheaters = secure_product.multiply(pk, shares, ca, cb, mc.LABEL, rng=rng, contributions={2: bad2})
    assert cheaters == [2]
    assert [mc.decrypt(1024, c) for c in c_ab] == [x * y % n for x, y in zip(a, b)]
