"""Private-key (CRT) encryption on the host side: the model of the prime split and the lift (tools/crt_model.py:
CrtEncPlan) against ``pow`` and ``%``, the identity r^N = CRT(rho_p, rho_q) it rests on, ``PaillierPrivateKey`` over the
model-backed double of tests/crt_enc_engine.py, and the refusals of the C ABI that need no launch.  No GPU."""

from __future__ import annotations

import ctypes
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import crt_model as cm  # noqa: E402

from crt_enc_engine import CrtEncEngine, FakeRng  # noqa: E402
from crt_engine import _ints  # noqa: E402
from protocols.distributed_keygen_amd import limbs, synthetic  # noqa: E402
from protocols.distributed_keygen_amd.private_key import PaillierPrivateKey  # noqa: E402

P64, Q67 = cm.key_of_bits(64, 67)


def _keys():
    gold = json.loads((ROOT / "tests" / "golden" / "private_key_primes.json").read_text())["keys"]
    k128 = synthetic.make_key(128)
    out = [(k128.p, k128.q), (P64, Q67)] + [(int(gold[kl]["p"], 16), int(gold[kl]["q"], 16)) for kl in ("1024", "2048", "4096")]
    return [pair[::o] for pair in out for o in (1, -1)]


KEYS = _keys()
MEDIUM = [k for k in KEYS if (k[0] * k[1]).bit_length() < 1100]
SHORT = [k for k in KEYS if (k[0] * k[1]).bit_length() < 200]          # the keys the double runs whole batches on


def crt(p, q, rho_p, rho_q):
    p2, q2 = p * p, q * q
    return rho_p + p2 * ((rho_q - rho_p) * pow(p2, -1, q2) % q2)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("idx", range(len(MEDIUM)))
def test_model_agrees_with_pow_and_the_formulas_in_both_prime_orders(idx):
    """enc_check: prime split, the lift in its three modes on directed noise, the status rows, fresh draws — every bound
    of the kernels asserted on the way.  (Full-width ``pow`` makes it seconds per key from key_length 2048: the two longest
    golden keys go through the directed tests below, which need none.)"""
    p, q = MEDIUM[idx]
    assert cm.enc_check(p, q, extra_words=3) == 34
    assert cm.enc_check(p, q, seed=11) >= 33


@pytest.mark.parametrize("idx", range(len(KEYS)))
def test_prime_split_of_edge_rows(idx):
    p, q = KEYS[idx]
    n = p * q
    rng = random.Random(idx)
    for width in (limbs.limbs_for(n), limbs.limbs_for(n * n) + 3, 1):
        plan = cm.CrtEncPlan(p, q, width)
        top = 1 << (32 * width)
        for r in (0, 1, p, q, n - 1, n, top - 1, rng.getrandbits(32 * width)):
            r %= top
            assert plan.prime_split(r) == (r % p, r % q), (width, r)
        assert (1 << plan.rp) >= 16 * max(p, q) and plan.split_bit + 4 <= plan.rp and 32 * width - plan.split_bit + 4 <= plan.rp


@pytest.mark.parametrize("idx", range(len(KEYS)))
def test_lift_in_three_modes_on_directed_noise(idx):
    p, q = KEYS[idx]
    n, p2, q2 = p * q, p * p, q * q
    rng = random.Random(100 + idx)
    plan = cm.CrtEncPlan(p, q)
    assert (1 << plan.r2) >= 16 * max(p2, q2)
    c0 = rng.randrange(n * n)
    noise = [(1, 1), (p2 - 1, q2 - 1), (rng.randrange(1, p2), rng.randrange(1, q2)),
             (p2 - 1, 1),                                    # rho_p above q^2 where p > q
             (min(p2, q2) - 1, 1), (p2 - 2, 2)]              # rho_q below c_p mod q^2: the negative difference
    for rho_p, rho_q in noise:
        rho = crt(p, q, rho_p, rho_q)
        assert rho % p2 == rho_p and rho % q2 == rho_q and plan.lift(rho_p, rho_q) == (rho, 0)
        for m in (0, 1, n - 1, rng.randrange(n)):
            assert plan.lift(rho_p, rho_q, m=m) == ((1 + m * n) * rho % (n * n), 0)
        assert plan.lift(rho_p, rho_q, halves=(c0 % p2, c0 % q2)) == (c0 * rho % (n * n), 0)
    for rho_p, rho_q, status in ((0, 1, 1), (1, 0, 2), (0, 0, 3), (0, q2 - 1, 1), (p2 - 1, 0, 2)):
        assert plan.lift(rho_p, rho_q) == (0, status) and plan.lift(rho_p, rho_q, m=n - 1) == (0, status)
        assert plan.lift(rho_p, rho_q, halves=(1, 1)) == (0, status)


@pytest.mark.parametrize("idx", range(len(KEYS)))
def test_two_short_chains_give_r_to_the_n(idx):
    """CRT(rho_p, rho_q) == pow(r, N, N^2) with rho_p = ((r mod p)^(q mod (p-1)) mod p)^p mod p^2."""
    p, q = KEYS[idx]
    n = p * q
    rng = random.Random(200 + idx)
    plan = cm.CrtEncPlan(p, q, limbs.limbs_for(n) + 1)
    assert (plan.e_p, plan.e_q) == (q % (p - 1), p % (q - 1)) == (n % (p - 1), n % (q - 1))
    r0 = rng.randrange(2, n)
    for r in (1, 2, n - 1, r0, r0 + 3 * n):
        rho_p, rho_q = plan.noise_of_r(r)
        full = pow(r, n, n * n)
        assert (rho_p, rho_q) == (full % (p * p), full % (q * q))
        assert plan.lift(rho_p, rho_q) == (full, 0) == (crt(p, q, rho_p, rho_q), 0)
    for r, status in ((0, 3), (7 * p, 1), (5 * q, 2), (n, 3)):
        assert plan.encrypt(5, r) == (0, status)


@pytest.mark.parametrize("idx", range(len(SHORT)))
def test_fresh_draws_are_nth_residues_that_decrypt(idx):
    p, q = SHORT[idx]
    n, lam = p * q, (p - 1) * (q - 1)
    rng = random.Random(300 + idx)
    plan = cm.CrtEncPlan(p, q)
    for _ in range(6):
        draw = rng.getrandbits(n.bit_length() + 64)
        rho, status = plan.lift(*plan.noise_of_draw(draw))
        assert status == 0 and pow(rho, lam, n * n) == 1
        m = rng.randrange(n)
        c, _ = plan.lift(*plan.noise_of_draw(draw), m=m)
        assert cm.lambda_decrypt(c, p, q) == m
        r = pow(rho, pow(n, -1, lam), n)                     # how r is recovered from rho
        assert pow(r, n, n * n) == rho


# ------------------------------------------------------------------ the key object over the double
@pytest.mark.parametrize("idx", range(len(SHORT)))
def test_encrypt_batch_with_given_randomness(idx):
    p, q = SHORT[idx]
    n = p * q
    n2 = n * n
    rng = random.Random(idx)
    eng = CrtEncEngine()
    key = PaillierPrivateKey(p, q, engine=eng)
    msgs = [0, 1, n - 1, -1, -(n // 2), p, q, rng.randrange(n), n + 5]
    rs = [1, 2, n - 1, rng.randrange(1, n), rng.randrange(1, n) + 3 * n, p + 1, q + 1, rng.randrange(1, n), -2]
    want = [(1 + (m % n) * n) * pow(r % n, n, n2) % n2 for m, r in zip(msgs, rs)]
    assert key.encrypt_batch(msgs, rs) == want
    assert key.encrypt_batch(iter(msgs), iter(rs), return_ok=True) == (want, [True] * len(msgs))
    assert key.encrypt(msgs[3], rs[3]) == want[3]
    assert key.decrypt_batch(want, signed=True) == [m % n - n if m % n > n // 2 else m % n for m in msgs]
    # randomness that shares a factor with N
    bad_r = [rs[0], 0, 7 * p, 5 * q, rs[1]]
    with pytest.raises(ValueError, match="shares a factor"):
        key.encrypt_batch(msgs[:5], bad_r)
    got, ok = key.encrypt_batch(msgs[:5], bad_r, return_ok=True)
    assert ok == [True, False, False, False, True] and got == [want[0], 0, 0, 0, (1 + (msgs[4] % n) * n) * pow(rs[1], n, n2) % n2]
    with pytest.raises(ValueError, match="one randomness per message"):
        key.encrypt_batch(msgs, rs[:-1])
    # re-randomisation
    cts = want[:4]
    assert key.randomize_batch(cts, rs[:4]) == [c * pow(r % n, n, n2) % n2 for c, r in zip(cts, rs)]
    with pytest.raises(ValueError, match="one randomness per ciphertext"):
        key.randomize_batch(cts, rs[:3])
    with pytest.raises(ValueError, match="shares a factor"):
        key.randomize_batch(cts[:1], [3 * q])


def test_fresh_mode_empty_batches_and_return_randomness():
    p, q = SHORT[0]
    n = p * q
    n2 = n * n
    eng = CrtEncEngine()
    key = PaillierPrivateKey(p, q, engine=eng)
    assert key.encrypt_batch([]) == [] and key.encrypt_batch([], return_ok=True) == ([], [])
    assert key.randomize_batch([], []) == [] and eng.calls == []
    rng = FakeRng(4)
    msgs = [5, -7, n - 1, 0]
    a = key.encrypt_batch(msgs, rng=rng)
    b = key.encrypt_batch(msgs, rng=rng)
    assert a != b and len(set(a + b)) == 8
    assert rng.calls[0] == (4, n.bit_length() + 64, max(limbs.limbs_for(n2), (n.bit_length() + 95) // 32))
    assert key.decrypt_batch(a, signed=True) == [5, -7, -1, 0] == key.decrypt_batch(b, signed=True)
    again = key.randomize_batch(a, rng=rng)
    assert again != a and key.decrypt_batch(again, signed=True) == [5, -7, -1, 0]
    # the engine level: exactly one source of randomness; the randomness comes back
    for kwargs in ({}, dict(randomness=[1] * 4, rng=rng)):
        with pytest.raises(ValueError, match="exactly one"):
            eng.private_encrypt_batch(msgs, p, q, **kwargs)
    cts, ok, draws = eng.private_encrypt_batch(msgs, p, q, rng=FakeRng(9), return_randomness=True)
    ref = FakeRng(9).rng
    assert draws == [ref.getrandbits(n.bit_length() + 64) for _ in msgs] and ok == [True] * 4
    assert cts == [(1 + (m % n) * n) * crt(p, q, pow(d, p, p * p), pow(d, q, q * q)) % n2 for m, d in zip(msgs, draws)]
    cts, ok, rs = eng.private_encrypt_batch(msgs, p, q, randomness=[3, 4, 5, 6], return_randomness=True)
    assert rs == [3, 4, 5, 6] and cts == [(1 + (m % n) * n) * pow(r, n, n2) % n2 for m, r in zip(msgs, rs)]
    assert eng.private_encrypt_batch([], p, q, rng=rng, return_randomness=True) == ([], [], [])
    m_t = eng.to_device(limbs.pack([1, 2], limbs.limbs_for(n)))
    d_t = eng.to_device(limbs.pack([11, 12], limbs.limbs_for(n2)))
    for kwargs in ({}, dict(rng=rng, draws_t=d_t), dict(randomness_t=m_t, draws_t=d_t), dict(randomness_t=m_t, rng=rng, draws_t=d_t)):
        with pytest.raises(ValueError, match="exactly one"):
            eng.private_encrypt_t(m_t, p, q, **kwargs)
    with pytest.raises(ValueError, match="one draw per ciphertext"):
        eng.private_encrypt_t(m_t, p, q, draws_t=d_t[:1])
    with pytest.raises(ValueError, match="no narrower than N"):
        eng.private_encrypt_t(m_t[:, :-1], p, q, draws_t=d_t)


def test_tensor_level_formats_of_the_key_object():
    p, q = SHORT[2]
    n = p * q
    n2 = n * n
    eng = CrtEncEngine()
    key = PaillierPrivateKey(p, q, engine=eng)
    msgs, rs = [3, n - 1, p, 9], [2, 3, 5 * q, 0]
    rows_t = lambda values, words: eng.to_device(limbs.pack(values, words))
    rows, status = key.encrypt_t(rows_t(msgs, limbs.limbs_for(n)), randomness_t=rows_t(rs, limbs.limbs_for(n)))
    assert rows.shape == (4, limbs.limbs_for(n2)) and rows.dtype == torch.int32 and status.tolist() == [0, 0, 2, 3]
    assert _ints(rows) == [(1 + msgs[0] * n) * pow(2, n, n2) % n2, (1 + msgs[1] * n) * pow(3, n, n2) % n2, 0, 0]
    again, status = key.randomize_t(rows[:2], randomness_t=rows_t([7, 8], limbs.limbs_for(n) + 2))
    assert _ints(again) == [c * pow(r, n, n2) % n2 for c, r in zip(_ints(rows[:2]), (7, 8))] and not status.any()
    noise, status = key.noise_t(2, randomness_t=rows_t([7, 8], limbs.limbs_for(n)))
    assert _ints(noise) == [pow(7, n, n2), pow(8, n, n2)] and not status.any()
    packed = eng.private_noise_t(2, p, q, draws_t=rows_t([p * p * 3, 5], limbs.limbs_for(n2)), packed=True)
    assert packed.shape == (2, limbs.limbs_for(n2) + 1) and packed[:, -1].tolist() == [1, 0] and not packed[0, :-1].any()
    assert [name for name, *_ in eng.calls].count("lift") == 4


def test_fixed_window_moves_the_prime_modexps_off_the_shared_exponent_schedule():
    """Engine._powmod_prime_t: powmod_shared_t's sliding-window schedule is a function of the secret exponent's bits; with
    set_fixed_window the launch is powmod_multi_t with one group, the generic kernel's fixed-window ladder."""
    from protocols.distributed_keygen_amd.engine import Engine

    class Stub:
        _fixed_window = False

        def __init__(self):
            self.calls = []

        def powmod_shared_t(self, rows_t, mod, exp):
            self.calls.append(("shared", mod, exp))
            return "shared"

        def powmod_multi_t(self, rows_t, mods, exps, group_size):
            self.calls.append(("multi", mods, exps, group_size))
            return "multi"

    rows = np.zeros((7, 3), dtype=np.uint32)
    stub = Stub()
    assert Engine._powmod_prime_t(stub, rows, 101, 13) == "shared"
    stub._fixed_window = True
    assert Engine._powmod_prime_t(stub, rows, 101, 13) == "multi"
    assert stub.calls == [("shared", 101, 13), ("multi", [101], [13], 7)]


@pytest.mark.parametrize("idx", range(len(SHORT)))
def test_fixed_window_route_inside_an_encryption(idx):
    """With the fixed window the two modexps modulo the primes of a real encryption go through powmod_multi_t with one
    group — nothing else changes, and the ciphertexts are the same bit for bit."""
    p, q = SHORT[idx]
    n = p * q
    rnd = random.Random(400 + idx)
    msgs, rs = [0, n - 1, rnd.randrange(n)], [1, n - 1, rnd.randrange(1, n)]
    runs = []
    for fixed in (False, True):
        eng = CrtEncEngine()
        eng._fixed_window = fixed
        rows, status = eng.private_encrypt_t(eng.to_device(limbs.pack(msgs, limbs.limbs_for(n))), p, q,
                                             randomness_t=eng.to_device(limbs.pack(rs, limbs.limbs_for(n))))
        assert not status.any()
        runs.append((rows, eng.calls))
    assert torch.equal(runs[0][0], runs[1][0]) and _ints(runs[0][0]) == [(1 + m * n) * pow(r, n, n * n) % (n * n) for m, r in zip(msgs, rs)]
    assert runs[0][1] == [("prime_split", 3), ("powmod_shared", 3), ("powmod_nsquare", 3), ("powmod_shared", 3), ("powmod_nsquare", 3),
                          ("lift", 3, "message")]
    assert runs[1][1] == [("prime_split", 3), ("powmod_multi", 1, 3, (q % (p - 1)).bit_length()), ("powmod_nsquare", 3),
                          ("powmod_multi", 1, 3, (p % (q - 1)).bit_length()), ("powmod_nsquare", 3), ("lift", 3, "message")]


def test_key_object_forwards_the_engine_keywords():
    p, q = SHORT[0]
    n = p * q
    eng = CrtEncEngine()
    key = PaillierPrivateKey(p, q, engine=eng)
    m_t = eng.to_device(limbs.pack([4, 5], limbs.limbs_for(n)))
    d_t = eng.to_device(limbs.pack([11, 12], limbs.limbs_for(n * n)))
    packed = key.encrypt_t(m_t, draws_t=d_t, side_by_side=False, packed=True)
    assert packed.shape == (2, limbs.limbs_for(n * n) + 1) and not packed[:, -1].any()
    rows, status = eng.private_encrypt_t(m_t, p, q, draws_t=d_t)
    assert (packed[:, :-1] == rows).all()
    rows2, _, kept = key.randomize_t(rows, draws_t=d_t, return_randomness=True)
    assert _ints(kept) == [11, 12] and _ints(rows2) != _ints(rows)
    assert key.noise_t(2, draws_t=d_t, packed=True).shape == packed.shape


# ------------------------------------------------------------------ the C ABI, without a launch
def test_abi_refusals_need_no_gpu():
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    p, q = P64, Q67
    lw = limbs.limbs_for(max(p, q))
    n = p * q
    limbs_n, limbs2 = limbs.limbs_for(n), limbs.limbs_for(n * n)
    rows = dict(p=limbs.pack_one(p, lw), q=limbs.pack_one(q, lw), even=limbs.pack_one(p + 1, lw),
                inv=limbs.pack_one(pow(p * p, -1, q * q), 2 * lw))
    ptr = {k: r.ctypes.data for k, r in rows.items()}
    plan = _lib.CrtEncPlan()
    block = (ctypes.c_uint32 * 4)()                              # never written: every call below returns before a launch
    dp = ctypes.addressof(block)
    ok = [ctypes.byref(plan), ptr["p"], ptr["q"], ptr["inv"], lw, limbs_n, dp, 1 << 20, None]

    def prepare(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return lib.mx_crt_enc_prepare(*args)

    ARG, SIZE, MODULUS, WORKSPACE = -1, -2, -3, -4
    for slot in (0, 1, 2, 3, 6):
        assert prepare(**{f"a{slot}": None}) == ARG, slot
    assert prepare(a4=0) == ARG and prepare(a4=-1) == ARG and prepare(a5=0) == ARG and prepare(a5=-2) == ARG
    assert prepare(a1=ptr["even"]) == MODULUS and prepare(a2=ptr["even"]) == MODULUS
    assert prepare(a2=ptr["p"]) == ARG                                         # p == q
    assert prepare(a5=5000) == SIZE                                            # randomness rows no lane group stages
    assert prepare(a7=16) == WORKSPACE
    wide = 270                                                                 # squares beyond the engine's widest modulus
    big = {k: limbs.pack_one(v, wide) for k, v in dict(p=(1 << (32 * wide - 1)) + 1, q=(1 << (32 * wide - 2)) + 1).items()}
    one = limbs.pack_one(1, 2 * wide)
    assert lib.mx_crt_enc_prepare(ctypes.byref(plan), big["p"].ctypes.data, big["q"].ctypes.data, one.ctypes.data, wide, 2 * wide,
                                  dp, 1 << 30, None) == SIZE
    assert lib.mx_crt_enc_plan_bytes(0, 4) == ARG and lib.mx_crt_enc_plan_bytes(4, 0) == ARG
    assert lib.mx_crt_enc_plan_bytes(lw, limbs_n) >= 15 * limbs.limbs_for(max(p, q) ** 2) * 4
    # the runs: a plan that was never prepared, null rows, no rows
    plan = _lib.CrtEncPlan()
    assert lib.mx_crt_prime_split_run(ctypes.byref(plan), dp, dp, 1, None) == ARG
    assert lib.mx_crt_prime_split_run(None, dp, dp, 1, None) == ARG
    assert lib.mx_crt_lift_run(ctypes.byref(plan), dp, dp, None, 0, None, dp, limbs2, dp, 1, None) == ARG
    plan.d_plan, plan.limbs, plan.limbs_r, plan.limbs2, plan.limbs_half, plan.limbs_n = dp, lw, limbs_n, limbs2, 5, limbs_n
    plan.p_bits, plan.q_bits = 64, 67
    for args in ((None, dp, 1), (dp, None, 1), (dp, dp, 0), (dp, dp, -3)):
        assert lib.mx_crt_prime_split_run(ctypes.byref(plan), *args, None) == ARG, args
    good = [dp, dp, dp, limbs_n, None, dp, limbs2, dp, 1]
    for slot, value in ((0, None), (1, None), (5, None), (8, 0), (8, -1),
                        (4, dp),                                               # a message and a ciphertext
                        (3, limbs_n - 1),                                      # message rows narrower than N
                        (6, limbs2 - 1),                                       # out_stride below limbs(N^2)
                        (7, None)):                                            # no place for the status
        args = list(good)
        args[slot] = value
        assert lib.mx_crt_lift_run(ctypes.byref(plan), *args, None) == ARG, slot
    assert lib.mx_crt_prime_split_run(ctypes.byref(plan), dp, dp, 1 << 40, None) == SIZE    # more rows than a launch addresses
    assert lib.mx_crt_lift_run(ctypes.byref(plan), *good[:8], 1 << 40, None) == SIZE
    assert lib.mx_version() == 404
