"""Private-key (CRT) decryption on the host side: the model of the two kernels (tools/crt_model.py) against ``pow`` and
``%``, ``PaillierPrivateKey`` over the model-backed double of tests/crt_engine.py, and the refusals of the C ABI that
need no launch.  No GPU."""

from __future__ import annotations

import ctypes
import math
import random
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import crt_model as cm  # noqa: E402

from crt_engine import CrtEngine  # noqa: E402
from protocols.distributed_keygen_amd import limbs, synthetic  # noqa: E402
from protocols.distributed_keygen_amd.private_key import PaillierPrivateKey, crt_constants  # noqa: E402
from protocols.distributed_keygen_amd.shared_key import PlainCiphertext  # noqa: E402

P64, Q67 = cm.key_of_bits(64, 67)


def _keys():
    k128, k1024 = synthetic.make_key(128), synthetic.make_key(1024)
    assert k128.p > k128.q and k1024.p < k1024.q and (k128.n.bit_length(), P64.bit_length(), Q67.bit_length()) == (131, 64, 67)
    return [(k128.p, k128.q), (k128.q, k128.p), (k1024.p, k1024.q), (k1024.q, k1024.p), (P64, Q67), (Q67, P64)]


KEYS = _keys()


def encrypt(p, q, m, rng):
    n = p * q
    return (1 + m * n) * pow(rng.randrange(1, n), n, n * n) % (n * n)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("idx", range(len(KEYS)))
def test_model_agrees_with_pow_and_the_formulas_in_both_prime_orders(idx):
    p, q = KEYS[idx]
    assert cm.check(p, q) == 30 and cm.check(p, q, extra_words=2) == 30


def test_model_at_key_length_2048():
    key = synthetic.make_key(2048)
    rng = random.Random(3)
    plan = cm.CrtPlan(key.p, key.q)
    lam = (key.p - 1) * (key.q - 1)
    for c in synthetic.random_ciphertexts(key, 2) + [encrypt(key.p, key.q, key.n - 1, rng)]:
        assert plan.split(c) == (c % key.p**2, c % key.q**2)
        assert plan.decrypt(c) == ((pow(c, lam, key.n_square) - 1) // key.n * pow(lam, -1, key.n) % key.n, 0)


@pytest.mark.parametrize("bits", [(64, 67), (67, 64), (30, 101), (101, 30), (300, 261), (5, 9), (261, 262)])
def test_model_bounds_hold_for_unequal_prime_lengths(bits):
    """One radix from the longer prime: q^2 wider than p^2 (other limb counts, other block counts) stays inside every
    bound the kernels rely on — the model asserts each of them on the way."""
    p, q = cm.key_of_bits(*bits)
    plan = cm.CrtPlan(p, q)
    assert (1 << plan.rs) >= 16 * max(p * p, q * q) and (1 << plan.r1) >= 16 * max(p, q)
    assert plan.split_bit + 4 <= plan.rs and 32 * plan.limbs2 - plan.split_bit + 4 <= plan.rs
    assert cm.check(p, q, seed=11) == 30


def test_model_recombines_the_directed_pairs():
    for p, q in KEYS[:2] + KEYS[4:]:
        plan = cm.CrtPlan(p, q)
        n = p * q
        big, small = max(p, q), min(p, q)
        # plaintexts that make m_p = m_q, m_q < m_p mod q, m_p >= q (when p > q) and a negative difference
        for m in (0, 5, small - 1, small, big - 1, big % small, n - 1, small + 1, (big - 1) % n, n - small):
            xp, xq = pow(1 + n, m, p * p), pow(1 + n, m, q * q)         # (1 + N)^m: x with L(x) h = m modulo the prime
            xp, xq = pow(xp, p - 1, p * p), pow(xq, q - 1, q * q)
            assert plan.recombine(xp, xq) == (m, 0)
        assert plan.recombine(1, 1) == (0, 0)
        assert plan.recombine(2, 1) == (0, 1) and plan.recombine(1, 2) == (0, 2) and plan.recombine(0, 0) == (0, 3)


# ------------------------------------------------------------------ the key object
def test_constructor_refusals():
    p, q = KEYS[0]
    for bad in ((p + 1, q), (p, q - 1), (2, q), (p, p), (1, q)):
        with pytest.raises(ValueError):
            PaillierPrivateKey(*bad)
    with pytest.raises(ValueError):            # q = 2 p + 1: p divides q - 1
        PaillierPrivateKey(11, 23)
    assert math.gcd(11 * 23, 10 * 22) != 1
    key = PaillierPrivateKey(p, q, engine=CrtEngine())
    assert key.n == p * q and (key.h_p, key.h_q, key.p_inv) == crt_constants(p, q)
    assert key.h_p == cm.h_constant(p, p * q) and key.p_inv * p % q == 1


@pytest.mark.parametrize("idx", range(len(KEYS)))
def test_decrypt_batch_signed_and_status(idx):
    p, q = KEYS[idx]
    n = p * q
    rng = random.Random(idx)
    eng = CrtEngine()
    key = PaillierPrivateKey(p, q, engine=eng)
    msgs = [0, 1, n - 1, p, q, p - 1, q - 1, n - p, n - q, n // 2, n // 2 + 1, rng.randrange(n)]
    cts = [encrypt(p, q, m, rng) for m in msgs]
    assert key.decrypt_batch(cts) == msgs
    assert key.decrypt_batch(iter(cts), signed=True) == [m - n if m > n // 2 else m for m in msgs]
    assert key.decrypt(cts[2], signed=True) == -1
    # c + k N^2 is the same ciphertext; c = 1 and N^2 - 1 decrypt to 0
    assert key.decrypt_batch([cts[3] + 5 * n * n, 1, n * n - 1]) == [p, 0, 0]
    bad = [cts[0], 0, cts[1], 7 * p, 3 * q, cts[2]]
    with pytest.raises(ValueError, match="valid ciphertext"):
        key.decrypt_batch(bad)
    got, ok = key.decrypt_batch(bad, return_ok=True, signed=True)
    assert ok == [True, False, True, False, False, True] and got == [0, 0, 1, 0, 0, -1]
    assert key.decrypt_batch(cts, return_ok=True) == (msgs, [True] * len(msgs))


def test_empty_batch_and_objects_with_get_value():
    p, q = KEYS[0]
    n = p * q
    rng = random.Random(9)
    eng = CrtEngine()
    key = PaillierPrivateKey(p, q, engine=eng)
    assert key.decrypt_batch([]) == [] and key.decrypt_batch([], return_ok=True) == ([], [])
    assert key.decrypt_sequence([]) == [] and eng.calls == []
    objs = [PlainCiphertext(encrypt(p, q, m, rng), n) for m in (7, n - 3)]
    assert all(o.fresh for o in objs)
    assert key.decrypt_sequence(objs + [encrypt(p, q, 11, rng)], signed=True) == [7, -3, 11]
    assert not any(o.fresh for o in objs)                      # get_value(), not peek_value()
    other = CrtEngine()
    assert key.decrypt_batch([objs[0].value], engine=other) == [7] and other.calls[0] == ("decrypt", 1)


def test_decrypt_t_returns_rows_in_the_format_of_combine_t():
    p, q = KEYS[4]
    n = p * q
    rng = random.Random(2)
    eng = CrtEngine()
    key = PaillierPrivateKey(p, q, engine=eng)
    msgs = [3, n - 1, p]
    rows = eng.to_device(limbs.pack([encrypt(p, q, m, rng) for m in msgs] + [0], limbs.limbs_for(n * n)))
    out, status = key.decrypt_t(rows)
    assert out.shape == (4, limbs.limbs_for(n)) and out.dtype == torch.int32
    assert limbs.unpack(eng.to_host(out)) == msgs + [0] and status.tolist() == [0, 0, 0, 3]
    assert eng.calls == [("split", 4), ("powmod_nsquare", 4), ("powmod_nsquare", 4), ("recombine", 4, False)]


# ------------------------------------------------------------------ the C ABI, without a launch
def test_abi_refusals_need_no_gpu():
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    p, q = KEYS[4]
    h_p, h_q, p_inv = crt_constants(p, q)
    lw = limbs.limbs_for(max(p, q))
    limbs2 = limbs.limbs_for((p * q) ** 2)
    rows = {k: limbs.pack_one(v, lw) for k, v in dict(p=p, q=q, hp=h_p, hq=h_q, pinv=p_inv, even=p + 1).items()}
    ptr = {k: r.ctypes.data for k, r in rows.items()}
    plan = _lib.CrtPlan()
    block = (ctypes.c_uint32 * 4)()                              # never written: every call below returns before a launch
    dp = ctypes.addressof(block)
    ok = [ctypes.byref(plan), ptr["p"], ptr["q"], ptr["hp"], ptr["hq"], ptr["pinv"], lw, limbs2, dp, 1 << 20, None]

    def prepare(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return lib.mx_crt_prepare(*args)

    ARG, SIZE, MODULUS, WORKSPACE = -1, -2, -3, -4
    for slot in (0, 1, 2, 3, 4, 5, 8):
        assert prepare(**{f"a{slot}": None}) == ARG, slot
    assert prepare(a6=0) == ARG and prepare(a6=-1) == ARG and prepare(a7=0) == ARG
    assert prepare(a1=ptr["even"]) == MODULUS and prepare(a2=ptr["even"]) == MODULUS
    assert prepare(a2=ptr["p"]) == ARG                                         # p == q
    assert prepare(a7=limbs2 - 1) == ARG                                       # rows too narrow for N^2
    assert prepare(a7=5000) == SIZE                                            # rows no lane group stages
    assert prepare(a9=16) == WORKSPACE
    wide = 270                                                                 # squares beyond the engine's widest modulus (16700 bits)
    big = {k: limbs.pack_one(v, wide) for k, v in dict(p=(1 << (32 * wide - 1)) + 1, q=(1 << (32 * wide - 2)) + 1, one=1).items()}
    assert lib.mx_crt_prepare(ctypes.byref(plan), big["p"].ctypes.data, big["q"].ctypes.data, big["one"].ctypes.data,
                              big["one"].ctypes.data, big["one"].ctypes.data, wide, 4 * wide, dp, 1 << 30, None) == SIZE
    assert lib.mx_crt_plan_bytes(0, 4) == ARG and lib.mx_crt_plan_bytes(4, 0) == ARG
    assert lib.mx_crt_plan_bytes(lw, limbs2) >= 12 * limbs.limbs_for(max(p, q) ** 2) * 4
    # the runs: a plan that was never prepared, null rows, no rows
    plan = _lib.CrtPlan()
    assert lib.mx_crt_split_run(ctypes.byref(plan), dp, dp, 1, None) == ARG
    assert lib.mx_crt_split_run(None, dp, dp, 1, None) == ARG
    plan.d_plan, plan.limbs, plan.limbs2, plan.limbs_half, plan.limbs_n = dp, lw, limbs2, 5, 5
    plan.p_bits, plan.q_bits = 64, 67
    for args in ((None, dp, 1), (dp, None, 1), (dp, dp, 0), (dp, dp, -3)):
        assert lib.mx_crt_split_run(ctypes.byref(plan), *args, None) == ARG, args
    for args in ((None, dp, dp, 5, dp, 1), (dp, None, dp, 5, dp, 1), (dp, dp, None, 5, dp, 1), (dp, dp, dp, 5, dp, 0),
                 (dp, dp, dp, 4, dp, 1),                                       # out_stride below limbs(N)
                 (dp, dp, dp, 5, None, 1)):                                    # no place for the status
        assert lib.mx_crt_recombine_run(ctypes.byref(plan), *args, None) == ARG, args
    assert lib.mx_crt_split_run(ctypes.byref(plan), dp, dp, 1 << 40, None) == SIZE      # more rows than a launch addresses
    assert lib.mx_version() == 404
