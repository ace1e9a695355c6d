"""Private-key (CRT) encryption on the GPU (csrc/mx_crt_enc.hpp, Engine.crt_prime_split_t / crt_lift_t /
private_encrypt_t / private_randomize_t / private_noise_t, the encryption side of private_key.PaillierPrivateKey), every
stage bit for bit against Python ints: the prime split against ``%``, the lift against the formulas on GIVEN noise rows, and
the whole route against ``(1 + m N) r^N mod N^2`` and ``Engine.encrypt_batch``.

Keys as in tests/test_gpu_private_key.py: synthetic.make_key at 128 (p > q), the golden primes at 1024, 2048 and 4096
(p < q) and one hand-made key with primes of 64 and 67 bits; every key also with (q, p) swapped.  Batches of 1, 2, 63, 64,
65 and 151 rows (1 and 65 at key_length 4096) are prefixes of one list per key.  The host never raises to a full-length
exponent per row: the randomness of row i is r0^i mod N, whose N-th power is (r0^N)^i, and the draws of the fresh mode
are d0^i mod N^2, whose p-th power modulo p^2 is (d0^p)^i — one ``pow`` per key and products after it."""

from __future__ import annotations

import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import crt_model as cm  # noqa: E402

BATCHES = (1, 2, 63, 64, 65, 151)
NAMES = ("k128", "k1024", "k2048", "k4096", "k64_67")
CASES = [(name, swapped) for name in NAMES for swapped in (False, True)]


class Key:
    """p, q, and per row i: a message, the randomness r0^i mod N with its noise (r0^N)^i, a draw d0^i mod N^2."""

    def __init__(self, p, q, seed):
        self.p, self.q, self.n = p, q, p * q
        n, n2 = self.n, self.n * self.n
        self.n2 = n2
        self.rng = rng = random.Random(seed)
        self.batches = (1, 65) if n.bit_length() > 4000 else BATCHES
        self.rows = max(self.batches)
        r0, d0 = rng.randrange(2, n), rng.randrange(2, n2)
        s0 = pow(r0, n, n2)
        self.r, self.rho, self.draws = [], [], []
        r, s, d = 1, 1, 1
        for _ in range(self.rows):
            r, s, d = r * r0 % n, s * s0 % n2, d * d0 % n2
            self.r.append(r)
            self.rho.append(s)
            self.draws.append(d)
        self.d0 = d0
        edge = [0, 1, n - 1, p, q, n - p, n // 2, n // 2 + 1]
        self.msgs = (edge + [rng.randrange(n) for _ in range(self.rows)])[: self.rows]
        self.cts = [(1 + m * n) * s % n2 for m, s in zip(self.msgs, self.rho)]

    def primes(self, swapped):
        return (self.q, self.p) if swapped else (self.p, self.q)

    def draw_noise(self, p, q):
        """CRT(pow(D, p, p^2), pow(D, q, q^2)) of every draw, as (rho_p list, rho_q list, rho list)."""
        p2, q2 = p * p, q * q
        ap, aq = pow(self.d0 % p2, p, p2), pow(self.d0 % q2, q, q2)
        inv = pow(p2, -1, q2)
        out_p, out_q, out = [], [], []
        xp, xq = 1, 1
        for _ in range(self.rows):
            xp, xq = xp * ap % p2, xq * aq % q2
            out_p.append(xp)
            out_q.append(xq)
            out.append(xp + p2 * ((xq - xp) * inv % q2))
        return out_p, out_q, out


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


@pytest.fixture(scope="module")
def keys():
    from protocols.distributed_keygen_amd import synthetic

    gold = json.loads((ROOT / "tests" / "golden" / "private_key_primes.json").read_text())["keys"]
    k128 = synthetic.make_key(128)
    out = {"k128": Key(k128.p, k128.q, 1), "k64_67": Key(*cm.key_of_bits(64, 67), 5)}
    for kl in (1024, 2048, 4096):
        out[f"k{kl}"] = Key(int(gold[str(kl)]["p"], 16), int(gold[str(kl)]["q"], 16), kl)
    assert out["k128"].p > out["k128"].q and out["k1024"].p < out["k1024"].q
    assert (out["k64_67"].p.bit_length(), out["k64_67"].q.bit_length()) == (64, 67)
    return out


def rows_of(eng, values, width):
    from protocols.distributed_keygen_amd import limbs

    return eng.to_device(limbs.pack(values, width))


def ints_of(eng, rows_t):
    from protocols.distributed_keygen_amd import limbs

    return limbs.unpack(eng.to_host(rows_t))


def widths(key):
    from protocols.distributed_keygen_amd import limbs

    p, q = key.p, key.q
    return limbs.limbs_for(key.n), limbs.limbs_for(key.n2), max(limbs.limbs_for(p * p), limbs.limbs_for(q * q))


def fill(values, count, make):
    return (values + [make() for _ in range(max(0, count - len(values)))])[:count]


# ------------------------------------------------------------------ the prime split
@pytest.mark.parametrize("name,swapped", CASES)
def test_prime_split_against_percent(eng, keys, name, swapped):
    key = keys[name]
    p, q = key.primes(swapped)
    ln, l2, half = widths(key)
    rng = random.Random(7)
    top = 1 << (32 * ln)
    edge = [0, 1, p, q, key.n - 1, key.n % top, top - 1, 7 * p % top, 5 * q % top, (top - 1) // p * p, (top - 1) // q * q + 1,
            rng.getrandbits(32 * ln)]
    rows = fill(edge, key.rows, lambda: rng.randrange(key.n))
    want = [[r % p for r in rows], [r % q for r in rows]]
    for b in key.batches:
        out_t = eng.crt_prime_split_t(rows_of(eng, rows[:b], ln), p, q)
        assert tuple(out_t.shape) == (2, b, half) and out_t[0].is_contiguous() and out_t[1].is_contiguous()
        assert [ints_of(eng, out_t[0]), ints_of(eng, out_t[1])] == [want[0][:b], want[1][:b]], b
    # rows three words wider than N^2, any value of that width; and rows of one word
    for width in (l2 + 3, 1):
        wide = [rng.getrandbits(32 * width) for _ in range(5)] + [(1 << (32 * width)) - 1, 0, key.n % (1 << (32 * width))]
        out_t = eng.crt_prime_split_t(rows_of(eng, wide, width), p, q)
        assert [ints_of(eng, out_t[0]), ints_of(eng, out_t[1])] == [[r % p for r in wide], [r % q for r in wide]], width


# ------------------------------------------------------------------ the lift on given noise
@pytest.mark.parametrize("name,swapped", CASES)
def test_lift_against_the_formulas_in_three_modes(eng, keys, name, swapped):
    key = keys[name]
    p, q = key.primes(swapped)
    n, n2, p2, q2 = key.n, key.n2, p * p, q * q
    ln, l2, half = widths(key)
    rng = random.Random(11)
    inv = pow(p2, -1, q2)
    # directed noise: units and extremes, rho_p above q^2 (where p > q), rho_q below c_p mod q^2 (the negative difference),
    # then the status rows
    noise = [(1, 1), (p2 - 1, q2 - 1), (p2 - 1, 1), (1, q2 - 1), (min(p2, q2) - 1, 1), (p2 - 2, 2), (0, 1), (1, 0), (0, 0),
             (0, q2 - 1), (p2 - 1, 0)]
    noise = fill(noise, key.rows, lambda: (rng.randrange(1, p2), rng.randrange(1, q2)))
    msgs = fill([0, 1, n - 1, n - 1, n - 1, 1, 5, 5, 5], key.rows, lambda: rng.randrange(n))
    cts = fill([1, n2 - 1, 0], key.rows, lambda: rng.randrange(n2))
    status = [(1 if a == 0 else 0) | (2 if b == 0 else 0) for a, b in noise]
    rho = [0 if s else a + p2 * ((b - a) * inv % q2) for (a, b), s in zip(noise, status)]
    want = {"noise": rho, "message": [(1 + m * n) * r % n2 for m, r in zip(msgs, rho)], "halves": [c * r % n2 for c, r in zip(cts, rho)]}
    rp_t, rq_t = rows_of(eng, [a for a, _ in noise], half), rows_of(eng, [b for _, b in noise], half)
    m_t, c_t = rows_of(eng, msgs, ln), rows_of(eng, cts, l2)
    for b in key.batches:
        halves_t = eng.crt_split_t(c_t[:b], p, q)
        for mode, kwargs in (("noise", {}), ("message", dict(messages_t=m_t[:b])), ("halves", dict(halves_t=halves_t))):
            out_t, st_t = eng.crt_lift_t(rp_t[:b], rq_t[:b], p, q, **kwargs)
            assert tuple(out_t.shape) == (b, l2) and st_t.cpu().tolist() == status[:b], (mode, b)
            assert ints_of(eng, out_t) == want[mode][:b], (mode, b)
    # packed rows, and message rows wider than N
    b = key.batches[-1]
    packed_t = eng.crt_lift_t(rp_t[:b], rq_t[:b], p, q, messages_t=rows_of(eng, msgs[:b], ln + 2), packed=True)
    assert tuple(packed_t.shape) == (b, l2 + 1) and packed_t[:, -1].cpu().tolist() == status[:b]
    assert ints_of(eng, packed_t[:, :l2].contiguous()) == want["message"][:b]
    with pytest.raises(ValueError):
        eng.crt_lift_t(rp_t[:2], rq_t[:2], p, q, messages_t=m_t[:2, : ln - 1])
    with pytest.raises(ValueError):
        eng.crt_lift_t(rp_t[:2], rq_t[:2], p, q, messages_t=m_t[:2], halves_t=eng.crt_split_t(c_t[:2], p, q))


# ------------------------------------------------------------------ encryption with the caller's r
@pytest.mark.parametrize("name,swapped", CASES)
def test_encrypt_with_given_randomness_is_the_reference_ciphertext(eng, keys, name, swapped):
    from protocols.distributed_keygen_amd import PaillierPrivateKey

    key = keys[name]
    p, q = key.primes(swapped)
    n = key.n
    ln, l2, _ = widths(key)
    m_t, r_t = rows_of(eng, key.msgs, ln), rows_of(eng, key.r, ln)
    for b in key.batches:
        out_t, st_t = eng.private_encrypt_t(m_t[:b], p, q, randomness_t=r_t[:b])
        assert tuple(out_t.shape) == (b, l2) and not bool(st_t.any()), b
        assert ints_of(eng, out_t) == key.cts[:b], b
    b = key.batches[-1] if len(key.batches) == 2 else 63
    seq_t, _ = eng.private_encrypt_t(m_t[:b], p, q, randomness_t=r_t[:b], side_by_side=False)
    assert ints_of(eng, seq_t) == key.cts[:b]
    # the existing route on the same (m, r); r + 3 N in rows one word wider is the same randomness
    assert eng.encrypt_batch(key.msgs[:b], key.r[:b], n) == key.cts[:b]
    wide_t, _ = eng.private_encrypt_t(m_t[:2], p, q, randomness_t=rows_of(eng, [r + 3 * n for r in key.r[:2]], ln + 1))
    assert ints_of(eng, wide_t) == key.cts[:2]
    noise_t, st_t = eng.private_noise_t(2, p, q, randomness_t=r_t[:2])
    assert ints_of(eng, noise_t) == key.rho[:2] and not bool(st_t.any())
    # randomness that shares a factor with N: a status and a zero row, ValueError at the int level
    bad = [key.r[0], 0, 7 * p, 5 * q, key.r[4 % key.rows], n]
    msgs = [3, 4, 5, 6, key.msgs[4 % key.rows], 7]
    out_t, st_t = eng.private_encrypt_t(rows_of(eng, msgs, ln), p, q, randomness_t=rows_of(eng, bad, ln + 1))
    good = [(1 + 3 * n) * key.rho[0] % key.n2, 0, 0, 0, (1 + msgs[4] * n) * key.rho[4 % key.rows] % key.n2, 0]
    assert st_t.cpu().tolist() == [0, 3, 1, 2, 0, 3] and ints_of(eng, out_t) == good
    pk = PaillierPrivateKey(p, q, engine=eng)
    with pytest.raises(ValueError, match="shares a factor"):
        pk.encrypt_batch(msgs, bad)
    assert pk.encrypt_batch(msgs, bad, return_ok=True) == (good, [True, False, False, False, True, False])
    assert pk.encrypt_batch(key.msgs[:3], key.r[:3]) == key.cts[:3]


@pytest.mark.parametrize("name,swapped", [("k128", False), ("k64_67", True), ("k1024", False), ("k2048", True), ("k4096", False)])
def test_fixed_window_reaches_all_four_modexps(eng, keys, name, swapped):
    """Under set_fixed_window(True) the modexps modulo the primes leave the shared-exponent route, whose sliding-window
    schedule is a function of the secret q mod (p-1), for the fixed-window ladder of powmod_multi_t, and the two modulo the
    squares get fixed-window plans — the same ciphertexts bit for bit."""
    key = keys[name]
    p, q = key.primes(swapped)
    ln, _, _ = widths(key)
    m_t, r_t = rows_of(eng, key.msgs, ln), rows_of(eng, key.r, ln)

    def refuse(*args, **kwargs):
        raise AssertionError("powmod_shared_t builds a schedule from the exponent's bits")

    eng.set_fixed_window(True)
    eng.powmod_shared_t = refuse
    try:
        got = {b: ints_of(eng, eng.private_encrypt_t(m_t[:b], p, q, randomness_t=r_t[:b])[0]) for b in (1, 65)}
        seq = ints_of(eng, eng.private_encrypt_t(m_t[:2], p, q, randomness_t=r_t[:2], side_by_side=False)[0])
        noise = ints_of(eng, eng.private_noise_t(2, p, q, randomness_t=r_t[:2])[0])
    finally:
        del eng.powmod_shared_t
        eng.set_fixed_window(False)
    assert got == {1: key.cts[:1], 65: key.cts[:65]} and seq == key.cts[:2] and noise == key.rho[:2]
    assert (p, p, True) in eng._n2_plans and (q, q, True) in eng._n2_plans
    with pytest.raises(AssertionError):                      # and without the setting the shared-exponent route is what runs
        eng.powmod_shared_t = refuse
        try:
            eng.private_encrypt_t(m_t[:1], p, q, randomness_t=r_t[:1])
        finally:
            del eng.powmod_shared_t


# ------------------------------------------------------------------ fresh randomness
@pytest.mark.parametrize("name,swapped", CASES)
def test_fresh_mode_with_given_draws_and_rerandomisation(eng, keys, name, swapped):
    key = keys[name]
    p, q = key.primes(swapped)
    n, n2 = key.n, key.n2
    ln, l2, half = widths(key)
    _, _, rho = key.draw_noise(p, q)
    want = [(1 + m * n) * r % n2 for m, r in zip(key.msgs, rho)]
    again = [c * r % n2 for c, r in zip(key.cts, rho)]
    m_t, d_t, c_t = rows_of(eng, key.msgs, ln), rows_of(eng, key.draws, l2), rows_of(eng, key.cts, l2)
    for b in key.batches:
        out_t, st_t = eng.private_encrypt_t(m_t[:b], p, q, draws_t=d_t[:b])
        assert not bool(st_t.any()) and ints_of(eng, out_t) == want[:b], b
        out_t, st_t = eng.private_randomize_t(c_t[:b], p, q, draws_t=d_t[:b])
        assert not bool(st_t.any()) and ints_of(eng, out_t) == again[:b], b
    b = key.batches[-1] if len(key.batches) == 2 else 65
    seq_t, _ = eng.private_encrypt_t(m_t[:b], p, q, draws_t=d_t[:b], side_by_side=False)
    assert ints_of(eng, seq_t) == want[:b]
    dec_t, st_t = eng.private_decrypt_t(eng.private_randomize_t(c_t[:b], p, q, draws_t=d_t[:b])[0], p, q)
    assert ints_of(eng, dec_t) == key.msgs[:b] and not bool(st_t.any())
    # draws of bits(N) + 64 bits, as the generator gives them, against pow; a draw that is a multiple of p^2
    rng = random.Random(21)
    draws = [rng.getrandbits(n.bit_length() + 64) for _ in range(2)] + [3 * p * p]
    out_t, st_t, kept_t = eng.private_encrypt_t(m_t[:3], p, q, draws_t=rows_of(eng, draws, l2 + 2), return_randomness=True)
    p2, q2 = p * p, q * q
    ref = [pow(d % p2, p, p2) + p2 * ((pow(d % q2, q, q2) - pow(d % p2, p, p2)) * pow(p2, -1, q2) % q2) for d in draws[:2]]
    assert ints_of(eng, out_t) == [(1 + m * n) * r % n2 for m, r in zip(key.msgs, ref)] + [0]
    assert st_t.cpu().tolist() == [0, 0, 1] and ints_of(eng, kept_t) == draws


@pytest.mark.parametrize("name,swapped", CASES)
def test_fresh_mode_with_the_device_generator(eng, keys, name, swapped):
    from protocols.distributed_keygen_amd.device_rng import DeviceRng

    key = keys[name]
    p, q = key.primes(swapped)
    n, n2 = key.n, key.n2
    ln, l2, _ = widths(key)
    b = 65 if key.n.bit_length() > 1000 else 151
    rng = DeviceRng(bytes(range(32)))
    m_t = rows_of(eng, key.msgs[:b], ln)
    one_t, st1_t, d_t = eng.private_encrypt_t(m_t, p, q, rng=rng, return_randomness=True)
    two_t, st2_t = eng.private_encrypt_t(m_t, p, q, rng=rng)
    assert not bool(st1_t.any()) and not bool(st2_t.any())
    one, two = ints_of(eng, one_t), ints_of(eng, two_t)
    assert len(set(one + two)) == 2 * b
    draws = ints_of(eng, d_t)
    assert max(d.bit_length() for d in draws) <= n.bit_length() + 64 and len(set(draws)) == b
    for cts_t in (one_t, two_t):
        dec_t, st_t = eng.private_decrypt_t(cts_t, p, q)
        assert ints_of(eng, dec_t) == key.msgs[:b] and not bool(st_t.any())
    # the noise is an N-th residue: its lambda-th power is 1
    lam = (p - 1) * (q - 1)
    for e in ((0,) if n.bit_length() > 4000 else (0, b - 1)):
        assert pow(one[e] * (1 - key.msgs[e] * n) % n2, lam, n2) == 1
    rr_t, st_t = eng.private_randomize_t(one_t, p, q, rng=rng)
    assert ints_of(eng, rr_t) != one and not bool(st_t.any())
    assert ints_of(eng, eng.private_decrypt_t(rr_t, p, q)[0]) == key.msgs[:b]
    for kwargs in ({}, dict(rng=rng, draws_t=d_t), dict(randomness_t=m_t, rng=rng)):
        with pytest.raises(ValueError, match="exactly one"):
            eng.private_encrypt_t(m_t, p, q, **kwargs)


# ------------------------------------------------------------------ the key object
@pytest.mark.parametrize("name", ("k128", "k64_67", "k2048"))
def test_key_object_round_trip_with_negative_messages(eng, keys, name):
    from protocols.distributed_keygen_amd import PaillierPrivateKey

    key = keys[name]
    pk = PaillierPrivateKey(key.p, key.q, engine=eng)
    n = key.n
    msgs = [0, 1, -1, n // 2, -(n // 2), 12345, -98765, n - 3, n + 4]
    want = [m % n - n if m % n > n // 2 else m % n for m in msgs]
    fresh = pk.encrypt_batch(msgs)
    assert pk.decrypt_batch(fresh, signed=True) == want and len(set(fresh)) == len(msgs)
    assert pk.encrypt_batch(msgs) != fresh
    given = pk.encrypt_batch(msgs, key.r[: len(msgs)])
    assert given == [(1 + (m % n) * n) * s % key.n2 for m, s in zip(msgs, key.rho)]
    assert pk.decrypt_batch(pk.randomize_batch(given), signed=True) == want
    assert pk.randomize_batch(given, key.r[: len(msgs)]) == [c * s % key.n2 for c, s in zip(given, key.rho)]
    assert pk.decrypt(pk.encrypt(-7), signed=True) == -7
    ln = widths(key)[0]
    m_t, r_t = rows_of(eng, [m % n for m in msgs], ln), rows_of(eng, key.r[: len(msgs)], ln)
    packed_t = pk.encrypt_t(m_t, randomness_t=r_t, side_by_side=False, packed=True)
    assert ints_of(eng, packed_t[:, :-1].contiguous()) == given and not bool(packed_t[:, -1].any())
    d_t = rows_of(eng, key.draws[: len(msgs)], widths(key)[1])
    assert ints_of(eng, pk.encrypt_t(m_t, draws_t=d_t)[0]) == ints_of(eng, eng.private_encrypt_t(m_t, key.p, key.q, draws_t=d_t)[0])
    assert ints_of(eng, pk.noise_t(2, draws_t=d_t[:2])[0]) == key.draw_noise(key.p, key.q)[2][:2]
    assert pk.encrypt_batch([]) == [] and pk.randomize_batch([], []) == []
    cts, ok, rs = eng.private_encrypt_batch(msgs[:3], key.p, key.q, randomness=[2, 0, 3], return_randomness=True)
    assert ok == [True, False, True] and rs == [2, 0, 3] and cts[1] == 0
    cts, ok, draws = eng.private_encrypt_batch(msgs, key.p, key.q, rng=pk._rng(None, None), return_randomness=True)
    p2, q2 = key.p**2, key.q**2
    rho = [pow(d % p2, key.p, p2) + p2 * ((pow(d % q2, key.q, q2) - pow(d % p2, key.p, p2)) * pow(p2, -1, q2) % q2) for d in draws[:2]]
    assert all(ok) and cts[:2] == [(1 + (m % n) * n) * r % key.n2 for m, r in zip(msgs, rho)]


def test_slot_packed_scores_of_a_key_holder(eng, keys):
    """encrypt_slots_t -> homomorphic.matmul -> decrypt_t -> slots.decode_t at key_length 128 against plaintext integers."""
    import torch

    from protocols.distributed_keygen_amd import PaillierPrivateKey, homomorphic, packing, slots

    key = keys["k128"]
    pk = PaillierPrivateKey(key.p, key.q, engine=eng)
    n = key.n
    B, I, R = 23, 3, 2
    rng = np.random.default_rng(3)
    x = rng.integers(-128, 128, size=(B, I))
    W = rng.integers(-255, 256, size=(R, I))
    bias = rng.integers(-1023, 1024, size=R)
    b = slots.slot_bits_for(8, 8, I, 10)
    k = packing.slots_per_ciphertext(n, b)
    J = -(-B // k)
    assert J > 1
    cols = []
    for f in range(I):
        rows_t, st_t = pk.encrypt_slots_t(np.ascontiguousarray(x[:, f]), b)
        assert tuple(rows_t.shape) == (J, widths(key)[1]) and not bool(st_t.any())
        cols.append(ints_of(eng, rows_t))
    assert pk.decrypt_batch(cols[0]) == slots.encode(np.ascontiguousarray(x[:, 0]), n, b, engine=eng)
    assert len(pk.encrypt_slots(np.ascontiguousarray(x[:, 0]), b)) == J
    packed_bias = [slots.encode([int(v)] * k, n, b, engine=eng)[0] for v in bias]
    out = homomorphic.matmul([[cols[f][j] for f in range(I)] for j in range(J)], W.tolist(), n=n, bias=packed_bias, engine=eng)
    flat = [out[j][r] for r in range(R) for j in range(J)]
    rows_t, st_t = pk.decrypt_t(rows_of(eng, flat, widths(key)[1]))
    assert not bool(st_t.any())
    scores = torch.stack([slots.decode_t(rows_t[r * J : (r + 1) * J], n, b, B, engine=eng) for r in range(R)], dim=1)
    assert (scores.cpu().numpy() == x @ W.T + bias).all()
