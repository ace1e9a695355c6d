"""Additive shares of the prime candidates and their Shamir sharings on the GPU (csrc/mx_share.hpp,
Engine.prime_candidates_t / shamir_share_t, shamir.generate_pq_t): bit for bit against tools/share_model.py — Python
``%`` and Horner on ints — for host-supplied and for device-drawn rows, in every lane geometry.

Moduli: the Shamir primes of tests/golden/reconstruct.json (key_length 64 and 128: one lane per element, 1024: four,
2048: eight) and, for the wider groups, odd numbers of the right length (the comparison is with ``%``, so any odd modulus
serves): 262 bits (two lanes), 4103 bits (sixteen), 8204 bits (thirty-two) and 8401 bits (sixty-four, the widest group).
The point sets are [1,2,3], [1..5] and [2,5,9,65535]; none of them has the nine points a sharing of degree 8 needs, so
[1..9] is there for that degree."""

from __future__ import annotations

import itertools
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import share_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes((7 * k + 3) & 0xFF for k in range(32))
FIXTURES = json.loads((ROOT / "tests" / "golden" / "reconstruct.json").read_text())
MODULI = {label: int(case["prime"], 16) for label, case in FIXTURES.items()}
MODULI.update({"odd262": (1 << 261) + 0x1F1, "odd4103": (1 << 4102) + 0x1F1, "odd8204": (1 << 8203) + 0x1F1,
               "odd8401": (1 << 8400) + 0x1F1})
POINT_SETS = ([1, 2, 3], [1, 2, 3, 4, 5], [2, 5, 9, 65535], list(range(1, 10)))
DEGREES = (1, 2, 4, 8)


def lanes(prime):
    """Lanes per element of the 9-limb geometry (csrc/mx_host.hpp: choose_geometry)."""
    nblk = -(-(prime.bit_length() + 4) // (29 * 9))
    k = 1
    while k < nblk:
        k *= 2
    return k


def test_the_moduli_cover_every_group_width():
    assert sorted(lanes(p) for p in MODULI.values()) == [1, 1, 2, 4, 8, 16, 32, 64]


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def make_rng(first_call=0, key=KEY):
    from protocols.distributed_keygen_amd.device_rng import DeviceRng

    return DeviceRng(key=key, first_call=first_call)


def rows_t(eng, values, words):
    from protocols.distributed_keygen_amd import limbs

    return eng.to_device(limbs.pack(list(values), words))


def draws_t(eng, draws, prime):
    from protocols.distributed_keygen_amd import limbs

    cw = sm.coefficient_words(prime)
    return eng.to_device(np.stack([limbs.pack(list(col), cw) for col in draws]))


def shares_of(eng, out_t):
    from protocols.distributed_keygen_amd import limbs

    host = eng.to_host(out_t)
    return [limbs.unpack(host[j]) for j in range(host.shape[0])]


def edge_draws(prime):
    return [0, prime - 1, prime, prime + 1, (1 << sm.coefficient_bits(prime)) - 1]


# ------------------------------------------------------------------ host-supplied draws, bit-exact against the model
BATCH_KINDS = ("one", "ragged", "second_wavefront", "several_workgroups")


def batch_of(kind, prime):
    return {"one": 1, "ragged": 7, "second_wavefront": 64 // lanes(prime) + 1, "several_workgroups": 300}[kind]


@pytest.mark.parametrize("kind", BATCH_KINDS)
@pytest.mark.parametrize("label", sorted(MODULI))
def test_shares_equal_the_model_for_host_supplied_draws(eng, label, kind):
    import torch

    prime = MODULI[label]
    batch = batch_of(kind, prime)
    rng = random.Random(f"{label}/{kind}")
    bits, limbs = sm.coefficient_bits(prime), (prime.bit_length() + 31) // 32
    edge = edge_draws(prime)
    ran = 0
    for points in POINT_SETS:
        for degree in DEGREES:
            if degree + 1 > len(points) or (points == POINT_SETS[3] and degree != 8):
                continue
            secrets = [rng.randrange(prime) for _ in range(batch)]
            secrets[0] = 0 if degree % 2 else prime - 1
            secrets[-1] = prime - 1 if degree % 2 else 0
            draws = [[rng.getrandbits(bits) for _ in range(batch)] for _ in range(degree)]
            for k in range(degree):                              # every edge draw somewhere, also at batch 1
                for e in range(min(batch, 5)):
                    draws[k][e] = edge[(e + k + ran) % 5]
            out_t = eng.shamir_share_t(rows_t(eng, secrets, limbs), prime, degree, points, draws_t=draws_t(eng, draws, prime))
            assert out_t.dtype == torch.int32 and tuple(out_t.shape) == (len(points), batch, limbs)
            assert shares_of(eng, out_t) == sm.shamir_share(secrets, draws, prime, points), (degree, points)
            ran += 1
    assert ran == 8


@pytest.mark.parametrize("label", sorted(MODULI))
def test_edge_draws_edge_secrets_and_the_sharing_of_zero(eng, label):
    prime = MODULI[label]
    limbs = (prime.bit_length() + 31) // 32
    edge = edge_draws(prime)
    points = [1, 2, 3, 4, 5]
    for degree in (1, 4):
        # element i: every coefficient drawn as edge[i % 5]; the secrets 0 and P - 1 against each of them
        draws = [[edge[i % 5] for i in range(10)] for _ in range(degree)]
        secrets = [0] * 5 + [prime - 1] * 5
        d_t = draws_t(eng, draws, prime)
        got = shares_of(eng, eng.shamir_share_t(rows_t(eng, secrets, limbs), prime, degree, points, draws_t=d_t))
        assert got == sm.shamir_share(secrets, draws, prime, points)
        assert all(0 <= v < prime for col in got for v in col)
        zero = shares_of(eng, eng.shamir_share_t(None, prime, degree, points, batch=10, draws_t=d_t))
        assert zero == sm.shamir_share([0] * 10, draws, prime, points)
        assert zero == shares_of(eng, eng.shamir_share_t(rows_t(eng, [0] * 10, limbs), prime, degree, points, draws_t=d_t))
    # an output tensor of the caller's, wider than the prime needs: the upper words are written as zero
    wide = eng.torch.full((5, 10, limbs + 2), -1, dtype=eng.torch.int32, device=eng.device)
    back = eng.shamir_share_t(rows_t(eng, secrets, limbs + 2), prime, 4, points, draws_t=d_t, out_t=wide)
    assert back is wide and shares_of(eng, wide) == sm.shamir_share(secrets, draws, prime, points)


# ------------------------------------------------------------------ device-drawn coefficients
@pytest.mark.parametrize("label,batch,degree,first_call", [
    ("k128_n5_t2", 70, 2, 0), ("k2048_n5_t2", 9, 4, (1 << 64) + 5), ("k1024_n3_t1", 17, 1, 3), ("odd262", 33, 3, 1 << 33)])
def test_device_drawn_coefficients_are_the_models_rows(eng, label, batch, degree, first_call):
    prime = MODULI[label]
    limbs = (prime.bit_length() + 31) // 32
    points = [1, 2, 3, 4, 5]
    rng = make_rng(first_call)
    secrets = [random.Random(label).randrange(prime) for _ in range(batch)]
    out_t = eng.shamir_share_t(rows_t(eng, secrets, limbs), prime, degree, points, rng=rng)
    assert rng.next_call == first_call + 1
    assert shares_of(eng, out_t) == sm.shamir_share(secrets, sm.device_draws(KEY, first_call, degree, batch, prime), prime, points)
    zero_t = eng.shamir_share_t(None, prime, degree, points, batch=batch, rng=rng)
    assert rng.next_call == first_call + 2
    assert shares_of(eng, zero_t) == sm.shamir_share(None, sm.device_draws(KEY, first_call + 1, degree, batch, prime), prime, points)
    # the int-level form: one more call, shares by point
    by_point = eng.shamir_share_batch(secrets, prime, degree, points, make_rng(first_call))
    assert [by_point[x] for x in points] == shares_of(eng, out_t)


# ------------------------------------------------------------------ polynomial properties
def test_every_subset_of_degree_plus_one_points_reconstructs_the_secret(eng):
    from protocols.distributed_keygen_amd import shamir

    prime = MODULI["k128_n5_t2"]
    secrets = [0, prime - 1] + [random.Random(9).randrange(prime) for _ in range(6)]
    points = [1, 2, 3, 4, 5]
    by_point = eng.shamir_share_batch(secrets, prime, 2, points, make_rng(40))
    for subset in itertools.combinations(points, 3):
        assert shamir.reconstruct_batch({x: by_point[x] for x in subset}, prime, 2, engine=eng) == secrets, subset


@pytest.mark.parametrize("label,degree", [("k64_n3_t1", 1), ("k1024_n3_t1", 4), ("k2048_n5_t2", 8)])      # prime moduli: Lagrange divides
def test_the_degree_is_not_higher_than_asked_for(eng, label, degree):
    """Two different degree+1-subsets of degree+2 points interpolate to the same value (the secret): a polynomial of a
    higher degree through these points would not."""
    from protocols.distributed_keygen_amd import shamir

    prime = MODULI[label]
    secrets = [random.Random(degree).randrange(prime) for _ in range(5)]
    points = [3, 1, 7, 2, 11, 5, 4, 9, 6, 8][: degree + 2]
    by_point = eng.shamir_share_batch(secrets, prime, degree, points, make_rng(77))
    first, last = points[: degree + 1], points[1:]
    assert shamir.reconstruct_batch({x: by_point[x] for x in first}, prime, degree, engine=eng) == secrets
    assert shamir.reconstruct_batch({x: by_point[x] for x in last}, prime, degree, engine=eng) == secrets


# ------------------------------------------------------------------ candidates
@pytest.mark.parametrize("count", [1, 65, 4097])
@pytest.mark.parametrize("prime_length", [8, 32, 35, 64, 67, 512, 1024, 2048])
def test_candidates_equal_the_model(eng, prime_length, count):
    import torch

    from protocols.distributed_keygen_amd import limbs

    bits = prime_length - 3
    in_words, words = (bits + 31) // 32, (prime_length + 31) // 32
    raw = np.random.default_rng(prime_length * 10007 + count).integers(0, 1 << 32, size=(count, in_words), dtype=np.uint64).astype("<u4")
    if bits % 32:
        raw[:, -1] &= np.uint32((1 << (bits % 32)) - 1)
    raw[0, :] = 0                                                 # r = 0 and r = 2^(L-3) - 1 among them
    if count > 1:
        raw[1, :] = 0xFFFFFFFF
        if bits % 32:
            raw[1, -1] = (1 << (bits % 32)) - 1
    r_ints = limbs.unpack(raw)
    for first in (True, False):
        out_t = eng.prime_candidates_t(count, prime_length, first, random_t=eng.to_device(raw))
        assert out_t.dtype == torch.int32 and tuple(out_t.shape) == (count, words)
        got = limbs.unpack(eng.to_host(out_t))
        assert got == [sm.candidate(r, prime_length, first) for r in r_ints]
        assert all(v.bit_length() == prime_length and v % 4 == (3 if first else 0) for v in got)
    # rows wider than needed are zero-filled
    wide_t = eng.prime_candidates_t(count, prime_length, True, random_t=eng.to_device(raw), row_words=words + 3)
    wide = eng.to_host(wide_t)
    assert wide.shape == (count, words + 3) and not wide[:, words:].any()
    assert limbs.unpack(wide) == [sm.candidate(r, prime_length, True) for r in r_ints]


@pytest.mark.parametrize("prime_length,count,first_call", [(67, 65, 0), (8, 300, 1 << 40), (512, 7, 12)])
def test_device_drawn_candidates_are_the_models(eng, prime_length, count, first_call):
    rng = make_rng(first_call)
    for k, first in enumerate((True, False)):
        got = eng.prime_candidates_batch(count, prime_length, first, rng)
        assert rng.next_call == first_call + k + 1
        assert got == sm.device_candidates(KEY, first_call + k, count, prime_length, first)


# ------------------------------------------------------------------ a round in small
def test_a_round_in_small_gives_the_product_of_the_summed_additive_shares(eng):
    """Five parties at the key_length 128 fixture's prime (n = 5, t = 2, prime length 64, 9 candidates): generate_pq_t
    per party, every party sums what it received, multiplies and adds on the device, and the five results interpolate
    to (sum p_additive) * (sum q_additive) for every candidate."""
    import torch

    from protocols.distributed_keygen_amd import shamir

    prime, n, t, length, batch = MODULI["k128_n5_t2"], 5, 2, 64, 9
    made = [shamir.generate_pq_t(i, length, prime, n, t, batch, make_rng(0, key=bytes([i] * 32)), engine=eng) for i in range(1, n + 1)]
    p_add = [eng._download_ints(m[0]) for m in made]
    q_add = [eng._download_ints(m[1]) for m in made]
    assert all(v % 4 == (3 if i == 0 else 0) and v.bit_length() == length for i in range(n) for v in p_add[i] + q_add[i])
    n_shares = {}
    for j in range(1, n + 1):
        received = {name: torch.stack([m[2][name][j - 1] for m in made]) for name in ("p", "q", "zero")}
        p_j, q_j, zero_j = (shamir.sum_shares_t(received[name], prime, engine=eng) for name in ("p", "q", "zero"))
        n_shares[j] = eng._download_ints(eng.shamir_fma_t(p_j, q_j, zero_j, prime))
    moduli = shamir.reconstruct_batch(n_shares, prime, 2 * t, engine=eng, points=[1, 2, 3, 4, 5])
    assert moduli == [sum(p[k] for p in p_add) * sum(q[k] for q in q_add) for k in range(batch)]
    # the int-level form of the same generator gives the same numbers
    p1, q1, shares1 = shamir.generate_pq_batch(1, length, prime, n, t, batch, make_rng(0, key=bytes([1] * 32)), engine=eng)
    assert (p1, q1, shares1) == sm.generate_pq(bytes([1] * 32), 0, 1, length, prime, n, t, batch)
    assert shamir.sum_shares_batch([shares1["zero"][j] for j in range(1, n + 1)], prime, engine=eng) == [
        sum(shares1["zero"][j][k] for j in range(1, n + 1)) % prime for k in range(batch)]


# ------------------------------------------------------------------ refusals
def test_refusals_come_before_any_draw(eng):
    prime = MODULI["k128_n5_t2"]
    limbs, cw = (prime.bit_length() + 31) // 32, sm.coefficient_words(prime)
    rng = make_rng(5)
    secrets_t = rows_t(eng, [1, 2, 3], limbs)
    good_draws = eng.torch.zeros((2, 3, cw), dtype=eng.torch.int32, device=eng.device)
    share = eng.shamir_share_t
    refused = [
        lambda: share(secrets_t, prime, 0, [1, 2, 3], rng=rng),                                   # degree < 1
        lambda: share(secrets_t, prime, 2, [1, 1, 2], rng=rng),                                   # points not distinct
        lambda: share(secrets_t, prime, 2, [0, 1, 2], rng=rng),                                   # a point below 1
        lambda: share(secrets_t, prime, 2, [1, 2, 1 << 16], rng=rng),                             # a point of 17 bits
        lambda: share(secrets_t, prime, 2, [1, 2.5, 3], rng=rng),                                 # not an integer
        lambda: share(secrets_t, prime, 2, [1, 2], rng=rng),                                      # fewer than degree + 1 points
        lambda: share(secrets_t, prime + 1, 2, [1, 2, 3], rng=rng),                               # an even prime
        lambda: share(secrets_t, prime, 2, [1, 2, 3]),                                            # neither rng nor rows
        lambda: share(secrets_t, prime, 2, [1, 2, 3], rng=rng, draws_t=good_draws),               # both
        lambda: share(secrets_t, prime, 2, [1, 2, 3], draws_t=good_draws[:, :, :-1]),             # rows too narrow
        lambda: share(secrets_t, prime, 2, [1, 2, 3], draws_t=good_draws[:1]),                    # one coefficient short
        lambda: share(secrets_t[0], prime, 2, [1, 2, 3], rng=rng),                                # secrets not [batch, limbs]
        lambda: share(secrets_t[:, :-1], prime, 2, [1, 2, 3], rng=rng),                           # secrets narrower than the prime
        lambda: share(None, prime, 2, [1, 2, 3], rng=rng),                                        # zero without batch=
        lambda: eng.shamir_share_batch([prime], prime, 2, [1, 2, 3], rng),                        # a secret outside [0, P)
        lambda: eng.shamir_share_batch([-1], prime, 2, [1, 2, 3], rng),
        lambda: eng.prime_candidates_t(3, 7, True, rng=rng),                                      # prime_length < 8
        lambda: eng.prime_candidates_t(3, 64, True),                                              # neither
        lambda: eng.prime_candidates_t(3, 64, True, rng=rng, random_t=good_draws[0, :, :2]),      # both
        lambda: eng.prime_candidates_t(3, 64, True, random_t=good_draws[0, :, :3]),               # random rows of another shape
        lambda: eng.prime_candidates_t(3, 64, True, rng=rng, row_words=1),                        # rows narrower than L bits
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
        assert rng.next_call == 5, k
