"""Homomorphic linear maps of Paillier ciphertexts on the GPU (csrc/mx_multiexp_n2.hpp, Engine.multiexp_nsquare_t,
homomorphic.py), bit-exact against pow and products."""

from __future__ import annotations

import ctypes
import random

import pytest

import hostpow

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def odd_modulus(bits: int, rng: random.Random) -> int:
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def key_n(key_length: int) -> int:
    from protocols.distributed_keygen_amd import synthetic

    return synthetic.make_key(key_length, 3, 1).n


def prod_mod(vals, m):
    acc = 1
    for v in vals:
        acc = acc * v % m
    return acc


@pytest.mark.parametrize("key_length", [128, 1024, 2048, 4096, "odd"])
def test_scale_matches_pow(eng, key_length):
    rng = random.Random(str(key_length))
    n = key_n(key_length) if key_length != "odd" else odd_modulus(1531, rng)
    n2 = n * n
    scalars = [0, 1, -1, (1 << 64) - 1, -(1 << 64), rng.randrange(n2), -rng.randrange(n2), n, n2, rng.getrandbits(64) - (1 << 63)]
    units = [1, n2 - 1, n2 + rng.randrange(1, n2), -rng.randrange(1, n2), rng.randrange(n2) | 1]
    if key_length == "odd":                 # a random odd N: keep the invertible inputs invertible
        import math

        units = [u for u in units if math.gcd(u % n2, n) == 1]
    cts = [u for u in units for _ in scalars] + [0, n, 0, n]
    ks = [k for _ in units for k in scalars] + [0, 0, 5, 2]
    got = eng.ciphertext_scale_batch(cts, ks, n)
    want = hostpow.powmod_many([(c % n2 if k >= 0 else pow(c, -1, n2), abs(k), n2) for c, k in zip(cts, ks)])
    assert got == want
    with pytest.raises(ValueError):
        eng.ciphertext_scale_batch([3, 0], [1, -1], n)
    with pytest.raises(ValueError):
        eng.ciphertext_scale_batch([n], [-2], n)


def test_sums_over_ragged_groups_and_split_k(eng):
    from protocols.distributed_keygen_amd import synthetic

    rng = random.Random(7)
    key = synthetic.make_key(2048, 3, 1)
    n, n2 = key.n, key.n_square
    big = synthetic.random_ciphertexts(key, 100_000, seed=3)
    groups = [[], [rng.randrange(n2)], [rng.randrange(n2), -5], [rng.randrange(n2) for _ in range(1000)], big]
    w, chunk, _ = eng.multiexp_nsquare_shape(n, 100_000, 1, 100_000, 1)
    assert chunk < 100_000, "one sum of 100 000 must run split-K"
    assert eng.ciphertext_sum_batch(groups, n) == [prod_mod([v % n2 for v in g], n2) for g in groups]


def test_dense_sparse_empty_and_zero_rows(eng):
    rng = random.Random(11)
    n = key_n(2048)
    n2 = n * n
    cts = [rng.randrange(n2) for _ in range(64)]
    W = [[rng.randrange(-(1 << 63), 1 << 63) for _ in range(64)] for _ in range(64)]
    bias = [rng.randrange(-n, 2 * n) for _ in range(64)]
    invs = {i: pow(c, -1, n2) for i, c in enumerate(cts)}
    terms = hostpow.powmod_many([(cts[i] if w >= 0 else invs[i], abs(w), n2) for row in W for i, w in enumerate(row)])
    want = [(1 + (bias[j] % n) * n) * prod_mod(terms[64 * j : 64 * j + 64], n2) % n2 for j in range(64)]
    assert eng.ciphertext_linear_map_batch(cts, W, n, bias=bias) == want
    sparse = [{}, {3: 0, 7: 0}, {5: -1}, {0: 1, 63: 2, 17: -(1 << 100)}, {i: 1 for i in range(0, 64, 3)}]
    want_s = []
    for row in sparse:
        acc = 1
        for i, w in row.items():
            acc = acc * pow(cts[i], w, n2) % n2
        want_s.append(acc)
    assert eng.ciphertext_linear_map_batch(cts, sparse, n) == want_s
    assert eng.ciphertext_linear_map_batch(cts, [[0] * 64, {}], n, bias=[5, n]) == [1 + 5 * n, 1]


def test_encrypted_linear_map_round_trip(eng):
    from protocols.distributed_keygen_amd import homomorphic, synthetic

    rng = random.Random(13)
    key = synthetic.make_key(1024, 3, 1)
    n, n2 = key.n, key.n_square
    m = [rng.randrange(n) for _ in range(16)]
    cts = [synthetic.encrypt(key, v, rng) for v in m]
    W = [[rng.randrange(-(1 << 63), 1 << 63) for _ in range(16)] for _ in range(8)]
    b = [rng.randrange(n) for _ in range(8)]
    y = homomorphic.linear_map(cts, W, n=n, bias=b, engine=eng)
    y = eng.randomize_batch(y, [rng.randrange(1, n) for _ in y], n)
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = y if e >= 0 else eng.modinv_batch(y, n2)
        partials.append(eng.powmod_nsquare_batch(bases, abs(e), n))
    out, ok = eng.combine_batch([[partials[i][k] for i in range(3)] for k in range(len(y))], n, key.theta_inv)
    assert all(ok)
    assert out == [(sum(w * v for w, v in zip(row, m)) + bj) % n for row, bj in zip(W, b)]


def test_every_instance_has_a_parity_case(eng):
    from protocols.distributed_keygen_amd import limbs

    lib = eng.lib
    cnt = lib.mx_multiexp_nsquare_instances(None, None, 0)
    lanes, lpls = (ctypes.c_int * cnt)(), (ctypes.c_int * cnt)()
    assert lib.mx_multiexp_nsquare_instances(lanes, lpls, cnt) == cnt
    want = {(lanes[i], lpls[i]) for i in range(cnt)}
    rng = random.Random(17)
    seen = set()
    for bits in (130, 200, 400, 900, 2000, 3000, 4000, 6000, 8000):
        n = odd_modulus(bits, rng)
        n2 = n * n
        k, l, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        ch = ctypes.c_int64()
        assert lib.mx_multiexp_nsquare_shape(bits, 4, 5, 4, 70, 0, 0, k, l, w, ch) == 0
        seen.add((k.value, l.value))
        cts = [rng.randrange(n2) for _ in range(4)] + [n2 + 3]
        W = [[rng.getrandbits(70) for _ in range(5)] for _ in range(5)]
        W[1] = [0, 1, 2, 3, 0]
        want_y = [prod_mod([pow(c, x, n2) for c, x in zip(cts, row)], n2) for row in W]
        x_t = eng.to_device(limbs.pack_reduced(cts, limbs.limbs_for(n2), n2))
        for window in (0, 1, 8):
            got = limbs.unpack(eng.to_host(eng.multiexp_nsquare_t(x_t, W, n, window=window)))
            assert got == want_y, (bits, window)
    assert seen == want


def test_two_streams_beside_a_partial_decryption(eng):
    import torch

    from protocols.distributed_keygen_amd import limbs

    rng = random.Random(19)
    n = key_n(2048)
    n2 = n * n
    l2 = limbs.limbs_for(n2)
    cts = [rng.randrange(n2) for _ in range(128)]
    maps = [[{i: rng.getrandbits(64) for i in rng.sample(range(128), 32)} for _ in range(96)] for _ in range(2)]
    exp = rng.getrandbits(2100)
    x_t = eng.to_device(limbs.pack_reduced(cts, l2, n2))
    want_maps = [[prod_mod([pow(cts[i], w, n2) for i, w in row.items()], n2) for row in m] for m in maps]
    want_pow = hostpow.powmod_many([(c, exp, n2) for c in cts])
    cur = torch.cuda.current_stream()
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for s, m in zip(sides, maps):
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            outs.append(eng.multiexp_nsquare_t(x_t, m, n))
    p_t = eng.powmod_nsquare_t(x_t, n, exp)
    for s in sides:
        cur.wait_stream(s)
    assert limbs.unpack(eng.to_host(p_t)) == want_pow
    for o, wm in zip(outs, want_maps):
        assert limbs.unpack(eng.to_host(o)) == wm
