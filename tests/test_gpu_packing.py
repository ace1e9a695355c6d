"""Packing of Paillier ciphertexts on the GPU (csrc/mx_pack_n2.hpp, Engine.pack_nsquare_t / ciphertext_pack_batch,
packing.py), bit-exact against a host Horner over pow, and packed threshold decryption end to end."""

from __future__ import annotations

import ctypes
import random

import pytest

import standin_harness as sh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def odd_modulus(bits: int, rng: random.Random) -> int:
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def host_pack(cts, n, slot_bits, slots):
    """Horner over pow: acc = c_top, then acc^(2^b) * c_i for every lower slot (rows past the end are 1)."""
    n2 = n * n
    out = []
    for j in range(0, len(cts), slots):
        row = [c % n2 for c in cts[j : j + slots]]
        acc = 1
        for c in reversed(row + [1] * (slots - len(row))):
            acc = pow(acc, 1 << slot_bits, n2) * c % n2
        out.append(acc)
    return out


def inputs_for(n, count, rng):
    n2 = n * n
    special = [0, 1, n, n2 - 1, n2 + 5, 3 * n2 + n, -7, -(n2 - 2), 2 * n]
    vals = special + [rng.randrange(n2) for _ in range(max(0, count - len(special)))]
    rng.shuffle(vals)
    return vals[:count]


@pytest.mark.parametrize("key_length", [128, 1024, 2048, 4096, "odd"])
def test_pack_matches_a_host_horner(eng, key_length):
    from protocols.distributed_keygen_amd import packing, synthetic

    rng = random.Random(str(key_length))
    n = synthetic.make_key(key_length, 3, 1).n if key_length != "odd" else odd_modulus(1531, rng)
    bits = n.bit_length()
    for b in (1, 2, 31, 32, 64, 100, bits - 2):
        k = packing.slots_per_ciphertext(n, b)
        for count in sorted({1, max(k - 1, 1), k, k + 1, 3 * k + 5}):
            cts = inputs_for(n, count, rng)
            got = eng.ciphertext_pack_batch(cts, n, b, k)
            assert len(got) == -(-count // k)
            assert got == host_pack(cts, n, b, k), (bits, b, count)
    # fewer slots than the layout's maximum, and one slot (the canonical residue)
    cts = inputs_for(n, 20, rng)
    assert eng.ciphertext_pack_batch(cts, n, 8, 3) == host_pack(cts, n, 8, 3)
    assert eng.ciphertext_pack_batch(cts, n, 8, 1) == [c % (n * n) for c in cts]
    with pytest.raises(ValueError):
        eng.ciphertext_pack_batch(cts, n, bits - 2, 2)


def test_every_instance_has_a_parity_case(eng):
    from protocols.distributed_keygen_amd import limbs

    lib = eng.lib
    cnt = lib.mx_pack_nsquare_instances(None, None, 0)
    lanes, lpls = (ctypes.c_int * cnt)(), (ctypes.c_int * cnt)()
    assert lib.mx_pack_nsquare_instances(lanes, lpls, cnt) == cnt
    want = {(lanes[i], lpls[i]) for i in range(cnt)}
    rng = random.Random(17)
    seen = set()
    for bits in (130, 200, 400, 900, 2000, 3000, 4000, 6000, 8000):
        n = odd_modulus(bits, rng)
        k_, l_, w_ = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        ch = ctypes.c_int64()
        assert lib.mx_multiexp_nsquare_shape(bits, 4, 5, 4, 70, 0, 0, k_, l_, w_, ch) == 0
        seen.add((k_.value, l_.value))
        b = (bits - 2) // 3
        cts = inputs_for(n, 8, rng)
        x_t = eng.to_device(limbs.pack_reduced(cts, limbs.limbs_for(n * n), n * n))
        got = limbs.unpack(eng.to_host(eng.pack_nsquare_t(x_t, n, b, 3)))
        assert got == host_pack(cts, n, b, 3), bits
    assert seen == want


def test_abi_refuses_bad_arguments(eng):
    import torch

    from protocols.distributed_keygen_amd import limbs

    rng = random.Random(23)
    n = odd_modulus(1030, rng)
    n2 = n * n
    l2 = limbs.limbs_for(n2)
    x_t = eng.to_device(limbs.pack_reduced([rng.randrange(n2) for _ in range(8)], l2, n2))
    out_t = torch.zeros((8, l2), dtype=torch.int32, device=eng.device)
    plan = eng.nsquare_plan(n, 1)
    lib = eng.lib
    s = eng._stream_ptr()
    run = lambda *a: lib.mx_pack_nsquare_run(*a)            # noqa: E731
    x, o = x_t.data_ptr(), out_t.data_ptr()
    eng._use_plan(plan)
    assert n.bit_length() - 2 == 1028
    assert run(plan.desc, x, 8, l2, 343, 3, o, 0, s) == -1            # slot_bits * slots = 1029 > bits(N) - 2
    assert run(plan.desc, x, 8, l2, 1029, 1, o, 0, s) == -1
    assert run(plan.desc, x, 0, l2, 8, 3, o, 0, s) == -1
    assert run(plan.desc, x, 8, l2, 8, 0, o, 0, s) == -1
    assert run(plan.desc, x, 8, l2, 0, 3, o, 0, s) == -1
    assert run(plan.desc, None, 8, l2, 8, 3, o, 0, s) == -1
    assert run(plan.desc, x, 8, l2, 8, 3, None, 0, s) == -1
    assert run(None, x, 8, l2, 8, 3, o, 0, s) == -1
    assert run(plan.desc, x, 8, l2 - 1, 8, 3, o, 0, s) == -1          # rows too narrow for N^2
    assert run(plan.desc, x, 8, l2, 8, 3, o, 18, s) == -2             # outside the narrow geometry
    assert int(out_t.abs().sum()) == 0                                # nothing was launched
    assert run(plan.desc, x, 8, l2, 1028, 1, o, 0, s) == 0            # b = bits(N) - 2, one slot
    torch.cuda.synchronize()
    host = limbs.unpack(eng.to_host(x_t))
    assert limbs.unpack(eng.to_host(out_t)) == host


def encrypt_many(eng, key, values, rng):
    """(1 + m N) r^N mod N^2 for every m, r^N on the device."""
    n, n2 = key.n, key.n_square
    return eng.randomize_batch([(1 + (m % n) * n) % n2 for m in values], [rng.randrange(1, n) for _ in values], n)


def threshold_decrypt(eng, key, cts):
    n2 = key.n_square
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = cts if e >= 0 else eng.modinv_batch(cts, n2)
        partials.append(eng.powmod_nsquare_batch(bases, abs(e), key.n))
    out, ok = eng.combine_batch([[partials[i][k] for i in range(3)] for k in range(len(cts))], key.n, key.theta_inv)
    assert all(ok)
    return out


def test_packed_round_trip_at_key_length_2048(eng):
    from protocols.distributed_keygen_amd import packing, synthetic

    rng = random.Random(29)
    key = synthetic.make_key(2048, 3, 1)
    n = key.n
    assert any(key.exponent(i) < 0 for i in (1, 2, 3))
    # 100 000 signed 32-bit values
    vals = [rng.randrange(-(1 << 31), 1 << 31) for _ in range(100_000)]
    vals[:4] = [-(1 << 31), (1 << 31) - 1, 0, -1]
    cts = encrypt_many(eng, key, vals, rng)
    packed = packing.pack(cts, 32, n=n, engine=eng)
    assert len(packed) == -(-len(vals) // packing.slots_per_ciphertext(n, 32))
    assert packing.unpack(threshold_decrypt(eng, key, packed), 32, len(vals), n) == vals
    # unsigned 64-bit values with a ragged tail
    k = packing.slots_per_ciphertext(n, 64)
    vals = [rng.getrandbits(64) for _ in range(50 * k + 7)]
    vals[-1], vals[0] = (1 << 64) - 1, 0
    packed = packing.pack(encrypt_many(eng, key, vals, rng), 64, n=n, engine=eng)
    assert len(packed) == 51
    assert packing.unpack(threshold_decrypt(eng, key, packed), 64, len(vals), n, signed=False) == vals


def test_decrypt_sequence_packed_through_the_patched_standin(eng):
    import asyncio

    from protocols.distributed_keygen_amd import packing, patch, synthetic

    key = synthetic.make_key(1024, 3, 1)
    rng = random.Random(31)
    vals = [rng.randrange(-(1 << 31), 1 << 31) for _ in range(500)]
    cts = encrypt_many(eng, key, vals, rng)
    patch.install(engine=eng, package=sh.PACKAGE)
    try:
        parties = sh.parties_for_key(key)
        cobjs = sh.ciphertexts(key, cts)
        sizes = []
        for dp in parties:
            orig = dp._decrypt_sequence_raw

            async def recording(seq, receivers=None, _orig=orig):
                seq = list(seq)
                sizes.append(len(seq))
                return await _orig(seq, receivers)

            dp._decrypt_sequence_raw = recording

        async def run():
            return await asyncio.gather(*[packing.decrypt_sequence_packed(dp, cobjs, 32, engine=eng) for dp in parties])

        assert asyncio.run(run()) == [vals] * 3
        assert sizes == [-(-500 // packing.slots_per_ciphertext(key.n, 32))] * 3
    finally:
        patch.uninstall()


def test_pack_on_one_stream_beside_a_partial_decryption_on_another(eng):
    import torch

    from protocols.distributed_keygen_amd import limbs

    rng = random.Random(37)
    n = odd_modulus(2048, rng)
    n2 = n * n
    l2 = limbs.limbs_for(n2)
    cts = [rng.randrange(n2) for _ in range(2000)]
    exp = rng.getrandbits(2100)
    x_t = eng.to_device(limbs.pack_reduced(cts, l2, n2))
    want_pack = host_pack(cts, n, 32, 63)
    want_pow = [pow(c, exp, n2) for c in cts[:64]]
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        p_t = eng.pack_nsquare_t(x_t, n, 32, 63)
    d_t = eng.powmod_nsquare_t(x_t, n, exp)
    cur.wait_stream(side)
    assert limbs.unpack(eng.to_host(p_t)) == want_pack
    assert limbs.unpack(eng.to_host(d_t))[:64] == want_pow
