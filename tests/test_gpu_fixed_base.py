"""Fixed-base encryption and re-randomisation on the GPU (csrc/mx_fixedbase_n2.hpp, Engine.fixed_base_*,
randomizer.py), bit-exact against CPython pow (tests/hostpow.py for the full-size batch)."""

from __future__ import annotations

import ctypes
import random

import pytest

import hostpow
import standin_harness as sh

pytestmark = pytest.mark.gpu

POWER, ENCRYPT, RANDOMIZE = 0, 1, 2


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def odd_modulus(bits: int, rng: random.Random) -> int:
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def modulus_for(key_length):
    from protocols.distributed_keygen_amd import synthetic

    if key_length == "odd":
        return odd_modulus(1531, random.Random("odd 1531"))      # no biprime: the kernels never ask
    return synthetic.make_key(key_length, 3, 1).n


def base_for(n, rng):
    y = rng.randrange(2, n)
    return pow((-y * y) % n, n, n * n)


_chains = {}


def chain_of(base, n2, exp_bits):
    """[base^(2^k) mod n2 for k < exp_bits], by pow, kept per (base, modulus)."""
    c = _chains.setdefault((base, n2), [base % n2])
    while len(c) < exp_bits:
        c.append(pow(c[-1], 2, n2))
    return c


def exponents_for(exp_bits, window, rng):
    """0, 1, the largest, one bit in every window in turn (its lowest and its highest), random ones."""
    top = (1 << exp_bits) - 1
    w = window or 1
    exps = [0, 1 & top, top]
    single = []
    for lo in range(0, exp_bits, w):
        single.append(lo)
        hi = min(lo + w, exp_bits) - 1
        if hi != lo and (lo // w) % 7 == 0:
            single.append(hi)
    exps += [1 << k for k in single]
    exps += [rng.getrandbits(exp_bits) for _ in range(5)]
    return exps, 3, len(single)


def expected_powers(base, n2, exp_bits, exps, first_single, n_single):
    chain = chain_of(base, n2, exp_bits)
    out = []
    for i, e in enumerate(exps):
        if first_single <= i < first_single + n_single:
            out.append(chain[e.bit_length() - 1])
        else:
            out.append(pow(base, e, n2))
    return out


def run_modes(eng, table, n, exps, powers, rng, garbage=False):
    """All three modes for the same exponents against `powers`; `garbage`: words and bits above exp_bits are set."""
    import numpy as np

    from protocols.distributed_keygen_amd import limbs

    n2 = n * n
    ln, l2 = limbs.limbs_for(n), limbs.limbs_for(n2)
    count = len(exps)
    ewords = (table.exp_bits + 31) // 32
    rows = limbs.pack(exps, ewords)
    if garbage:
        rows = rows.copy()
        spare = 32 * ewords - table.exp_bits
        if spare:
            rows[:, -1] |= np.uint32(((1 << spare) - 1) << (32 - spare))
    e_t = eng.to_device(rows)
    msgs = ([0, 1, n - 1] + [rng.randrange(n) for _ in range(count)])[:count]
    cts = ([0, 1, n, 2 * n, n2 - 1] + [rng.randrange(n2) for _ in range(count)])[:count]
    rng.shuffle(msgs)
    rng.shuffle(cts)
    got = limbs.unpack(eng.to_host(eng.fixed_base_power_t(table, e_t)))
    assert got == powers, ("power", n.bit_length(), table.exp_bits, table.window)
    got = limbs.unpack(eng.to_host(eng.fixed_base_encrypt_t(table, e_t, eng.to_device(limbs.pack(msgs, ln)))))
    assert got == [(1 + m * n) * h % n2 for m, h in zip(msgs, powers)], ("encrypt", n.bit_length(), table.exp_bits, table.window)
    got = limbs.unpack(eng.to_host(eng.fixed_base_randomize_t(table, e_t, eng.to_device(limbs.pack(cts, l2)))))
    assert got == [c * h % n2 for c, h in zip(cts, powers)], ("randomize", n.bit_length(), table.exp_bits, table.window)


@pytest.mark.parametrize("window", [0, 1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("key_length", [128, 1024, 2048, 4096, "odd"])
def test_three_modes_match_pow(eng, key_length, window):
    n = modulus_for(key_length)
    n2, bits = n * n, n.bit_length()
    rng = random.Random(f"{key_length} {window}")
    base = base_for(n, random.Random(str(key_length)))
    w = window or 4
    for exp_bits in sorted({1, 2, max(w - 1, 1), w, w + 1, 63, 64, 65, -(-bits // 2), bits, bits + 64}):
        table = eng.fixed_base_table(n, base, exp_bits, window)
        assert table.exp_bits == exp_bits and 1 <= table.window <= 8 and (window == 0 or table.window == window)
        assert table.windows == -(-exp_bits // table.window)
        exps, first, n_single = exponents_for(exp_bits, table.window, rng)
        powers = expected_powers(base, n2, exp_bits, exps, first, n_single)
        run_modes(eng, table, n, exps, powers, rng, garbage=exp_bits % 32 != 0 and window in (0, 3, 8))


@pytest.mark.parametrize("key_length", [128, 1024, 2048, 4096, "odd"])
def test_degenerate_bases(eng, key_length):
    n = modulus_for(key_length)
    n2, bits = n * n, n.bit_length()
    rng = random.Random(f"bases {key_length}")
    for base in (0, 1, n, n2 - 1):
        for window, exp_bits in ((3, 1), (3, 65), (0, -(-bits // 2)), (8, 70)):
            table = eng.fixed_base_table(n, base, exp_bits, window)
            exps = [0, 1, (1 << exp_bits) - 1, 2 & ((1 << exp_bits) - 1)] + [rng.getrandbits(exp_bits) for _ in range(4)]
            run_modes(eng, table, n, exps, [pow(base, e, n2) for e in exps], rng)
    # the int-level forms reduce their arguments: a base and ciphertexts above N^2, negative messages
    base = base_for(n, rng)
    exps = [rng.getrandbits(40) for _ in range(6)]
    pw = [pow(base, e, n2) for e in exps]
    assert eng.fixed_base_power_batch(exps, n, base + 3 * n2, 40) == pw
    msgs = [0, -5, n - 1, 424242, -n, 2 * n + 1]
    assert eng.fixed_base_encrypt_batch(msgs, exps, n, base, 40) == [(1 + (m % n) * n) * h % n2 for m, h in zip(msgs, pw)]
    cts = [0, n2 + 5, -7, n, 2 * n, n2 - 1]
    assert eng.fixed_base_randomize_batch(cts, exps, n, base, 40, window=5) == [c % n2 * h % n2 for c, h in zip(cts, pw)]
    with pytest.raises(ValueError):
        eng.fixed_base_power_batch([1 << 40], n, base, 40)
    with pytest.raises(ValueError):
        eng.fixed_base_power_batch([-1], n, base, 40)
    assert eng.fixed_base_power_batch([], n, base, 40) == []


def shape_of(lib, bits, exp_bits, count, window=0, budget=0):
    k, l, w, nw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib.mx_fixedbase_nsquare_shape(bits, exp_bits, count, budget, 0, window, k, l, w, nw)
    return rc, k.value, l.value, w.value, nw.value


@pytest.mark.parametrize("key_length", [128, 1024, 2048, 4096, "odd"])
def test_counts_around_a_wavefront(eng, key_length):
    n = modulus_for(key_length)
    n2, bits = n * n, n.bit_length()
    rng = random.Random(f"counts {key_length}")
    base = base_for(n, rng)
    exp_bits = 48
    rc, lanes, _, _, _ = shape_of(eng.lib, bits, exp_bits, 1)
    assert rc == 0
    gpw = 64 // lanes
    table = eng.fixed_base_table(n, base, exp_bits, 6)
    for count in sorted({1, max(gpw - 1, 1), gpw, gpw + 1, 3 * gpw + 1}):
        exps = [rng.getrandbits(exp_bits) for _ in range(count)]
        run_modes(eng, table, n, exps, [pow(base, e, n2) for e in exps], rng)


def test_ten_thousand_at_key_length_2048(eng):
    from protocols.distributed_keygen_amd import limbs

    n = modulus_for(2048)
    n2 = n * n
    rng = random.Random(41)
    base = base_for(n, rng)
    exp_bits = -(-n.bit_length() // 2)
    count = 10_000
    exps = [rng.getrandbits(exp_bits) for _ in range(count)]
    exps[:3] = [0, 1, (1 << exp_bits) - 1]
    powers = hostpow.powmod_many([(base, e, n2) for e in exps])
    table = eng.fixed_base_table(n, base, exp_bits)
    run_modes(eng, table, n, exps, powers, rng)
    cts = [rng.randrange(n2) for _ in range(count)]
    assert eng.fixed_base_randomize_batch(cts, exps, n, base, exp_bits) == [c * h % n2 for c, h in zip(cts, powers)]
    assert limbs.unpack(eng.to_host(eng.fixed_base_power_t(table, eng.fixed_base_exponent_rows(exps, exp_bits)))) == powers


def test_every_instance_has_a_parity_case(eng):
    lib = eng.lib
    cnt = lib.mx_fixedbase_nsquare_instances(None, None, 0)
    lanes, lpls = (ctypes.c_int * cnt)(), (ctypes.c_int * cnt)()
    assert lib.mx_fixedbase_nsquare_instances(lanes, lpls, cnt) == cnt
    want = {(lanes[i], lpls[i]) for i in range(cnt)}
    rng = random.Random(17)
    seen = set()
    for bits in (130, 200, 400, 900, 2000, 3000, 4000, 6000, 8000):
        n = odd_modulus(bits, rng)
        exp_bits = 77
        rc, k, l, w, nw = shape_of(lib, bits, exp_bits, 9)
        assert rc == 0 and nw == -(-exp_bits // w)
        seen.add((k, l))
        base = rng.randrange(n * n)
        exps = [0, 1, (1 << exp_bits) - 1] + [rng.getrandbits(exp_bits) for _ in range(6)]
        powers = [pow(base, e, n * n) for e in exps]
        for window in (0, 5):
            run_modes(eng, eng.fixed_base_table(n, base, exp_bits, window), n, exps, powers, rng, garbage=True)
    assert seen == want


def test_window_model_respects_the_budget_and_an_explicit_window(eng):
    lib = eng.lib
    bits = 2051
    rc, k, l, w_many, _ = shape_of(lib, bits, 1026, 1_000_000)
    rc2, _, _, w_one, _ = shape_of(lib, bits, 1026, 1)
    assert rc == 0 and rc2 == 0 and 1 <= w_one <= w_many <= 8
    for w in range(1, 9):
        assert shape_of(lib, bits, 1026, 1000, window=w)[3] == w
        need = lib.mx_fixedbase_nsquare_table_bytes(bits, 1026, 0, w)
        assert need >= -(-1026 // w) * (2 * k * l * 4 << w)
    tight = lib.mx_fixedbase_nsquare_table_bytes(bits, 1026, 0, 4)
    assert shape_of(lib, bits, 1026, 1_000_000, budget=tight)[3] <= 4
    assert shape_of(lib, bits, 1026, 0)[0] == -1 and shape_of(lib, bits, 0, 10)[0] == -1
    assert shape_of(lib, bits, 2 * bits + 65, 10)[0] == -1 and shape_of(lib, bits, 10, 10, window=9)[0] == -1
    assert shape_of(lib, 40000, 10, 10)[0] == -2
    assert lib.mx_fixedbase_nsquare_table_bytes(bits, 1026, 0, 0) == -1
    assert lib.mx_fixedbase_nsquare_table_bytes(bits, 1026, 18, 4) == -2


def test_abi_refuses_bad_arguments(eng):
    import torch

    from protocols.distributed_keygen_amd import limbs

    rng = random.Random(23)
    n = odd_modulus(1030, rng)
    n2 = n * n
    ln, l2 = limbs.limbs_for(n), limbs.limbs_for(n2)
    lib = eng.lib
    s = eng._stream_ptr()
    plan = eng.nsquare_plan(n, 1)
    eng._use_plan(plan)
    exp_bits, w = 100, 4
    base = rng.randrange(n2)
    b_t = eng.to_device(limbs.pack([base], l2))
    need = lib.mx_fixedbase_nsquare_table_bytes(n.bit_length(), exp_bits, 0, w)
    assert need > 0
    tab_t = torch.zeros(need, dtype=torch.uint8, device=eng.device)
    prep = lambda *a: lib.mx_fixedbase_nsquare_prepare(*a)            # noqa: E731
    b, t = b_t.data_ptr(), tab_t.data_ptr()
    assert prep(None, b, l2, exp_bits, 0, w, t, need, s) == -1
    assert prep(plan.desc, None, l2, exp_bits, 0, w, t, need, s) == -1
    assert prep(plan.desc, b, l2, exp_bits, 0, w, None, need, s) == -1
    assert prep(plan.desc, b, l2, 0, 0, w, t, need, s) == -1
    assert prep(plan.desc, b, l2, 2 * n.bit_length() + 65, 0, w, t, 1 << 40, s) == -1
    assert prep(plan.desc, b, l2, exp_bits, 0, 0, t, need, s) == -1
    assert prep(plan.desc, b, l2, exp_bits, 0, 9, t, need, s) == -1
    assert prep(plan.desc, b, l2, exp_bits, 0, w, t, need - 1, s) == -1       # table buffer too small
    assert prep(plan.desc, b, l2, exp_bits, 0, w + 1, t, need, s) == -1       # ... for this window
    assert prep(plan.desc, b, l2 - 1, exp_bits, 0, w, t, need, s) == -1       # rows too narrow for N^2
    assert prep(plan.desc, b, l2, exp_bits, 18, w, t, need, s) == -2          # outside the narrow geometry
    torch.cuda.synchronize()
    assert int(tab_t.sum()) == 0                                              # nothing was launched
    assert prep(plan.desc, b, l2, exp_bits, 0, w, t, need, s) == 0

    count = 8
    exps = [rng.getrandbits(exp_bits) for _ in range(count)]
    e_t = eng.to_device(limbs.pack(exps, 4))
    msgs = [rng.randrange(n) for _ in range(count)]
    cts = [rng.randrange(n2) for _ in range(count)]
    m_t, c_t = eng.to_device(limbs.pack(msgs, ln)), eng.to_device(limbs.pack(cts, l2))
    out_t = torch.zeros((count, l2), dtype=torch.int32, device=eng.device)
    run = lambda *a: lib.mx_fixedbase_nsquare_run(*a)                 # noqa: E731
    e, m, c, o = e_t.data_ptr(), m_t.data_ptr(), c_t.data_ptr(), out_t.data_ptr()
    assert run(None, t, exp_bits, w, POWER, e, None, 0, o, count, l2, 0, s) == -1
    assert run(plan.desc, None, exp_bits, w, POWER, e, None, 0, o, count, l2, 0, s) == -1
    assert run(plan.desc, t, exp_bits, w, POWER, None, None, 0, o, count, l2, 0, s) == -1
    assert run(plan.desc, t, exp_bits, w, POWER, e, None, 0, None, count, l2, 0, s) == -1
    assert run(plan.desc, t, exp_bits, w, POWER, e, None, 0, o, 0, l2, 0, s) == -1
    assert run(plan.desc, t, 0, w, POWER, e, None, 0, o, count, l2, 0, s) == -1
    assert run(plan.desc, t, 2 * n.bit_length() + 65, w, POWER, e, None, 0, o, count, l2, 0, s) == -1
    assert run(plan.desc, t, exp_bits, 0, POWER, e, None, 0, o, count, l2, 0, s) == -1
    assert run(plan.desc, t, exp_bits, 9, POWER, e, None, 0, o, count, l2, 0, s) == -1
    assert run(plan.desc, t, exp_bits, w, 3, e, None, 0, o, count, l2, 0, s) == -1            # no such mode
    assert run(plan.desc, t, exp_bits, w, ENCRYPT, e, None, ln, o, count, l2, 0, s) == -1     # operand missing
    assert run(plan.desc, t, exp_bits, w, RANDOMIZE, e, None, l2, o, count, l2, 0, s) == -1
    assert run(plan.desc, t, exp_bits, w, ENCRYPT, e, m, ln - 1, o, count, l2, 0, s) == -1    # rows too narrow for N
    assert run(plan.desc, t, exp_bits, w, RANDOMIZE, e, c, l2 - 1, o, count, l2, 0, s) == -1  # ... for N^2
    assert run(plan.desc, t, exp_bits, w, POWER, e, None, 0, o, count, l2 - 1, 0, s) == -1
    assert run(plan.desc, t, exp_bits, w, POWER, e, None, 0, o, count, l2, 18, s) == -2       # outside the narrow geometry
    torch.cuda.synchronize()
    assert int(out_t.abs().sum()) == 0                                        # nothing was launched
    powers = [pow(base, x, n2) for x in exps]
    assert run(plan.desc, t, exp_bits, w, POWER, e, None, 0, o, count, l2, 0, s) == 0
    assert limbs.unpack(eng.to_host(out_t)) == powers
    assert run(plan.desc, t, exp_bits, w, ENCRYPT, e, m, ln, o, count, l2, 0, s) == 0
    assert limbs.unpack(eng.to_host(out_t)) == [(1 + x * n) * h % n2 for x, h in zip(msgs, powers)]
    assert run(plan.desc, t, exp_bits, w, RANDOMIZE, e, c, l2, o, count, l2, 0, s) == 0
    assert limbs.unpack(eng.to_host(out_t)) == [x * h % n2 for x, h in zip(cts, powers)]


def test_one_table_on_two_streams_beside_a_partial_decryption(eng):
    import torch

    from protocols.distributed_keygen_amd import limbs

    rng = random.Random(37)
    n = odd_modulus(2048, rng)
    n2 = n * n
    ln, l2 = limbs.limbs_for(n), limbs.limbs_for(n2)
    exp_bits = 1024
    base = rng.randrange(n2)
    count = 3000
    exps_a = [rng.getrandbits(exp_bits) for _ in range(count)]
    exps_b = [rng.getrandbits(exp_bits) for _ in range(count)]
    msgs = [rng.randrange(n) for _ in range(count)]
    cts = [rng.randrange(n2) for _ in range(count)]
    share = rng.getrandbits(2100)
    pw = hostpow.powmod_many([(base, e, n2) for e in exps_a + exps_b] + [(c, share, n2) for c in cts[:64]])
    table = eng.fixed_base_table(n, base, exp_bits)
    ea_t, eb_t = eng.fixed_base_exponent_rows(exps_a, exp_bits), eng.fixed_base_exponent_rows(exps_b, exp_bits)
    m_t, c_t = eng.to_device(limbs.pack(msgs, ln)), eng.to_device(limbs.pack(cts, l2))
    cur = torch.cuda.current_stream()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(cur)
    s2.wait_stream(cur)
    with torch.cuda.stream(s1):
        a_t = eng.fixed_base_encrypt_t(table, ea_t, m_t)
    with torch.cuda.stream(s2):
        b_t = eng.fixed_base_randomize_t(table, eb_t, c_t)
    d_t = eng.powmod_nsquare_t(c_t, n, share)
    cur.wait_stream(s1)
    cur.wait_stream(s2)
    assert limbs.unpack(eng.to_host(a_t)) == [(1 + m * n) * h % n2 for m, h in zip(msgs, pw[:count])]
    assert limbs.unpack(eng.to_host(b_t)) == [c * h % n2 for c, h in zip(cts, pw[count : 2 * count])]
    assert limbs.unpack(eng.to_host(d_t))[:64] == pw[2 * count :]


def test_a_table_evicted_while_launches_that_read_it_are_pending(eng):
    import torch

    from protocols.distributed_keygen_amd import Engine, limbs

    rng = random.Random(43)
    n = odd_modulus(2048, rng)
    n2 = n * n
    l2 = limbs.limbs_for(n2)
    exp_bits = 1024
    base = rng.randrange(n2)
    count = 4000
    exps = [rng.getrandbits(exp_bits) for _ in range(count)]
    want = hostpow.powmod_many([(base, e, n2) for e in exps])
    small = odd_modulus(130, rng)
    key = (n, base, exp_bits, 7)
    table = eng.fixed_base_table(*key)
    nbytes = table.nbytes
    e_t = eng.fixed_base_exponent_rows(exps, exp_bits)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        outs = [eng.fixed_base_power_t(table, e_t) for _ in range(4)]      # pending on the side stream
    del table
    for k in range(Engine.MAX_PLANS + 1):                                  # ... while more tables than the cache keeps arrive
        eng.fixed_base_table(small, 3 + k, 16, 2)
    assert key not in eng._fixed_base_tables
    # the evicted block is free for reuse on this stream: whoever gets it next overwrites it — but not before the
    # launches of the side stream that read it have finished (Engine._cache_plan)
    junk = [torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=eng.device) for _ in range(2)]
    cur.wait_stream(side)
    for o_t in outs:
        assert limbs.unpack(eng.to_host(o_t)) == want
    del junk
    assert limbs.unpack(eng.to_host(eng.fixed_base_power_t(eng.fixed_base_table(*key), e_t))) == want    # rebuilt


# ---- round trips (the helpers' logic of tests/test_gpu_packing.py) ---------------------------------------------------
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


def test_fast_encrypt_pack_decrypt_round_trip_at_key_length_2048(eng):
    from protocols.distributed_keygen_amd import packing, randomizer, synthetic

    rng = random.Random(29)
    key = synthetic.make_key(2048, 3, 1)
    n = key.n
    assert key.p % 4 == 3 and key.q % 4 == 3
    h_s = randomizer.generate_base(n, rng=rng, engine=eng)
    y_check = pow(h_s, (key.p - 1) * (key.q - 1), n * n)
    assert y_check == 1                                             # an N-th power: decryption does not see it
    fr = randomizer.FastRandomizer(n, h_s, engine=eng)
    assert fr.exp_bits == -(-n.bit_length() // 2)
    vals = [rng.randrange(-(1 << 31), 1 << 31) for _ in range(100_000)]
    vals[:4] = [-(1 << 31), (1 << 31) - 1, 0, -1]
    cts = fr.encrypt(vals)
    assert len(set(cts[:1000])) == 1000
    packed = packing.pack(cts, 32, n=n, engine=eng, randomizer=fr)
    assert len(packed) == -(-len(vals) // packing.slots_per_ciphertext(n, 32))
    assert packed != packing.pack(cts, 32, n=n, engine=eng)
    assert packing.unpack(threshold_decrypt(eng, key, packed), 32, len(vals), n) == vals
    # deterministic with given exponents, and equal to the definition
    exps = [rng.getrandbits(fr.exp_bits) for _ in range(5)]
    assert fr.encrypt(vals[:5], exponents=exps) == [(1 + (m % n) * n) * pow(h_s, a, n * n) % (n * n) for m, a in zip(vals, exps)]
    assert fr.randomizers(5, exponents=exps) == [pow(h_s, a, n * n) for a in exps]


def test_linear_map_with_a_randomizer_through_the_patched_standin(eng):
    from protocols.distributed_keygen_amd import homomorphic, patch, randomizer, synthetic

    key = synthetic.make_key(1024, 3, 1)
    n, n2 = key.n, key.n_square
    rng = random.Random(31)
    h_s = randomizer.generate_base(n, rng=rng, engine=eng)
    fr = randomizer.FastRandomizer(n, h_s, engine=eng)
    x = [rng.randrange(-1000, 1000) for _ in range(12)]
    W = [[rng.randrange(-50, 50) for _ in x] for _ in range(7)]
    b = [rng.randrange(-10**6, 10**6) for _ in W]
    want = [(sum(w * v for w, v in zip(row, x)) + bj) % n for row, bj in zip(W, b)]
    cts = fr.encrypt(x)
    plain = homomorphic.linear_map(cts, W, n=n, bias=b, engine=eng)
    ea = [rng.getrandbits(fr.exp_bits) for _ in W]
    eb = [rng.getrandbits(fr.exp_bits) for _ in W]
    ya = homomorphic.linear_map(cts, W, n=n, bias=b, engine=eng, randomizer=_Given(fr, ea))
    yb = homomorphic.linear_map(cts, W, n=n, bias=b, engine=eng, randomizer=_Given(fr, eb))
    assert ya == [c * pow(h_s, a, n2) % n2 for c, a in zip(plain, ea)]
    assert yb == [c * pow(h_s, a, n2) % n2 for c, a in zip(plain, eb)]
    assert all(u != v for u, v in zip(ya, yb))
    yc = homomorphic.linear_map(cts, W, n=n, bias=b, engine=eng, randomizer=fr)          # drawn exponents
    assert all(u != v for u, v in zip(yc, plain))
    patch.install(engine=eng, package=sh.PACKAGE)
    try:
        parties = sh.parties_for_key(key)
        for y in (ya, yb, yc):
            res = sh.decrypt_sequence(parties, sh.ciphertexts(key, y))
            for party in res:
                assert [r.value % n for r in party] == want
    finally:
        patch.uninstall()
    # the other operations keep their rows on the device the same way
    sc = homomorphic.scale(cts[:3], [2, -3, 5], n=n, engine=eng)
    assert homomorphic.scale(cts[:3], [2, -3, 5], n=n, engine=eng, randomizer=_Given(fr, ea[:3])) == [
        c * pow(h_s, a, n2) % n2 for c, a in zip(sc, ea)]
    ad = homomorphic.add(cts[:3], cts[3:6], n=n, engine=eng)
    assert homomorphic.add(cts[:3], cts[3:6], n=n, engine=eng, randomizer=_Given(fr, ea[:3])) == [
        c * pow(h_s, a, n2) % n2 for c, a in zip(ad, ea)]
    ng = homomorphic.neg(cts[:3], n=n, engine=eng)
    assert homomorphic.neg(cts[:3], n=n, engine=eng, randomizer=_Given(fr, ea[:3])) == [
        c * pow(h_s, a, n2) % n2 for c, a in zip(ng, ea)]
    sg = homomorphic.sum_groups([cts[:5], [], cts[5:]], n=n, engine=eng)
    assert homomorphic.sum_groups([cts[:5], [], cts[5:]], n=n, engine=eng, randomizer=_Given(fr, ea[:3])) == [
        c * pow(h_s, a, n2) % n2 for c, a in zip(sg, ea)]


class _Given:
    """A FastRandomizer whose next draw is a given list of exponents."""

    def __init__(self, fr, exps):
        self.fr, self.exps = fr, list(exps)

    def spec(self, n, count):
        return self.fr.spec(n, count, exponents=self.exps)
