"""The jointly random generators of the biprimality test on the GPU (csrc/mx_generators.hpp, Engine.generator_shares_t /
generator_sum_t, biprime.BiprimeRound.draw_generator_shares / sum_generators): bit for bit against
tools/generators_model.py — Python ``%`` on ints — for host-supplied and device-drawn rows, in every lane geometry.

Moduli: the candidate moduli of tests/golden/biprime.json (key_length 64 and 128: one lane per row, 1024: four, 2048:
eight) and, for the other groups, the odd stand-ins of tests/test_gpu_shamir_share.py: 262 bits (two lanes), 4103 bits
(sixteen), 8204 bits (thirty-two) and 8401 bits (sixty-four).  A class of moduli is widened to the count a shape needs with
further odd numbers of the same length (the comparison is with ``%``: any odd modulus serves)."""

from __future__ import annotations

import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import generators_model as gm  # noqa: E402

from conftest import unhex  # noqa: E402
from generators_engine import split_shares  # noqa: E402
from oracle import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes((11 * k + 5) & 0xFF for k in range(32))
CANDIDATES = json.loads((ROOT / "tests" / "golden" / "biprime.json").read_text())["candidates"]
CLASSES = {}
for _c in CANDIDATES:
    CLASSES.setdefault(_c["label"].split("_")[0], []).append(unhex(_c["modulus"]))
CLASSES.update({"odd262": [(1 << 261) + 0x1F1], "odd4103": [(1 << 4102) + 0x1F1], "odd8204": [(1 << 8203) + 0x1F1],
                "odd8401": [(1 << 8400) + 0x1F1]})
SHAPES = {"one": (1, 1), "ragged": (3, 5), "group_across_wavefronts": (2, 40)}


def lanes(modulus):
    """Lanes per row of the 9-limb geometry (csrc/mx_host.hpp: choose_geometry)."""
    nblk = -(-(modulus.bit_length() + 4) // (29 * 9))
    k = 1
    while k < nblk:
        k *= 2
    return k


def moduli_of(label, count):
    """`count` odd moduli of the class: its own first, then numbers of the widest one's length."""
    own = CLASSES[label]
    rnd = random.Random(label)
    bits = max(m.bit_length() for m in own)
    return (own + [rnd.getrandbits(bits - 1) | (1 << (bits - 1)) | 1 for _ in range(max(0, count - len(own)))])[:count]


def test_the_moduli_cover_every_group_width():
    assert sorted({lanes(max(ms)) for ms in CLASSES.values()}) == [1, 2, 4, 8, 16, 32, 64]
    assert {label: lanes(max(ms)) for label, ms in CLASSES.items()} == {
        "k64": 1, "k128": 1, "k1024": 4, "k2048": 8, "odd262": 2, "odd4103": 16, "odd8204": 32, "odd8401": 64}


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


def ints_of(eng, out_t):
    from protocols.distributed_keygen_amd import limbs

    return limbs.unpack(eng.to_host(out_t.reshape(-1, out_t.shape[-1])))


def nested(flat, G):
    return [flat[c : c + G] for c in range(0, len(flat), G)]


def edge_draws(modulus, bits):
    return [0, modulus - 1, modulus, modulus + 1, (1 << bits) - 1]


def draws_for(mods, G, rnd):
    """S * G draws of B + 64 bits with every edge draw of every modulus in front of its group (as far as G reaches)."""
    bits = gm.draw_bits(mods)
    draws = []
    for c, n in enumerate(mods):
        edge = edge_draws(n, bits)
        draws.extend(edge[(k + c) % 5] if k < 5 else rnd.getrandbits(bits) for k in range(G))
    return draws


# ------------------------------------------------------------------ shares: host-supplied draws, bit-exact against the model
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("label", sorted(CLASSES))
def test_shares_equal_the_model_for_host_supplied_edge_draws(eng, label, shape):
    import torch

    S, G = SHAPES[shape]
    mods = moduli_of(label, S)
    limbs = gm.draw_bits(mods) - 64 + 31 >> 5
    draws = draws_for(mods, G, random.Random(f"{label}/{shape}"))
    out_t = eng.generator_shares_t(mods, G, draws_t=rows_t(eng, draws, gm.draw_words(mods)))
    assert out_t.dtype == torch.int32 and tuple(out_t.shape) == (S * G, limbs)
    got = nested(ints_of(eng, out_t), G)
    assert got == gm.shares_of_draws(draws, mods, G)
    assert all(0 <= s < n for row, n in zip(got, mods) for s in row)


@pytest.mark.parametrize("label", sorted(CLASSES))
def test_every_edge_draw_of_a_single_row(eng, label):
    """1 x 1 has room for one draw: all five edges, one launch each."""
    n = CLASSES[label][0]
    for d in edge_draws(n, n.bit_length() + 64):
        out_t = eng.generator_shares_t([n], 1, draws_t=rows_t(eng, [d], gm.draw_words([n])))
        assert ints_of(eng, out_t) == [d % n], (label, hex(d))


def test_shares_over_several_workgroups_at_key_length_128(eng):
    S, G = 33, 160
    mods = moduli_of("k128", S)
    draws = draws_for(mods, G, random.Random("several workgroups"))
    got = nested(ints_of(eng, eng.generator_shares_t(mods, G, draws_t=rows_t(eng, draws, gm.draw_words(mods)))), G)
    assert got == gm.shares_of_draws(draws, mods, G)


@pytest.mark.parametrize("labels", [("k64", "k128"), ("k128", "odd262"), ("k64", "k2048"), ("k1024", "k64", "k2048")])
def test_moduli_of_different_bit_lengths_share_a_launch(eng, labels):
    """B, the draw width and the lane group come from the widest modulus; the short ones are reduced all the same."""
    mods = [m for label in labels for m in moduli_of(label, 2)]
    assert len({m.bit_length() for m in mods}) >= 2
    G = 7
    draws = draws_for(mods, G, random.Random("/".join(labels)))
    got = nested(ints_of(eng, eng.generator_shares_t(mods, G, draws_t=rows_t(eng, draws, gm.draw_words(mods)))), G)
    assert got == gm.shares_of_draws(draws, mods, G)
    # ... and summed: three parties' unreduced rows
    limbs = max(m.bit_length() for m in mods) + 31 >> 5
    rnd = random.Random(5)
    by_party = {j: [[rnd.getrandbits(32 * limbs) for _ in range(G)] for _ in mods] for j in (1, 2, 3)}
    shares_t = eng.to_device(np.stack([_pack(by_party[j], limbs) for j in (1, 2, 3)]))
    assert nested(ints_of(eng, eng.generator_sum_t(shares_t, mods, G)), G) == gm.generators(by_party, mods, G)


def _pack(lists, limbs):
    from protocols.distributed_keygen_amd import limbs as _limbs

    return _limbs.pack([v for row in lists for v in row], limbs)


# ------------------------------------------------------------------ shares: device-drawn rows with an injected key
@pytest.mark.parametrize("label,S,G,first_call", [
    ("k128", 5, 160, 0), ("k2048", 2, 9, (1 << 64) + 5), ("k1024", 3, 17, 3), ("odd262", 4, 33, 1 << 33), ("odd8401", 1, 3, 7)])
def test_device_drawn_shares_are_the_models(eng, label, S, G, first_call):
    mods = moduli_of(label, S)
    rng = make_rng(first_call)
    out_t = eng.generator_shares_t(mods, G, rng=rng)
    assert rng.next_call == first_call + 1                          # ONE rows call
    assert nested(ints_of(eng, out_t), G) == gm.shares(KEY, first_call, mods, G)
    # the int level and the device (rows, bits) operand give the same shares for the same call number
    from protocols.distributed_keygen_amd import limbs as _limbs

    limbs = out_t.shape[1]
    pair = (eng.to_device(_limbs.pack(mods, limbs)), max(m.bit_length() for m in mods))
    again = eng.generator_shares_t(pair, G, rng=make_rng(first_call))
    assert eng.torch.equal(again, out_t)
    assert eng.generator_shares_batch(mods, G, make_rng(first_call)) == gm.shares(KEY, first_call, mods, G)


# ------------------------------------------------------------------ sums against sum % N
def _max_parties():
    from protocols.distributed_keygen_amd import _lib

    return _lib.MX_GEN_MAX_PARTIES


@pytest.mark.parametrize("parties", [1, 2, 3, 5, "max"])
@pytest.mark.parametrize("label", sorted(CLASSES))
def test_sums_equal_sum_mod_n(eng, label, parties):
    parties = _max_parties() if parties == "max" else parties
    S, G = 3, 6
    mods = moduli_of(label, S)
    limbs = max(m.bit_length() for m in mods) + 31 >> 5
    top = (1 << 32 * limbs) - 1
    rnd = random.Random(f"{label}/{parties}")
    # per candidate: all N - 1, all N (where a row holds it), all zero, all 2^(32 limbs) - 1, a mixture, random rows
    by_party = {j: [] for j in range(1, parties + 1)}
    for n in mods:
        for j in by_party:
            by_party[j].append([n - 1, min(n, top), 0, top, (n - 1, min(n, top), 0, top)[j % 4], rnd.getrandbits(32 * limbs)])
    shares_t = eng.to_device(np.stack([_pack(by_party[j], limbs) for j in by_party]))
    out_t = eng.generator_sum_t(shares_t, mods, G)
    assert tuple(out_t.shape) == (S * G, limbs)
    got = nested(ints_of(eng, out_t), G)
    assert got == gm.generators(by_party, mods, G)
    assert all(0 <= g < n for row, n in zip(got, mods) for g in row)
    for row, n in zip(got, mods):
        assert row[0] == parties * (n - 1) % n and row[2] == 0 and row[3] == parties * top % n
        if n <= top:
            assert row[1] == 0


def test_sums_over_several_workgroups_and_the_int_level(eng):
    S, G = 33, 160
    mods = moduli_of("k128", S)
    rnd = random.Random(9)
    by_party = {j: [[rnd.randrange(n + 1) for _ in range(G)] for n in mods] for j in (1, 2, 3)}
    by_party[2][0][0] = -5                                           # the int level reduces these on the host
    by_party[3][1][1] = mods[1] << 200
    assert eng.generator_sum_batch([by_party[j] for j in (1, 2, 3)], mods, G) == gm.generators(by_party, mods, G)


# ------------------------------------------------------------------ the golden chain: shares -> generators -> v, on the device
def test_golden_shares_sum_to_the_recorded_generators_and_give_the_recorded_v(eng):
    from protocols.distributed_keygen_amd import limbs as _limbs

    rnd = random.Random(77)
    for cand in CANDIDATES:
        n, parties, keep = unhex(cand["modulus"]), cand["n_parties"], cand["correct_param_biprime"]
        gs = [unhex(g) for g in cand["g_values"]]
        limbs = _limbs.limbs_for(n)
        cols = split_shares(gs, n, parties, rnd, unreduced_below=1 << 32 * limbs)
        assert cols[1][0] == n and any(s >= n for s in cols[1][1:2])
        shares_t = eng.to_device(np.stack([_limbs.pack(cols[j], limbs) for j in sorted(cols)]))
        g_t = eng.generator_sum_t(shares_t, [n], len(gs))
        for i in range(1, parties + 1):
            e = oracle.biprime_exponent(i, n, unhex(cand["p_parts"][i - 1]), unhex(cand["q_parts"][i - 1]))
            v_t, cnt_t = eng.biprime_v_t(g_t, [n], [e], len(gs), keep)        # the generator rows never leave the device
            count = int(cnt_t.cpu()[0])
            assert ints_of(eng, v_t)[:count] == [unhex(v) for v in cand["v"][str(i)]], (cand["label"], i)
        assert ints_of(eng, g_t) == gs, cand["label"]


# ------------------------------------------------------------------ C ABI: every refusal, and nothing launched
def test_c_abi_refusals_launch_nothing(eng):
    from protocols.distributed_keygen_amd import _lib
    from protocols.distributed_keygen_amd import limbs as _limbs

    lib, torch = eng.lib, eng.torch
    n = CLASSES["k128"][0]
    limbs, bits, S, G = _limbs.limbs_for(n), n.bit_length(), 2, 3
    cw = (bits + 64 + 31) // 32
    h_mods = _limbs.pack([n, n], limbs)
    h_even = _limbs.pack([n, n + 1], limbs)
    h_wide = _limbs.pack([n, (1 << bits) + 1], limbs)
    d_mods = eng.to_device(h_mods)
    draws = torch.zeros((S * G, cw), dtype=torch.int32, device=eng.device)
    shares = torch.zeros((3, S * G, limbs), dtype=torch.int32, device=eng.device)
    out = torch.full((S * G, limbs), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    ws_bytes = lib.mx_generator_workspace_bytes(limbs, S)
    assert ws_bytes >= S * limbs * 4 and lib.mx_generator_workspace_bytes(0, S) == -1
    ws = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device=eng.device)
    stream = eng._stream_ptr()
    ARG, SIZE, MOD, WS = -1, -2, -3, -4
    hm = h_mods.ctypes.data
    wide_limbs = 600                              # rows of 19200 bits: room for more than the engine's widest modulus
    wide_bits = 29 * 9 * 64 - 3

    def shares_call(d=draws.data_ptr(), o=out.data_ptr(), m=d_mods.data_ptr(), h=hm, l=limbs, b=bits, s=S, g=G, w=ws.data_ptr(), wb=ws_bytes):
        return lib.mx_generator_shares(d, o, m, h, l, b, s, g, w, wb, stream)

    def sum_call(d=shares.data_ptr(), p=3, o=out.data_ptr(), m=d_mods.data_ptr(), h=hm, l=limbs, b=bits, s=S, g=G, w=ws.data_ptr(), wb=ws_bytes):
        return lib.mx_generator_sum(d, p, o, m, h, l, b, s, g, w, wb, stream)

    refused = [
        (shares_call(d=None), ARG), (shares_call(o=None), ARG), (shares_call(m=None), ARG), (shares_call(w=None), ARG),
        (shares_call(l=0), ARG), (shares_call(s=-1), ARG), (shares_call(g=-1), ARG), (shares_call(b=1), ARG),
        (shares_call(b=32 * limbs + 1), ARG),
        (shares_call(h=h_even.ctypes.data), MOD), (shares_call(h=h_wide.ctypes.data), MOD),
        (shares_call(l=wide_limbs, b=wide_bits, h=None), SIZE), (shares_call(wb=ws_bytes - 256), WS),
        (sum_call(d=None), ARG), (sum_call(o=None), ARG), (sum_call(m=None), ARG), (sum_call(w=None), ARG),
        (sum_call(l=0), ARG), (sum_call(s=-1), ARG), (sum_call(g=-1), ARG), (sum_call(p=0), ARG),
        (sum_call(p=_lib.MX_GEN_MAX_PARTIES + 1), ARG),
        (sum_call(h=h_even.ctypes.data), MOD), (sum_call(l=wide_limbs, b=wide_bits, h=None), SIZE), (sum_call(wb=ws_bytes - 256), WS),
        (shares_call(s=0), 0), (shares_call(g=0), 0), (sum_call(s=0), 0), (sum_call(g=0), 0),      # nothing to do: MX_OK, no launch
    ]
    eng.synchronize()
    assert [rc for rc, _ in refused] == [want for _, want in refused]
    assert bool((out == 0x5A5A5A5A).all()) and bool((ws == 0x5A).all())
    assert _lib.MX_GEN_MAX_PARTIES >= 16 and lib.mx_version() == 404
    # the same calls, not refused, do write
    assert shares_call() == 0 and sum_call() == 0
    eng.synchronize()
    assert bool((out == 0).all()) and not bool((ws == 0x5A).all())


def test_engine_refusals_come_before_any_draw(eng):
    n = CLASSES["k128"][0]
    rng = make_rng(5)
    cw = gm.draw_words([n])
    good = eng.torch.zeros((6, cw), dtype=eng.torch.int32, device=eng.device)
    shares = eng.torch.zeros((2, 6, 5), dtype=eng.torch.int32, device=eng.device)
    refused = [
        lambda: eng.generator_shares_t([n, n], 0, rng=rng),                                      # group_size < 1
        lambda: eng.generator_shares_t([n, n + 1], 3, rng=rng),                                  # an even modulus
        lambda: eng.generator_shares_t([n, 1], 3, rng=rng),                                      # a modulus below 3
        lambda: eng.generator_shares_t([n, n], 3),                                               # neither rng nor rows
        lambda: eng.generator_shares_t([n, n], 3, rng=rng, draws_t=good),                        # both
        lambda: eng.generator_shares_t([n, n], 3, draws_t=good[:, :-1]),                         # rows too narrow
        lambda: eng.generator_shares_t([n, n], 3, draws_t=good[:5]),                             # a row short
        lambda: eng.generator_shares_t([n, n], 3, rng=rng, out_t=good[:5]),                         # an output of another shape
        lambda: eng.generator_shares_batch([n, n + 1], 3, rng),
        lambda: eng.generator_shares_batch([n, n], 0, rng),
        lambda: eng.generator_sum_t(shares, [n, n + 1], 3),
        lambda: eng.generator_sum_t(shares, [n, n, n], 3),                                       # rows of other candidates
        lambda: eng.generator_sum_t(shares[0], [n, n], 3),                                       # not [parties, rows, limbs]
        lambda: eng.generator_sum_t(shares.repeat(9, 1, 1), [n, n], 3),                          # more than MX_GEN_MAX_PARTIES
        lambda: eng.generator_sum_batch([[[1, 2, 3]]], [n, n], 3),                               # a candidate short
        lambda: eng.generator_sum_batch([], [n], 3),                                             # no party
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
        assert rng.next_call == 5, k
    assert eng.generator_shares_batch([], 3, rng) == [] and rng.next_call == 5                   # no survivor: no draw


# ------------------------------------------------------------------ BiprimeRound on the real engine, three parties in one process
@pytest.fixture(scope="module")
def round_128(eng):
    """A round at key_length 128 with three parties: candidate shares, one planted biprime, the Shamir shares of the
    moduli, and every party's BiprimeRound behind reconstruct + sieve."""
    import sympy

    from protocols.distributed_keygen_amd import biprime, synthetic

    rnd = random.Random(128)
    n_parties, t, half, batch = 3, 1, 64, 300
    primes = oracle.small_prime_list(200)
    field = int(sympy.nextprime(1 << (2 * (half + 4) + 44)))
    shares = [synthetic.candidate_shares(rnd, n_parties, half) for _ in range(batch)]

    def prime_shares():
        """candidate shares whose sum is a prime (3 modulo 4 by their shape)"""
        while True:
            parts = synthetic.candidate_shares(rnd, n_parties, half)[0]
            if sympy.isprime(sum(parts)):
                return parts

    shares[5] = (prime_shares(), prime_shares())                   # a planted biprime
    moduli = [sum(p) * sum(q) for p, q in shares]
    points = list(range(1, n_parties + 1))
    by_party = {i: [] for i in points}
    for m in moduli:
        coeffs = [m] + [rnd.randrange(field) for _ in range(2 * t)]
        for i in points:
            by_party[i].append(sum(c * pow(i, e, field) for e, c in enumerate(coeffs)) % field)

    def rounds():
        out = {}
        for i in points:
            out[i] = biprime.BiprimeRound(eng)
            out[i].reconstruct_and_sieve(by_party, field, 2 * t, primes, points=points)
        return out

    return dict(points=points, shares=shares, rounds=rounds, by_party=by_party, field=field, primes=primes, t=t)


def test_biprime_round_draw_sum_v_verdicts_equal_the_list_path(eng, round_128):
    from protocols.distributed_keygen_amd import biprime

    points, keep = round_128["points"], 10
    G = keep * biprime.JACOBI_CORRECTION_FACTOR
    rounds = round_128["rounds"]()
    surv, mods = rounds[1].survivors, rounds[1].moduli
    assert len(mods) >= 3 and 5 in surv
    rng = make_rng(40)
    drawn = {i: rounds[i].draw_generator_shares(rng, G) for i in points}
    assert rng.next_call == 43                                        # one call number per party and round
    assert drawn == {i: gm.shares(KEY, 40 + k, mods, G) for k, i in enumerate(points)}
    want_g = gm.generators(drawn, mods, G)
    ps = {i: [round_128["shares"][k][0][i - 1] for k in surv] for i in points}
    qs = {i: [round_128["shares"][k][1][i - 1] for k in surv] for i in points}
    v, v_list = {}, {}
    for i in points:
        handle = rounds[i].sum_generators({j: drawn[j] for j in points}, i)
        assert isinstance(handle, biprime.GeneratorRows) and len(handle) == len(mods) and handle.rows is not None
        v[i] = rounds[i].v_calculation(handle, i, ps[i], qs[i], keep)
        v_list[i] = biprime.biprime_test_v_calculation_batch(want_g, i, mods, ps[i], qs[i], keep, eng)
        assert v[i] == v_list[i]
        assert handle.lists() == want_g
    v_by = [{i: v[i][c] for i in points} for c in range(len(mods))]
    want = biprime.biprime_test_with_v_i_batch(v_by, mods, keep, eng, errors="return")
    for i in points:
        assert rounds[i].verdicts(v_by, keep, errors="return") == want
    assert want[surv.index(5)] is True
    # a tampered own share is honoured: the sum follows the lists handed in, not the rows kept on the device
    bad = {j: [list(r) for r in drawn[j]] for j in points}
    bad[2][0][0] = (bad[2][0][0] + 1) % mods[0]
    assert rounds[2].sum_generators(bad, 2).lists() == gm.generators(bad, mods, G)


def test_round_coalescer_merges_the_parties_v_calculations_into_one_launch(eng, round_128):
    import asyncio

    from protocols.distributed_keygen_amd import biprime
    from protocols.distributed_keygen_amd.coalesce import RoundCoalescer

    points, keep = round_128["points"], 10
    G = keep * biprime.JACOBI_CORRECTION_FACTOR
    batcher = RoundCoalescer(eng)
    rounds = {i: biprime.BiprimeRound(eng) for i in points}
    rng = make_rng(90)
    shares = round_128["shares"]

    async def party(i, table):
        rnd = rounds[i]
        await batcher.reconstruct_and_sieve(rnd, round_128["by_party"], round_128["field"], 2 * round_128["t"], round_128["primes"],
                                            points=points)
        table[i] = rnd.draw_generator_shares(rng, G)
        await asyncio.sleep(0)
        while len(table) < len(points):                               # the exchange: every party's shares, as ints
            await asyncio.sleep(0)
        handle = rnd.sum_generators({j: table[j] for j in points}, i)
        ps = [shares[k][0][i - 1] for k in rnd.survivors]
        qs = [shares[k][1][i - 1] for k in rnd.survivors]
        return await batcher.v_calculation(rnd, handle, i, ps, qs, keep), handle

    async def run():
        table = {}
        return await asyncio.gather(*[party(i, table) for i in points]), table

    results, table = asyncio.run(run())
    mods = rounds[1].moduli
    want_g = gm.generators(table, mods, G)
    assert batcher.stats["v_requests"] == 3 and batcher.stats["v_launches"] == 1
    for i, (v, handle) in zip(points, results):
        ps = [shares[k][0][i - 1] for k in rounds[i].survivors]
        qs = [shares[k][1][i - 1] for k in rounds[i].survivors]
        assert v == biprime.biprime_test_v_calculation_batch(want_g, i, mods, ps, qs, keep, eng)
        assert handle.lists() == want_g
    v_by = [{i: results[k][0][c] for k, i in enumerate(points)} for c in range(len(mods))]
    want = biprime.biprime_test_with_v_i_batch(v_by, mods, keep, eng, errors="return")
    assert all(rounds[i].verdicts(v_by, keep, errors="return") == want for i in points)
