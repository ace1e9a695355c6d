"""The generator step of a key-generation round on the host side (tools/generators_model.py, biprime.BiprimeRound
.draw_generator_shares / sum_generators, patch.install(generator_rng=...)): the model against plain Python, the order of
the draws, the rule for a party's own rows, the rebound ``__biprime_test_g_generation`` and the golden generators — with
the model-backed doubles of tests/generators_engine.py.  No GPU."""

from __future__ import annotations

import json
import random
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import chacha_model as cm  # noqa: E402
import generators_model as gm  # noqa: E402

from conftest import unhex  # noqa: E402
from fake_engine import FakeEngine  # noqa: E402
import generators_harness as gh  # noqa: E402
from generators_engine import DrawEngine, GeneratorsEngine, split_shares  # noqa: E402
from oracle import oracle  # noqa: E402
from protocols.distributed_keygen_amd import biprime  # noqa: E402
from protocols.distributed_keygen_amd.device_rng import DeviceRng  # noqa: E402

KEY = bytes((5 * k + 9) & 0xFF for k in range(32))
CANDIDATES = json.loads((ROOT / "tests" / "golden" / "biprime.json").read_text())["candidates"]


# ------------------------------------------------------------------ the model against plain Python
def test_model_reduces_every_edge_draw_and_takes_the_width_from_the_widest_modulus():
    mods = [(1 << 61) - 1, (1 << 127) - 1, 1000003, (1 << 200) + 235]
    B = 201
    assert gm.draw_bits(mods) == B + 64 and gm.draw_words(mods) == 9
    assert biprime.generator_draw_width(mods) == (B + 64, 9)
    G = 5
    draws = [d for n in mods for d in (0, n - 1, n, n + 1, (1 << (B + 64)) - 1)]
    got = gm.shares_of_draws(draws, mods, G)
    assert got == [[0, n - 1, 0, 1, ((1 << 265) - 1) % n] for n in mods]
    # device draws: ONE rows call of S * G rows, row c * G + k for generator k of candidate c, B + 64 bits in cw words
    rows = cm.row_ints(KEY, 7, len(mods) * G, B + 64, 9)
    assert gm.device_draws(KEY, 7, mods, G) == rows and all(r < 1 << (B + 64) for r in rows)
    assert gm.shares(KEY, 7, mods, G) == [[rows[c * G + k] % n for k in range(G)] for c, n in enumerate(mods)]
    # the sum is the reference's sum(shares) % N for any integer share
    by_party = {1: gm.shares(KEY, 7, mods, G), 2: [[n] * G for n in mods], 3: [[-3, n << 80, 0, 5 * n + 1, n - 1] for n in mods]}
    want = [[sum(by_party[j][c][k] for j in by_party) % n for k in range(G)] for c, n in enumerate(mods)]
    assert gm.generators(by_party, mods, G) == want
    with pytest.raises(ValueError):
        gm.shares_of_draws(draws[:-1], mods, G)
    with pytest.raises(ValueError):
        gm.generators({1: by_party[1][:-1]}, mods, G)


def test_the_correction_factor_is_the_references():
    ref = ROOT / "oracle" / "_ref" / "distributed_keygen" / "distributed_keygen.py"
    if ref.exists():
        assert f"JACOBI_CORRECTION_FACTOR = {biprime.JACOBI_CORRECTION_FACTOR}\n" in ref.read_text()
    assert biprime.JACOBI_CORRECTION_FACTOR == 4


# ------------------------------------------------------------------ the module-level functions, with and without the engine forms
def _moduli(rnd, count, bits=(60, 66)):
    return [(rnd.getrandbits(rnd.choice(bits)) | (1 << 50) | 1) for _ in range(count)]


@pytest.mark.parametrize("engine_class", [DrawEngine, GeneratorsEngine])
def test_module_level_shares_and_sums_equal_the_model(engine_class):
    rnd = random.Random(3)
    mods, G = _moduli(rnd, 6), 8
    eng, rng = engine_class(), DeviceRng(key=KEY, first_call=20)
    mine = biprime.biprime_test_g_shares_batch(mods, G, rng, eng)
    assert mine == gm.shares(KEY, 20, mods, G) and rng.next_call == 21
    bits, words = gm.draw_bits(mods), gm.draw_words(mods)
    assert [c for c in eng.gen_calls if c[0] == "chacha"] == [("chacha", 20, len(mods) * G, bits, words)]
    others = {2: [[rnd.randrange(n + 1) for _ in range(G)] for n in mods], 3: [[n, -1, n << 70] + [0] * (G - 3) for n in mods]}
    table = {1: mine, **others}
    assert biprime.biprime_test_g_sum_batch([table[j] for j in (1, 2, 3)], mods, G, eng) == gm.generators(table, mods, G)
    assert biprime.biprime_test_g_shares_batch([], G, rng, eng) == [] and rng.next_call == 21


@pytest.mark.parametrize("engine_class", [DrawEngine, GeneratorsEngine])
def test_no_call_number_is_taken_on_a_refusal(engine_class):
    eng, rng = engine_class(), DeviceRng(key=KEY, first_call=5)
    rnd = biprime.BiprimeRound(eng)
    rnd.moduli, rnd.survivors = [1000003, 1000033], [0, 1]
    refused = [
        lambda: biprime.biprime_test_g_shares_batch([1000003, 1000004], 4, rng, eng),          # an even modulus
        lambda: biprime.biprime_test_g_shares_batch([1000003, 1], 4, rng, eng),                # a modulus below 3
        lambda: biprime.biprime_test_g_shares_batch([1000003], 0, rng, eng),                   # no generator
        lambda: biprime.biprime_test_g_shares_batch([1000003], 4, None, eng),                  # no generator of rows
        lambda: rnd.draw_generator_shares(rng, 0),
        lambda: rnd.draw_generator_shares(None, 4),
        lambda: biprime.biprime_test_g_sum_batch([[[1, 2]]], [1000003], 3, eng),               # a share short
        lambda: biprime.biprime_test_g_sum_batch([], [1000003], 3, eng),                       # no party
        lambda: biprime.biprime_test_g_sum_batch([[[1, 2, 3]]], [1000004], 3, eng),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
        assert rng.next_call == 5 and not eng.gen_calls, k
    assert rnd.draw_generator_shares(rng, 4) == gm.shares(KEY, 5, rnd.moduli, 4) and rng.next_call == 6      # one per round


# ------------------------------------------------------------------ BiprimeRound with the double
def _sieved_round(eng, rnd):
    import sympy

    prime = int(sympy.nextprime(1 << 150))
    degree, points = 2, [1, 2, 3]
    moduli = [(rnd.getrandbits(62) | 1) * (rnd.getrandbits(62) | 1) for _ in range(300)]
    cols = {i: [] for i in points}
    for m in moduli:
        co = [m] + [rnd.randrange(prime) for _ in range(degree)]
        for i in points:
            cols[i].append(sum(c * i ** k for k, c in enumerate(co)) % prime)
    primes = [int(q) for q in sympy.primerange(3, 150)]
    out = biprime.BiprimeRound(eng)
    out.reconstruct_and_sieve(cols, prime, degree, primes, points=points)
    assert len(out.moduli) >= 10
    return out


@pytest.mark.parametrize("engine_class", [FakeEngine, DrawEngine, GeneratorsEngine])
def test_round_draw_exchange_sum_v_equals_the_list_path(engine_class):
    """draw -> exchange -> sum -> v_calculation(handle) against the same steps on lists; engines without the generator
    forms (FakeEngine: not even rows — the own shares then come from the model) run the sum and the v-calculation
    through the list-level functions."""
    rnd = random.Random(21)
    eng = engine_class()
    this = _sieved_round(eng, rnd)
    mods, keep = this.moduli, 5
    G = keep * biprime.JACOBI_CORRECTION_FACTOR
    rng = DeviceRng(key=KEY, first_call=33)
    own = this.draw_generator_shares(rng, G) if engine_class is not FakeEngine else gm.shares(KEY, 33, mods, G)
    assert own == gm.shares(KEY, 33, mods, G)
    table = {2: own, 1: [[rnd.randrange(n + 1) for _ in range(G)] for n in mods], 3: [[rnd.randrange(n) for _ in range(G)] for n in mods]}
    want_g = gm.generators(table, mods, G)
    handle = this.sum_generators(table, 2)
    assert isinstance(handle, biprime.GeneratorRows) and len(handle) == len(mods) and handle.group_size == G
    ps = [rnd.getrandbits(50) for _ in mods]
    qs = [rnd.getrandbits(50) for _ in mods]
    calls_before = list(getattr(eng, "gen_calls", []))
    v = this.v_calculation(handle, 2, ps, qs, keep)
    assert v == biprime.biprime_test_v_calculation_batch(want_g, 2, mods, ps, qs, keep, FakeEngine())
    assert handle.lists() == want_g
    if engine_class is GeneratorsEngine:
        assert handle.rows is not None and ("own_share_rows_from_device", len(mods)) in calls_before
        assert eng.gen_calls[-1] == ("v_from_generator_rows", len(mods))      # the handle's rows went to the v-calculation as they are
        # the same through the merged form of co-located parties
        other = biprime.BiprimeRound(eng)
        other.adopt_sieve(this)
        h2 = other.sum_generators(dict(table), 3)
        assert h2 == handle and h2 is not handle
        merged = biprime.BiprimeRound.v_calculation_merged([this, other], [(handle, 2, ps, qs, keep), (h2, 3, qs, ps, keep)])
        assert merged[0] == v and merged[1] == biprime.biprime_test_v_calculation_batch(want_g, 3, mods, qs, ps, keep, FakeEngine())
    else:
        assert handle.rows is None


def test_own_rows_stand_in_only_for_the_drawn_lists():
    rnd = random.Random(8)
    eng = GeneratorsEngine()
    this = _sieved_round(eng, rnd)
    mods, G = this.moduli, 6
    own = this.draw_generator_shares(DeviceRng(key=KEY, first_call=1), G)
    other = [[rnd.randrange(n) for _ in range(G)] for n in mods]

    def summed(mine):
        eng.gen_calls.clear()
        got = this.sum_generators({1: other, 2: mine}, 2).lists()
        assert got == gm.generators({1: other, 2: mine}, mods, G)
        return any(c[0] == "own_share_rows_from_device" for c in eng.gen_calls)

    assert summed(own) is True                                          # the very lists that were drawn
    assert summed([list(r) for r in own]) is True                        # equal copies (what the containers hand back)
    tampered = [list(r) for r in own]
    tampered[3][2] = (tampered[3][2] + 1) % mods[3]
    assert summed(tampered) is False                                     # a changed share is honoured: packed like any other
    assert summed([[n] * G for n in mods]) is False
    eng.gen_calls.clear()
    this.sum_generators({1: other, 3: own}, 2)                           # this party's index is not among the shares
    assert not any(c[0] == "own_share_rows_from_device" for c in eng.gen_calls)
    # a new sieve forgets the drawn rows
    this.adopt_sieve(this)
    assert summed(own) is False


# ------------------------------------------------------------------ generators from the golden data
def test_golden_generators_are_the_sums_of_their_shares():
    rnd = random.Random(2024)
    eng = GeneratorsEngine()
    for cand in CANDIDATES:
        n, parties = unhex(cand["modulus"]), cand["n_parties"]
        gs = [unhex(g) for g in cand["g_values"]]
        cols = split_shares(gs, n, parties, rnd)
        assert cols[1][0] == n and (len(gs) < 2 or cols[1][1] < 0)       # a share equal to N and an unreduced one
        table = {j: [cols[j]] for j in cols}
        assert gm.generators(table, [n], len(gs)) == [gs]
        assert biprime.biprime_test_g_sum_batch([table[j] for j in sorted(table)], [n], len(gs), eng) == [gs]
        assert biprime.biprime_test_g_sum_batch([table[j] for j in sorted(table)], [n], len(gs), FakeEngine()) == [gs]
        this = biprime.BiprimeRound(eng)
        this.moduli, this.survivors = [n], [0]
        handle = this.sum_generators(table, 1)
        assert handle.lists() == [gs]
        if n.bit_length() > 1100:                                        # (the double's Jacobi symbols and modexps are Python's)
            continue
        e = oracle.biprime_exponent(1, n, unhex(cand["p_parts"][0]), unhex(cand["q_parts"][0]))
        got = eng.biprime_v_batch(None, [e], [n], cand["correct_param_biprime"], g_rows=(handle.rows, len(gs)))
        assert got == [[unhex(v) for v in cand["v"]["1"]]], cand["label"]


# ------------------------------------------------------------------ patch.install(generator_rng=...) on the stand-in package
# (the same checks run on the real reference in tests/test_patch_reference_generators.py)
def test_patched_generator_step_is_a_drop_in():
    gh.check_patched_generator_step_is_a_drop_in(*gh.standin_package())


def test_the_rebound_method_keeps_the_references_signature_and_return_type():
    gh.check_the_rebound_method_keeps_the_references_signature_and_return_type(*gh.standin_package())


def test_install_without_generator_rng_leaves_the_method_alone():
    gh.check_install_without_generator_rng_leaves_the_method_alone(*gh.standin_package())
