"""Host logic of the range proofs (range_proof.py) over the Python-int double of the engine (range_engine.py), bit-exact
against the model (tools/range_model.py).  No GPU."""

from __future__ import annotations

import ctypes
import random

import pytest

import range_cases as rc
from range_cases import rm
from range_engine import RangeEngine, tamperings

from protocols.distributed_keygen_amd import limbs, range_proof
from protocols.distributed_keygen_amd.device_rng import DeviceRng

N1K = rc.modulus(1024)
BITS = 64


def proven(n, aux_bits, bits, count, call=40, label=rc.LABEL):
    eng = RangeEngine()
    params, secret, mpar = rc.parameters(aux_bits)
    msgs, rands, cts = rc.statements(n, bits, count)
    proofs = range_proof.prove_batch(n, params, bits, msgs, rands, label, rng=DeviceRng(key=rc.KEY, first_call=call), ciphertexts=cts, engine=eng)
    return eng, params, mpar, msgs, rands, cts, proofs


def test_the_golden_parameters_come_from_the_recorded_seed():
    assert rc.PARAMS128["seed"] == 20261020 and "seeded search" in rc.PARAMS128["provenance"]
    ph, qh, lam, tau = rc.secrets128()
    assert ph != qh and (ph * qh).bit_length() == 128 and {ph, qh}.isdisjoint(rc.primes(128))
    for x in (ph, qh, (ph - 1) // 2, (qh - 1) // 2):
        assert pow(2, x - 1, x) == 1 and pow(3, x - 1, x) == 1
    assert {k: v for k, v in rm.golden_parameters(20261020).items()} == rc.PARAMS128


@pytest.mark.parametrize("key_length,aux_bits,bits", [(1024, 128, 64), (1024, 2048, 1), (2048, 1024, 2048 - 259)])
def test_the_model_is_complete(key_length, aux_bits, bits):
    n = rc.modulus(key_length)
    _, _, mpar = rc.parameters(aux_bits)
    msgs, rands, cts = rc.statements(n, bits, 3)
    cols = rc.model_proofs(n, mpar, bits, rc.LABEL, msgs, rands, 9)
    for k, c in enumerate(cts):
        assert rm.verify(n, mpar, bits, rc.LABEL, c, [col[k] for col in cols])


def test_proofs_equal_the_model_bit_for_bit_and_verify():
    eng, params, mpar, msgs, rands, cts, proofs = proven(N1K, 128, BITS, 7)
    assert proofs.to_ints() == rc.model_proofs(N1K, mpar, BITS, rc.LABEL, msgs, rands, 40)
    assert range_proof.context(N1K, params, BITS, rc.LABEL) == rm.context(N1K, mpar, BITS, rc.LABEL)
    assert range_proof.shape(N1K, params.nh, BITS) == rm.shape(N1K, mpar, BITS) == eng.range_shape(N1K, params.nh, BITS)
    assert range_proof.verify_batch(N1K, params, BITS, cts, proofs, rc.LABEL, engine=eng) == [True] * 7
    again = range_proof.RangeProofs.from_ints(*proofs.to_ints(), N1K, params, BITS)
    assert again.unfit == [False] * 7
    assert range_proof.verify_batch(N1K, params, BITS, cts, again, rc.LABEL, engine=eng) == [True] * 7
    # a short auxiliary modulus: every product of two powers is one modexp per term, the message term BITS long
    assert not [c for c in eng.calls if c[0] == "multiexp_mod"]
    assert [c for c in eng.calls if c[0] == "powmod_multi"][:2] == [("powmod_multi", 7, 1, 128 + 128), ("powmod_multi", 7, 1, BITS)]


def test_an_auxiliary_modulus_above_the_crossover_takes_the_multi_exponentiation():
    """Above 2084 bits the shared-base products run through multiexp_mod_t (the longer term first, a length per term); the
    proofs are the model's either way.  The mechanics need no safe primes: any odd modulus with units s and t will do."""
    import random

    eng = RangeEngine()
    nh = random.Random(21).getrandbits(2100) | (1 << 2099) | 1
    params = range_proof.RangeParameters(nh, pow(3, 12345, nh), 9)
    mpar = rm.Parameters(*params.to_ints())
    assert eng.range_uses_multiexp(nh) and not eng.range_uses_multiexp(nh >> 16)
    msgs, rands, cts = rc.statements(N1K, BITS, 3)
    proofs = range_proof.prove_batch(N1K, params, BITS, msgs, rands, rc.LABEL, rng=DeviceRng(key=rc.KEY, first_call=40), ciphertexts=cts, engine=eng)
    assert proofs.to_ints() == rc.model_proofs(N1K, mpar, BITS, rc.LABEL, msgs, rands, 40)
    assert range_proof.verify_batch(N1K, params, BITS, cts, proofs, rc.LABEL, engine=eng) == [True] * 3
    shared = [c for c in eng.calls if c[0] == "multiexp_mod"]
    assert len(shared) == 3 and all(c[1:4] == (2, 3, 2) for c in shared)          # S, C and the left of the second equation
    assert all(c[3] == 128 for c in eng.calls if c[0] == "powmod_multi")          # rho r^e and C S^e: per-row bases never take it


@pytest.mark.parametrize("key_length,aux_bits", [(1024, 2048), (2048, 1024)])
def test_mixed_widths_equal_the_model(key_length, aux_bits):
    n = rc.modulus(key_length)
    eng, params, mpar, msgs, rands, cts, proofs = proven(n, aux_bits, 32, 3)
    assert proofs.to_ints() == rc.model_proofs(n, mpar, 32, rc.LABEL, msgs, rands, 40)
    assert range_proof.verify_batch(n, params, 32, cts, proofs, rc.LABEL, engine=eng) == [True] * 3


def test_every_tampering_is_false_for_its_row_only():
    eng, params, mpar, msgs, rands, cts, proofs = proven(N1K, 128, BITS, 3)
    ints = tuple(list(col) for col in proofs.to_ints())
    other = rm.encrypt(N1K, 5, 77)
    for name, tcts, *cols in tamperings(N1K, params, ints, cts, other):
        spoiled = range_proof.RangeProofs.from_ints(*cols, N1K, params, BITS)
        assert range_proof.verify_batch(N1K, params, BITS, tcts, spoiled, rc.LABEL, engine=eng) == [True, False, True], name
        assert not rm.verify(N1K, mpar, BITS, rc.LABEL, tcts[1], [col[1] for col in cols]), name
    # the label, the claimed length and the parameters are bound by ctx: every row fails
    assert range_proof.verify_batch(N1K, params, BITS, cts, proofs, b"another session", engine=eng) == [False] * 3
    assert range_proof.verify_batch(N1K, params, BITS + 1, cts, proofs, rc.LABEL, engine=eng) == [False] * 3
    other_params, _, _ = rc.parameters(128)
    other_params = range_proof.RangeParameters(other_params.nh, other_params.s * other_params.t % other_params.nh, other_params.t)
    assert range_proof.verify_batch(N1K, other_params, BITS, cts, proofs, rc.LABEL, engine=eng) == [False] * 3
    p1k, _, _ = rc.parameters(1024)
    moved = range_proof.RangeProofs.from_ints(*ints, N1K, p1k, BITS)          # another Nh altogether: rows re-packed at its widths
    assert range_proof.verify_batch(N1K, p1k, BITS, cts, moved, rc.LABEL, engine=eng) == [False] * 3


def test_the_bounds_of_z1_and_z3_are_exact():
    """z1 = 2^(l + 257) - 1 passes the range check and 2^(l + 257) does not; likewise z3 at 2^(Bh + 385).  The challenge
    hashes the commitments, so nobody can build a proof whose equations hold for a z1 of their choosing: the exact bound
    is shown where it is enforced, on the range check (``range_bounds_t``), in the model and in the double alike."""
    eng, params, mpar, msgs, rands, cts, proofs = proven(N1K, 128, BITS, 2)
    sh = range_proof.shape(N1K, params.nh, BITS)
    assert (sh["z1_bits"], sh["z3_bits"]) == (BITS + 257, 128 + 385)
    ints = [list(col) for col in proofs.to_ints()]
    for which, top in ((3, 1 << sh["z1_bits"]), (5, 1 << sh["z3_bits"])):
        for value, expect in ((top - 1, True), (top, False)):
            cols = [list(col) for col in ints]
            cols[which][1] = value
            spoiled = range_proof.RangeProofs.from_ints(*cols, N1K, params, BITS)
            assert spoiled.unfit == [False, False]
            c_t = eng.to_device(limbs.pack(cts, sh["limbs2"]))
            assert list(eng.range_bounds_t(c_t, *(eng.to_device(r) for r in spoiled.rows()), N1K, params.nh, BITS)) == [True, expect]
            assert rm.in_range(N1K, mpar, BITS, cts[1], [col[1] for col in cols]) is expect
            assert range_proof.verify_batch(N1K, params, BITS, cts, spoiled, rc.LABEL, engine=eng) == [True, False]


def test_the_slack_and_what_lies_beyond_it():
    """An honest prover with m = 2^l still verifies (the documented slack); one with m >= 2^(l + 257) cannot."""
    eng = RangeEngine()
    params, _, mpar = rc.parameters(128)
    sh = range_proof.shape(N1K, params.nh, BITS)
    alpha, mu, gamma, rho = (d[0] for d in rm.device_draws(rc.KEY, 3, 1, N1K, mpar, BITS))
    r = 12345
    # m = 2^l (one past the claimed range): still verifies — the slack
    m = 1 << BITS
    c = rm.encrypt(N1K, m, r)
    proof = rm.prove(N1K, mpar, BITS, rc.LABEL, m, r, alpha, mu, gamma, rho)
    assert rm.verify(N1K, mpar, BITS, rc.LABEL, c, proof)
    got = range_proof.prove_batch(N1K, params, BITS, [m], [r], rc.LABEL, rng=DeviceRng(key=rc.KEY, first_call=3), engine=eng)
    assert tuple(col[0] for col in got.to_ints()) == proof
    assert range_proof.verify_batch(N1K, params, BITS, [c], got, rc.LABEL, engine=eng) == [True]
    # m >= 2^(l + E + K + 1): z1 = alpha + e m >= 2^(l + 257) unless e = 0 — the honest algorithm cannot make it verify
    m = 1 << sh["z1_bits"]
    c = rm.encrypt(N1K, m, r)
    proof = rm.prove(N1K, mpar, BITS, rc.LABEL, m, r, alpha, mu, gamma, rho)
    assert proof[3] >= 1 << sh["z1_bits"] and not rm.verify(N1K, mpar, BITS, rc.LABEL, c, proof)
    # this z1 does not even fit its row: the response kernel says so in its status, and the double lets no prover pass with one set
    assert proof[3] >> (32 * sh["z1_words"])
    with pytest.raises(AssertionError, match="overflowed"):
        range_proof.prove_batch(N1K, params, BITS, [m], [r], rc.LABEL, rng=DeviceRng(key=rc.KEY, first_call=3), engine=eng)
    # what the engine returns then — the low words of z1 beside the rest of the proof — is refused like any other
    cut = proof[:3] + (proof[3] & ((1 << (32 * sh["z1_words"])) - 1),) + proof[4:]
    got = range_proof.RangeProofs.from_ints(*([v] for v in cut), N1K, params, BITS)
    assert got.unfit == [False] and range_proof.verify_batch(N1K, params, BITS, [c], got, rc.LABEL, engine=eng) == [False]


def test_the_extreme_messages_prove():
    eng, params, mpar, msgs, rands, cts, proofs = proven(N1K, 128, BITS, 3)
    assert msgs[:2] == [0, (1 << BITS) - 1]
    assert range_proof.verify_batch(N1K, params, BITS, cts, proofs, rc.LABEL, engine=eng) == [True] * 3


def test_encrypt_with_proof_round_trip():
    eng = RangeEngine()
    params, _, mpar = rc.parameters(128)
    cts, proofs = range_proof.encrypt_with_proof(N1K, params, BITS, [3, 0, (1 << BITS) - 1], rc.LABEL, rng=DeviceRng(key=rc.KEY, first_call=1), engine=eng)
    assert range_proof.verify_batch(N1K, params, BITS, cts, proofs, rc.LABEL, engine=eng) == [True] * 3
    for k, c in enumerate(cts):
        assert rm.verify(N1K, mpar, BITS, rc.LABEL, c, [col[k] for col in proofs.to_ints()])
    with pytest.raises(ValueError):
        range_proof.encrypt_with_proof(N1K, params, BITS, [1 << BITS], rc.LABEL, engine=eng)


def test_every_refusal_happens_without_an_engine_call():
    eng = RangeEngine()
    params, _, _ = rc.parameters(128)
    n128 = rc.modulus(128)
    msgs, rands, cts = rc.statements(N1K, BITS, 2)
    empty = range_proof.prove_batch(N1K, params, BITS, [], [], rc.LABEL, engine=eng)
    assert len(empty) == 0 and range_proof.verify_batch(N1K, params, BITS, [], empty, rc.LABEL, engine=eng) == []
    good = range_proof.prove_batch(N1K, params, BITS, msgs, rands, rc.LABEL, rng=DeviceRng(key=rc.KEY), ciphertexts=cts, engine=eng)
    eng.calls.clear()
    for bad in (lambda: range_proof.prove_batch(n128, params, 1, [0], [3], rc.LABEL, engine=eng),             # no l fits a 128-bit N
                lambda: range_proof.prove_batch(N1K, params, 1024 - 258, msgs, rands, rc.LABEL, engine=eng),   # l + 258 > bits(N) - 1
                lambda: range_proof.prove_batch(N1K, params, 0, msgs, rands, rc.LABEL, engine=eng),
                lambda: range_proof.prove_batch(N1K, params, BITS, msgs, rands[:1], rc.LABEL, engine=eng),
                lambda: range_proof.prove_batch(N1K, params, BITS, msgs, rands, rc.LABEL, ciphertexts=cts[:1], engine=eng),
                lambda: range_proof.prove_batch(N1K, params, BITS, [-1, 0], rands, rc.LABEL, engine=eng),
                lambda: range_proof.prove_batch(N1K, params, BITS, msgs, rands, "a str label", engine=eng),
                lambda: range_proof.prove_batch(N1K - 1, params, BITS, msgs, rands, rc.LABEL, engine=eng),
                lambda: range_proof.verify_batch(N1K, params, 1024 - 258, cts, good, rc.LABEL, engine=eng),
                lambda: range_proof.verify_batch(n128, params, 1, cts, good, rc.LABEL, engine=eng),
                lambda: range_proof.verify_batch(N1K, params, BITS, cts[:1], good, rc.LABEL, engine=eng),
                lambda: range_proof.encrypt_with_proof(n128, params, 1, [0], rc.LABEL, engine=eng),
                lambda: range_proof.RangeParameters(params.nh + 1, params.s, params.t),                        # an even Nh
                lambda: range_proof.RangeParameters(params.nh, 0, params.t),
                lambda: range_proof.RangeProofs.from_ints([1], [1], [1], [1], [1], [], N1K, params, BITS)):
        with pytest.raises(ValueError):
            bad()
    assert eng.calls == []
    assert range_proof.shape(N1K, params.nh, 1024 - 259)["z1_bits"] == 1022          # the longest length a 1024-bit N carries


def test_the_parameter_proof():
    params, secret, mpar = rc.parameters(128)
    proof = params.prove_parameters(secret, rand=random.Random(3))
    assert proof == rm.prove_parameters(mpar, secret[1], secret[2], secret[0], random.Random(3))
    assert params.verify_parameters(proof) and rm.verify_parameters(mpar, proof)
    assert params.to_ints() == (mpar.nh, mpar.s, mpar.t) and range_proof.RangeParameters.from_ints(*params.to_ints()).verify_parameters(proof)
    # s = -t^lambda is not in <t> (t generates the squares; -1 is not one modulo a product of primes 3 mod 4)
    outside = range_proof.RangeParameters(params.nh, params.nh - params.s, params.t)
    forged = rm.prove_parameters(rm.Parameters(*outside.to_ints()), secret[1], secret[2], secret[0], random.Random(3))
    assert not outside.verify_parameters(forged) and not rm.verify_parameters(rm.Parameters(*outside.to_ints()), forged)
    with pytest.raises(ValueError):
        outside.prove_parameters(secret)
    # malformed proofs are False, not exceptions
    a, z = proof
    for bad in ((a[:-1], z), (a, z[:-1]), ([0] + a[1:], z), (a, [params.nh] + z[1:]), (a, [z[0] + 1] + z[1:]), None, (a,), ("x", z)):
        assert not params.verify_parameters(bad)


def test_generate_draws_safe_primes_through_the_engine():
    eng = RangeEngine()
    params, secret = range_proof.RangeParameters.generate(128, engine=eng, rng=DeviceRng(key=rc.KEY, first_call=3), rand=random.Random(2))
    lam, ph, qh = secret
    assert ph * qh == params.nh and params.bits == 128 and pow(params.t, lam, params.nh) == params.s
    for x in (ph, qh, (ph - 1) // 2, (qh - 1) // 2):
        assert pow(2, x - 1, x) == 1
    assert any(c[0] == "safe_prime_search" for c in eng.calls) and any(c[0] == "safe_prime" for c in eng.calls)      # found, then vetted
    assert params.verify_parameters(params.prove_parameters(secret, rand=random.Random(4)))


def test_the_header_declares_what_the_library_exports():
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    lanes, lpl = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    assert lib.mx_multiexp_instances(lanes, lpl, 8) == 7 and list(lanes)[:7] == [1, 2, 4, 8, 16, 32, 64] and set(list(lpl)[:7]) == {9}
    assert lib.mx_multiexp_instances(None, None, 0) == 7 and lib.mx_multiexp_instances(None, None, 3) == -1
    for name in ("mx_multiexp_shape", "mx_multiexp_workspace_bytes", "mx_multiexp_run", "mx_multiexp_instances", "mx_response_rows"):
        assert name in (rc.HERE.parent / "include" / "mxpaillier.h").read_text()
    assert lib.mx_version() == 404


def test_every_multiexp_instance_has_a_case():
    """mx_multiexp_instances against the cases test_gpu_range_proofs.py runs (range_cases.MULTIEXP_CASES), through the
    library's own shape query — an instance without a case fails here, on the CPU."""
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    lanes, lpl = (ctypes.c_int * 16)(), (ctypes.c_int * 16)()
    count = lib.mx_multiexp_instances(lanes, lpl, 16)
    reachable = {(lanes[i], lpl[i]) for i in range(count)}
    covered, rows_of_k = set(), {}
    for name, mod, counts, terms, window, wbits, shared in rc.MULTIEXP_CASES:
        k, l, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.mx_multiexp_shape(mod.bit_length(), terms, max(counts), terms, wbits, window, k, l, w) == 0, name
        assert w.value == window
        covered.add((k.value, l.value))
        rows_of_k.setdefault(k.value, set()).update(counts)
        assert max(counts) <= 9 or mod.bit_length() < 4096, name
        cmod, inputs, index, weights = rc.multiexp_case(name)[:4]
        used = {inputs[i] for row in index for i in row}
        assert {0, 1} <= used and (cmod - 1 in used or len(inputs) < 3), name          # the bases 0, 1 and M - 1 are read by some row
    for k, counts in rows_of_k.items():             # one row fewer and one more than fill a wavefront, for every instance
        assert {64 // k - 1, 64 // k + 1} - {0} <= counts, (k, sorted(counts))
    assert {1, 7, 65} <= set().union(*rows_of_k.values())
    assert {c[3] for c in rc.MULTIEXP_CASES} == {1, 2, 3} and {c[4] for c in rc.MULTIEXP_CASES} == {1, 4, 5, 8}
    assert {c[5] for c in rc.MULTIEXP_CASES} >= {1, 31, 33, 128} and any(c[5] == c[1].bit_length() + 385 for c in rc.MULTIEXP_CASES)
    assert {c[1].bit_length() for c in rc.MULTIEXP_CASES} >= {64, 128, 1024, 2048, 4096}
    assert reachable == covered == {(k, 9) for k in (1, 2, 4, 8, 16, 32, 64)}
    # the automatic window: operation counts within the table budget, 1 .. 8
    k, l, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.mx_multiexp_shape(2048, 2, 10000, 2, 2433, 0, k, l, w) == 0 and (k.value, l.value) == (8, 9) and 5 <= w.value <= 8
    assert lib.mx_multiexp_shape(2048, 20000, 10000, 2, 128, 0, k, l, w) == 0 and 2 <= w.value <= 4
    assert lib.mx_multiexp_shape(2048, 2, 2, 2, 1, 0, k, l, w) == 0 and w.value == 1
    assert lib.mx_multiexp_shape(16701, 2, 2, 2, 8, 0, k, l, w) == -2 and lib.mx_multiexp_shape(2048, 2, 2, 2, 16385, 0, k, l, w) == -1
    assert lib.mx_multiexp_shape(2048, 2, 2, 2, 8, 9, k, l, w) == -1 and lib.mx_multiexp_shape(2048, 2, 2, 2, 8, 0, None, l, w) == -1
    # the queries refuse the counts the run refuses
    for bad in ((2048, 0, 2, 2, 8), (2048, 2, 0, 2, 8), (2048, 2, 2, 0, 8), (2048, 2, 2, 65537, 8), (2048, 2, 2, 2, 0)):
        assert lib.mx_multiexp_shape(*bad, 0, k, l, w) == -1, bad
    assert lib.mx_multiexp_workspace_bytes(2048, 64, 2, 2, 5) == 3 * 256 + 2 * 32 * 8 * 9 * 4          # M, R mod M, two term lengths, two tables
    assert lib.mx_multiexp_workspace_bytes(2048, 64, 2, 65, 5) == 4 * 256 + 2 * 32 * 8 * 9 * 4
    for bad in ((2048, 0, 2, 2, 5), (2048, 64, 0, 2, 5), (2048, 64, 2, 0, 5), (2048, 64, 2, 65537, 5), (2048, 64, 2, 2, 0), (2048, 64, 2, 2, 9)):
        assert lib.mx_multiexp_workspace_bytes(*bad) == -1, bad
    assert lib.mx_multiexp_workspace_bytes(16701, 600, 2, 2, 5) == -2
