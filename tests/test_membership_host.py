"""Host logic of the one-of-k membership proofs (membership.py) over the Python-int double of the engine
(member_engine.py), bit-exact against the model (tools/member_model.py).  No GPU."""

from __future__ import annotations

import numpy as np
import pytest

import member_cases as mc
from member_cases import mm
from member_engine import MemberEngine, forgeries, tamperings

from protocols.distributed_keygen_amd import limbs, membership, slots
from protocols.distributed_keygen_amd.device_rng import DeviceRng

N128, N1K, N2K = mc.modulus(128), mc.modulus(1024), mc.modulus(2048)
M128 = mc.M128


def proven(n, values, count, call=40, label=mc.LABEL):
    eng = MemberEngine()
    index, msgs, rands, cts = mc.statements(n, values, count)
    proofs = membership.prove_batch(n, values, msgs, rands, label, rng=DeviceRng(key=mc.KEY, first_call=call), ciphertexts=cts, engine=eng)
    return eng, index, msgs, rands, cts, proofs


def row_of(cols, r):
    return [col[r] for col in cols]


@pytest.mark.parametrize("key_length", [128, 1024, 2048])
@pytest.mark.parametrize("name", ["bit", "signed", "one_hot", "k16"])
def test_the_model_is_complete_with_every_slot_as_the_real_one(key_length, name):
    n = mc.modulus(key_length)
    values = mc.value_sets(n)[name]
    k = len(values)
    zt, et = mm.device_draws(mc.KEY, 9, k, n, k)
    for i in range(k):
        r = 12345 + i
        c = mm.encrypt(n, values[i], r)
        proof = mm.prove(n, values, mc.LABEL, i, r, zt[i], et[i])
        assert mm.verify(n, values, mc.LABEL, c, proof), (name, i)
        # (the equations once more, independently; the long list at real key lengths leaves the repeat of verify's k
        # N-bit powers to the first and the last slot)
        assert key_length > 128 and k == 16 and 0 < i < k - 1 or mc.equations_hold(n, values, mc.LABEL, c, proof), (name, i)
        assert proof[1][i] == (mm.challenge(mm.context(n, values, mc.LABEL), c, proof[0], mm.limbs_for(n * n)) - sum(et[i]) + et[i][i]) & M128
        assert [e for j, e in enumerate(proof[1]) if j != i] == [e for j, e in enumerate(et[i]) if j != i]
        shifted = c * (1 + n) % (n * n)                                         # the same proof against c (1 + N)
        assert not mm.verify(n, values, mc.LABEL, shifted, proof) and not mc.equations_hold(n, values, mc.LABEL, shifted, proof)


def test_the_models_verify_agrees_with_the_equations_on_spoiled_proofs():
    values = mc.value_sets(N128)["one_hot"]
    zt, et = mm.device_draws(mc.KEY, 3, 1, N128, 5)
    c = mm.encrypt(N128, values[2], 99)
    a, es, zs = mm.prove(N128, values, mc.LABEL, 2, 99, zt[0], et[0])
    for proof in ((a, es, zs), (a, [es[1], es[0]] + es[2:], zs), ([a[0] * 4 % (N128 * N128)] + a[1:], es, zs),
                  (a, es, zs[:-1] + [zs[-1] * 3 % N128]), (a, [(es[0] + 1) & M128, (es[1] - 1) & M128] + es[2:], zs), (a, [es[0] ^ 1] + es[1:], zs)):
        assert mm.verify(N128, values, mc.LABEL, c, proof) == mc.equations_hold(N128, values, mc.LABEL, c, proof) == (proof == (a, es, zs))


@pytest.mark.parametrize("key_length,name,count", [(1024, "bit", 5), (1024, "one_hot", 7), (1024, "k16", 3), (2048, "signed", 3)])
def test_proofs_equal_the_model_bit_for_bit_and_verify(key_length, name, count):
    n = mc.modulus(key_length)
    values = mc.value_sets(n)[name]
    eng, index, msgs, rands, cts, proofs = proven(n, values, count)
    assert proofs.to_ints() == mc.model_proofs(n, values, mc.LABEL, index, rands, 40)
    assert membership.context(n, values, mc.LABEL) == mm.context(n, values, mc.LABEL)
    assert membership.shape(n, len(values)) == mm.shape(n, len(values)) == eng.member_shape(n, len(values))
    assert membership.verify_batch(n, values, cts, proofs, mc.LABEL, engine=eng) == [True] * count
    again = membership.MembershipProofs.from_ints(*proofs.to_ints(), n, len(values))
    assert again.unfit == [False] * count and all((x == eng.to_host(y)).all() for x, y in zip(again.rows(), proofs.rows()))
    assert membership.verify_batch(n, values, cts, again, mc.LABEL, engine=eng) == [True] * count
    # the composition: two draws, ONE inverse per ciphertext, count k wide N-th powers, one multi-exponentiation per side
    k = len(values)
    assert [c for c in eng.calls if c[0] == "modinv"] == [("modinv", count)]
    assert [c for c in eng.calls if c[0] == "member_challenges"] == [("member_challenges", 0, count, k), ("member_challenges", 1, count, k)] + [
        ("member_challenges", 2, count, k)] * 2
    assert [c[1:] for c in eng.calls if c[0] == "multiexp_rows"] == [(count * k, count * k, 1, 128)] + [(2 * count * k, count * k, 2, 128)] * 2


def test_the_double_takes_the_smallest_key_and_equals_the_model():
    """The engine entries take any N the N^2 kernels take (the 260-bit refusal is the module's): the 128-bit golden key,
    k = 2 and k = 5, every slot real somewhere."""
    eng = MemberEngine()
    for name, count in (("bit", 5), ("one_hot", 7)):
        values = mc.value_sets(N128)[name]
        k = len(values)
        sh = eng.member_shape(N128, k)
        index, msgs, rands, cts = mc.statements(N128, values, count)
        ctx = mm.context(N128, values, mc.LABEL)
        rows = eng.member_prove_t(eng.to_device(limbs.pack(cts, sh["limbs2"]).reshape(count, -1)), eng.to_device(np.array(index, dtype=np.uint32)),
                                  eng.to_device(limbs.pack(rands, sh["limbs_n"]).reshape(count, -1)), N128, values, ctx,
                                  rng=DeviceRng(key=mc.KEY, first_call=7))
        assert membership.MembershipProofs(*rows, k).to_ints() == mc.model_proofs(N128, values, mc.LABEL, index, rands, 7)
        assert list(eng.member_verify_t(eng.to_device(limbs.pack(cts, sh["limbs2"]).reshape(count, -1)), *rows, N128, values, ctx)) == [True] * count


@pytest.mark.parametrize("name", ["bit", "one_hot"])
def test_every_tampering_is_false_for_its_row_only(name):
    values = mc.value_sets(N1K)[name]
    k = len(values)
    eng, index, msgs, rands, cts, proofs = proven(N1K, values, 3)
    ints = proofs.to_ints()
    for what, tcts, a, e, z in tamperings(N1K, values, ints, cts):
        spoiled = membership.MembershipProofs.from_ints(a, e, z, N1K, k)
        assert membership.verify_batch(N1K, values, tcts, spoiled, mc.LABEL, engine=eng) == [True, False, True], what
        assert not mm.verify(N1K, values, mc.LABEL, tcts[1], (a[1], e[1], z[1])), what
        assert mm.verify(N1K, values, mc.LABEL, tcts[0], (a[0], e[0], z[0])) and mm.verify(N1K, values, mc.LABEL, tcts[2], (a[2], e[2], z[2]))
    # the label, the list IN ITS ORDER and N are bound by ctx (and by the equations): every row fails
    assert membership.verify_batch(N1K, values, cts, proofs, b"another session", engine=eng) == [False] * 3
    reordered = values[1:] + values[:1]
    assert membership.verify_batch(N1K, reordered, cts, proofs, mc.LABEL, engine=eng) == [False] * 3
    other_n = N1K + 2
    moved = membership.MembershipProofs.from_ints(*ints, other_n, k)
    assert membership.verify_batch(other_n, values, cts, moved, mc.LABEL, engine=eng) == [False] * 3
    assert not any(mm.verify(other_n, values, mc.LABEL, c, row_of(ints, r)) for r, c in enumerate(cts))
    # a ciphertext of a value outside the list has no proof: whatever slot the prover claims, the row is False
    outside = mm.encrypt(N1K, max(values) + 1, rands[1])
    zt, et = mm.device_draws(mc.KEY, 3, 1, N1K, k)
    for claim in range(k):
        forged = mm.prove(N1K, values, mc.LABEL, claim, rands[1], zt[0], et[0], c=outside)
        assert not mm.verify(N1K, values, mc.LABEL, outside, forged)
        got = membership.MembershipProofs.from_ints(*([ints[j][0], forged[j], ints[j][2]] for j in range(3)), N1K, k)
        assert membership.verify_batch(N1K, values, [cts[0], outside, cts[2]], got, mc.LABEL, engine=eng) == [True, False, True]
    # the forgeries that need no witness at all: zero satisfies every equation, so zero is refused
    for what, forged in forgeries(N1K, values, mc.LABEL, outside):
        assert not mm.verify(N1K, values, mc.LABEL, outside, forged) and not mm.in_range(N1K, k, outside, forged), what
        got = membership.MembershipProofs.from_ints(*([ints[j][0], forged[j], ints[j][2]] for j in range(3)), N1K, k)
        assert membership.verify_batch(N1K, values, [cts[0], outside, cts[2]], got, mc.LABEL, engine=eng) == [True, False, True], what


@pytest.mark.parametrize("k", [2, 3, 16])
def test_the_challenge_modes(k):
    eng = MemberEngine()
    e, sims, index = mc.directed_challenges(k)
    count = len(e)
    e_t = eng.to_device(limbs.pack(e, 4).reshape(count, 4))
    sim_t = eng.to_device(limbs.pack([v for row in sims for v in row], 4).reshape(count, 4 * k))
    index_t = eng.to_device(np.array(index, dtype=np.uint32))

    def slots_of(rows_t):
        flat = limbs.unpack(eng.to_host(rows_t).reshape(count * k, 4))
        return [flat[r * k : (r + 1) * k] for r in range(count)]

    masked = slots_of(eng.member_challenges_t(None, sim_t, index_t, 0))
    split = slots_of(eng.member_challenges_t(e_t, sim_t, index_t, 1))
    assert masked == mm.challenges(0, e, sims, index) and split == mm.challenges(1, e, sims, index)
    for r in range(count):
        i = index[r]
        assert masked[r][i] == 0 and all(masked[r][j] == sims[r][j] == split[r][j] for j in range(k) if j != i)
        assert sum(split[r]) & M128 == e[r] and 0 <= split[r][i] <= M128
    # what the directed rows are for, written out: all-ones sims and e = 0 leave k - 1 in the real slot; e = 2^128 - 1 over zero sims itself
    assert split[0][index[0]] == k - 1 and split[1][index[1]] == k - 2 and split[4][index[4]] == M128 and split[5][index[5]] == 0
    split_t = eng.member_challenges_t(e_t, sim_t, index_t, 1)
    assert list(eng.member_challenges_t(e_t, split_t, None, 2)) == [0] * count == mm.challenges(2, e, split, index)
    for word in range(4):
        spoiled = eng.to_host(split_t).copy()
        spoiled[3, 4 * (k - 1) + word] ^= 1 << 31
        assert list(eng.member_challenges_t(e_t, eng.to_device(spoiled), None, 2)) == [0, 0, 0, 1] + [0] * (count - 4)
    for bad in (lambda: eng.member_challenges_t(e_t, sim_t, index_t, 3), lambda: eng.member_challenges_t(e_t, sim_t[:, :4], index_t, 1),
                lambda: eng.member_challenges_t(e_t, sim_t, index_t + k, 1), lambda: eng.member_challenges_t(e_t[:1], sim_t, index_t, 2)):
        with pytest.raises(ValueError):
            bad()


def test_every_refusal_happens_without_an_engine_call():
    eng = MemberEngine()
    values = [0, 1]
    index, msgs, rands, cts = mc.statements(N1K, values, 2)
    empty = membership.prove_batch(N1K, values, [], [], mc.LABEL, engine=eng)
    assert len(empty) == 0 and membership.verify_batch(N1K, values, [], empty, mc.LABEL, engine=eng) == []
    assert membership.encrypt_with_proof(N1K, values, [], mc.LABEL, engine=eng)[0] == []
    good = membership.prove_batch(N1K, values, msgs, rands, mc.LABEL, rng=DeviceRng(key=mc.KEY), ciphertexts=cts, engine=eng)
    eng.calls.clear()
    n259 = (1 << 258) | 1
    assert n259.bit_length() == 259
    for bad in (lambda: membership.prove_batch(N1K, [0], [0, 0], rands, mc.LABEL, engine=eng),                       # k = 1
                lambda: membership.prove_batch(N1K, list(range(17)), msgs, rands, mc.LABEL, engine=eng),           # k = 17
                lambda: membership.prove_batch(N1K, [0, 1, 1], msgs, rands, mc.LABEL, engine=eng),                 # a duplicate
                lambda: membership.prove_batch(N1K, [0, N1K], [0, 0], rands, mc.LABEL, engine=eng),                # s_j >= N
                lambda: membership.prove_batch(N1K, [0, -1], [0, 0], rands, mc.LABEL, engine=eng),
                lambda: membership.prove_batch(N128, values, msgs, rands, mc.LABEL, engine=eng),                   # bits(N) < 260
                lambda: membership.prove_batch(n259, values, msgs, rands, mc.LABEL, engine=eng),
                lambda: membership.prove_batch(N1K - 1, values, msgs, rands, mc.LABEL, engine=eng),                # an even N
                lambda: membership.prove_batch(N1K, values, [0, 2], rands, mc.LABEL, engine=eng),                  # a message outside S
                lambda: membership.prove_batch(N1K, values, msgs, rands[:1], mc.LABEL, engine=eng),
                lambda: membership.prove_batch(N1K, values, msgs, rands, mc.LABEL, ciphertexts=cts[:1], engine=eng),
                lambda: membership.prove_batch(N1K, values, msgs, rands, "a str label", engine=eng),
                lambda: membership.encrypt_with_proof(N1K, values, [2], mc.LABEL, engine=eng),
                lambda: membership.encrypt_with_proof(N128, values, [0], mc.LABEL, engine=eng),
                lambda: membership.verify_batch(N128, values, cts, good, mc.LABEL, engine=eng),
                lambda: membership.verify_batch(N1K, values, cts[:1], good, mc.LABEL, engine=eng),
                lambda: membership.verify_batch(N1K, [0, 1, 2], cts, good, mc.LABEL, engine=eng),                  # proofs over another k
                lambda: membership.verify_batch(N1K, [0], cts, good, mc.LABEL, engine=eng),
                lambda: membership.MembershipProofs.from_ints([[1, 1]], [[1, 1]], [], N1K, 2),
                lambda: membership.MembershipProofs.from_ints([[1]], [[1]], [[1]], N1K, 1),
                lambda: slots.one_hot_values(N128, 16, 8), lambda: slots.one_hot_values(N128, 16, 0)):
        with pytest.raises(ValueError):
            bad()
    assert eng.calls == []
    assert membership.shape((1 << 259) | 1, 2)["draw_bits"] == 260 + 64          # the shortest modulus the module takes
    assert slots.one_hot_values(N128, 16, 7) == [1 << (16 * j) for j in range(7)]


def test_encrypt_with_proof_round_trip():
    eng = MemberEngine()
    values = slots.one_hot_values(N1K, 16, 4)
    msgs = [values[3], values[0], values[2]]
    cts, proofs = membership.encrypt_with_proof(N1K, values, msgs, mc.LABEL, rng=DeviceRng(key=mc.KEY, first_call=1), engine=eng)
    assert membership.verify_batch(N1K, values, cts, proofs, mc.LABEL, engine=eng) == [True] * 3
    cols = proofs.to_ints()
    assert all(mm.verify(N1K, values, mc.LABEL, c, row_of(cols, r)) for r, c in enumerate(cts))
    two_votes = cts[1] * (1 + values[1] * N1K) % (N1K * N1K)                     # 2^0 + 2^16: no member of the list
    assert membership.verify_batch(N1K, values, [cts[0], two_votes, cts[2]], proofs, mc.LABEL, engine=eng) == [True, False, True]


def test_the_header_declares_what_the_library_exports():
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    header = (mc.HERE.parent / "include" / "mxpaillier.h").read_text()
    for name in ("mx_member_challenges", "MX_MEMBER_MASK", "MX_MEMBER_SPLIT", "MX_MEMBER_SUM", "MX_MEMBER_MIN_K", "MX_MEMBER_MAX_K"):
        assert name in header
    assert hasattr(lib, "mx_member_challenges") and "mx_member_challenges" in _lib.SYMBOLS
    assert (_lib.MX_MEMBER_MASK, _lib.MX_MEMBER_SPLIT, _lib.MX_MEMBER_SUM, _lib.MX_MEMBER_MIN_K, _lib.MX_MEMBER_MAX_K) == (0, 1, 2, 2, 16)
    # the refusals need no GPU: they come back before anything is launched
    for args in ((None, None, None, None, None, 2, 1, 0), (None, 8, 8, 8, None, 2, 1, 1), (8, 8, None, None, None, 2, 1, 2),
                 (8, 8, 8, 8, 8, 1, 1, 0), (8, 8, 8, 8, 8, 17, 1, 1), (8, 8, 8, 8, 8, 2, -1, 2), (8, 8, 8, 8, 8, 2, 1, 3), (8, 8, 8, 8, 8, 2, 1, -1),
                 (8, 8, None, 8, 8, 2, 1, 0), (8, 8, 8, None, 8, 2, 1, 1)):
        assert lib.mx_member_challenges(*args, None) == -1, args
    assert lib.mx_member_challenges(8, 8, 8, 8, 8, 2, (256 << 31) + 1, 0, None) == -2
    assert lib.mx_member_challenges(8, 8, 8, 8, 8, 2, 0, 0, None) == 0          # a count of 0: nothing to launch
    assert lib.mx_version() == 404
