"""The challenge kernel of the one-of-k membership proofs (csrc/mx_member.hpp) and the proofs over it on the GPU —
Engine.member_challenges_t / member_prove_t / member_verify_t and membership.py — bit for bit against Python ints and
tools/member_model.py.

The engine entries take any N the N^2 kernels take, so the row-by-row comparison runs at the 128-bit golden key (the
module itself refuses moduli below 260 bits); the end-to-end cases run at 1024 and 2048 bits."""

from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

import member_cases as mc  # noqa: E402
from member_cases import mm  # noqa: E402
from member_engine import forgeries, tamperings  # noqa: E402

N128 = mc.modulus(128)
M128 = mc.M128


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def rows_of(eng, values, width, per_row=1):
    from protocols.distributed_keygen_amd import limbs

    return eng.to_device(limbs.pack(values, width).reshape(len(values) // per_row, width * per_row))


def slots_of(eng, rows_t, k):
    from protocols.distributed_keygen_amd import limbs

    flat = limbs.unpack(eng.to_host(rows_t.contiguous().view(rows_t.shape[0] * k, -1)))
    return [flat[r * k : (r + 1) * k] for r in range(rows_t.shape[0])]


# ------------------------------------------------------------------ the challenge kernel
@pytest.mark.parametrize("k", [2, 3, 16])
def test_member_challenges_equal_python_ints(eng, k):
    import torch

    directed = mc.directed_challenges(k)
    for count in (1, 63, 64, 65, 257):
        e, sims, index = mc.random_challenges(k, count, 1000 * k + count)
        if count == 257:                                      # the directed carries and borrows, in rows of several workgroups' launch
            for r, row in enumerate(zip(*directed)):
                e[r * 3 % count], sims[r * 3 % count], index[r * 3 % count] = row
        e_t = rows_of(eng, e, 4)
        sim_t = rows_of(eng, [v for row in sims for v in row], 4, k)
        index_t = torch.tensor(index, dtype=torch.int32, device=eng.device)
        masked_t = eng.member_challenges_t(None, sim_t, index_t, 0)
        split_t = eng.member_challenges_t(e_t, sim_t, index_t, 1)
        masked, split = slots_of(eng, masked_t, k), slots_of(eng, split_t, k)
        assert masked == mm.challenges(0, e, sims, index) and split == mm.challenges(1, e, sims, index), count
        assert slots_of(eng, sim_t, k) == sims                                       # the inputs are left as they were
        for r in range(count):                                                       # mode 0 leaves every other slot bit-identical
            assert masked[r][index[r]] == 0 and all(masked[r][j] == sims[r][j] for j in range(k) if j != index[r])
            assert sum(split[r]) & M128 == e[r]
        # in place: out is sim
        mine_t = sim_t.clone()
        assert eng.member_challenges_t(e_t, mine_t, index_t, 1, out_t=mine_t) is mine_t and slots_of(eng, mine_t, k) == split
        mine_t = sim_t.clone()
        eng.member_challenges_t(None, mine_t, index_t, 0, out_t=mine_t)
        assert slots_of(eng, mine_t, k) == masked
        # mode 2: clean on the split rows, 1 on the random ones, and exactly the rows where one word of one e_j was changed
        assert [int(s) for s in eng.member_challenges_t(e_t, split_t, None, 2).cpu()] == [0] * count
        assert [int(s) for s in eng.member_challenges_t(e_t, sim_t, None, 2).cpu()] == mm.challenges(2, e, sims, index)
        for word in range(4):
            spoiled_t = split_t.clone()
            hit = sorted({(7 * word + 3) % count, count - 1, (count // 2 + word) % count})
            for r in hit:
                spoiled_t[r, 4 * ((r + word) % k) + word] ^= 1 << (5 + word)
            assert [int(s) for s in eng.member_challenges_t(e_t, spoiled_t, None, 2).cpu()] == [int(r in hit) for r in range(count)], (count, word)


def test_member_challenges_refusals_launch_nothing(eng):
    import torch

    k = 3
    e, sims, index = mc.random_challenges(k, 4, 9)
    e_t, sim_t = rows_of(eng, e, 4), rows_of(eng, [v for row in sims for v in row], 4, k)
    index_t = torch.tensor(index, dtype=torch.int32, device=eng.device)
    out_t = torch.zeros_like(sim_t)
    st = torch.full((4,), 7, dtype=torch.uint8, device=eng.device)
    for bad in (lambda: eng.member_challenges_t(e_t, sim_t, index_t, 3),
                lambda: eng.member_challenges_t(e_t, sim_t[:, :4].contiguous(), index_t, 1),                  # k = 1
                lambda: eng.member_challenges_t(e_t, torch.cat([sim_t] * 6, dim=1).contiguous(), index_t, 1),   # k = 18
                lambda: eng.member_challenges_t(e_t, sim_t[:, :11].contiguous(), index_t, 1),                 # no multiple of four words
                lambda: eng.member_challenges_t(e_t[:2].contiguous(), sim_t, index_t, 1),
                lambda: eng.member_challenges_t(None, sim_t, index_t, 2),
                lambda: eng.member_challenges_t(e_t, sim_t, index_t.to(torch.int64), 1),
                lambda: eng.member_challenges_t(e_t, sim_t, index_t[:3].contiguous(), 0),
                lambda: eng.member_challenges_t(e_t, sim_t, index_t + k, 1),                                  # an index outside [0, k)
                lambda: eng.member_challenges_t(e_t, sim_t, index_t - k, 0),
                lambda: eng.member_challenges_t(e_t, sim_t, None, 1),
                lambda: eng.member_challenges_t(e_t, sim_t, index_t, 1, out_t=out_t[:2].contiguous())):
        with pytest.raises(ValueError):
            bad()
    empty_t = eng.member_challenges_t(e_t[:0].contiguous(), sim_t[:0].contiguous(), index_t[:0].contiguous(), 1)
    assert tuple(empty_t.shape) == (0, 4 * k) and tuple(eng.member_challenges_t(e_t[:0].contiguous(), sim_t[:0].contiguous(), None, 2).shape) == (0,)
    # the C entry itself: bad arguments come back as a status, before anything is launched
    lib = eng.lib
    good = [e_t.data_ptr(), sim_t.data_ptr(), index_t.data_ptr(), out_t.data_ptr(), st.data_ptr(), k, 4, 1, None]
    names = ("e", "sim", "index", "out", "status", "k", "count", "mode", "stream")

    def run(**change):
        args = list(good)
        for key, v in change.items():
            args[names.index(key)] = v
        return lib.mx_member_challenges(*args)

    for change in (dict(e=None), dict(sim=None), dict(index=None), dict(out=None), dict(mode=2, status=None), dict(mode=0, sim=None),
                   dict(mode=0, index=None), dict(k=1), dict(k=17), dict(k=0), dict(count=-1), dict(mode=3), dict(mode=-1)):
        assert run(**change) == -1, change
    assert run(count=(256 << 31) + 1) == -2
    assert run(count=0) == 0
    eng.synchronize()
    assert not bool(out_t.any()) and [int(s) for s in st.cpu()] == [7] * 4 and slots_of(eng, sim_t, k) == sims


# ------------------------------------------------------------------ the proofs
def verdicts(eng, n, values, cts, a, e, z, label):
    """membership.verify_batch without the module's refusal of short moduli: received ints -> rows -> member_verify_t."""
    from protocols.distributed_keygen_amd import membership

    k = len(values)
    proofs = membership.MembershipProofs.from_ints(a, e, z, n, k)
    c_rows, c_fit = membership._rows_of(cts, membership.shape(n, k)["limbs2"])
    got = eng.member_verify_t(eng.to_device(c_rows), *(eng.to_device(t) for t in proofs.rows()), n, values, membership.context(n, values, label))
    return [bool(g) and f and not u for g, f, u in zip(got.cpu(), c_fit, proofs.unfit)]


@pytest.mark.parametrize("name", ["bit", "one_hot"])
def test_proofs_at_the_smallest_key_equal_the_model_row_for_row(eng, name):
    import torch

    from protocols.distributed_keygen_amd import DeviceRng, membership

    values = mc.value_sets(N128)[name]
    k, count = len(values), 65
    sh = eng.member_shape(N128, k)
    index, msgs, rands, cts = mc.statements(N128, values, count)
    assert set(index) == set(range(k))                                               # every slot is the real one somewhere
    ctx = membership.context(N128, values, mc.LABEL)
    assert ctx == mm.context(N128, values, mc.LABEL) and sh == mm.shape(N128, k) == membership.shape(N128, k)
    cts_t = rows_of(eng, cts, sh["limbs2"])
    index_t = torch.tensor(index, dtype=torch.int32, device=eng.device)
    rows = eng.member_prove_t(cts_t, index_t, rows_of(eng, rands, sh["limbs_n"]), N128, values, ctx, rng=DeviceRng(key=mc.KEY, first_call=40))
    assert [tuple(t.shape) for t in rows] == [(count, k * sh["limbs2"]), (count, 4 * k), (count, k * sh["limbs_n"])]
    got = membership.MembershipProofs(*rows, k).to_ints()
    want = mc.model_proofs(N128, values, mc.LABEL, index, rands, 40)
    for field, g, w in zip(membership.MembershipProofs.FIELDS, got, want):
        assert g == w, field
    assert [bool(v) for v in eng.member_verify_t(cts_t, *rows, N128, values, ctx).cpu()] == [True] * count
    # verdicts per row: every tampering spoils row 1 of the first three rows and nothing else
    ints = tuple([list(r) for r in col[:3]] for col in got)
    for what, tcts, a, e, z in tamperings(N128, values, ints, cts[:3]):
        assert verdicts(eng, N128, values, tcts, a, e, z, mc.LABEL) == [True, False, True], what
    # the forgeries that need no witness, for a ciphertext of a value outside the list: zero satisfies every equation
    outside = mm.encrypt(N128, max(values) + 1, rands[1])
    for what, forged in forgeries(N128, values, mc.LABEL, outside):
        a, e, z = ([ints[j][0], forged[j], ints[j][2]] for j in range(3))
        assert verdicts(eng, N128, values, [cts[0], outside, cts[2]], a, e, z, mc.LABEL) == [True, False, True], what
        assert not mm.verify(N128, values, mc.LABEL, outside, forged), what
    assert verdicts(eng, N128, values, cts[:3], *ints, b"another session") == [False] * 3
    assert verdicts(eng, N128, values[1:] + values[:1], cts[:3], *ints, mc.LABEL) == [False] * 3
    assert verdicts(eng, N128 + 2, values, cts[:3], *ints, mc.LABEL) == [False] * 3
    with pytest.raises(ValueError):                                                  # the engine reads the index for its range
        eng.member_prove_t(cts_t, index_t + k, rows_of(eng, rands, sh["limbs_n"]), N128, values, ctx, rng=DeviceRng())
    with pytest.raises(ValueError):                                                  # and the module refuses a modulus this short
        membership.prove_batch(N128, values, msgs, rands, mc.LABEL, engine=eng)


@pytest.mark.parametrize("key_length", [1024, 2048])
def test_end_to_end_with_one_cheating_row(eng, key_length):
    from protocols.distributed_keygen_amd import DeviceRng, membership

    n = mc.modulus(key_length)
    values = mc.value_sets(n)["signed"]                                              # k = 3: 0, 1 and -1
    msgs = [values[r % 3] for r in range(8)]
    cts, proofs = membership.encrypt_with_proof(n, values, msgs, mc.LABEL, rng=DeviceRng(key=mc.KEY, first_call=5), engine=eng)
    assert membership.verify_batch(n, values, cts, proofs, mc.LABEL, engine=eng) == [True] * 8
    cols = proofs.to_ints()
    assert mm.verify(n, values, mc.LABEL, cts[4], [col[4] for col in cols])         # the model accepts one of the engine's proofs
    cheat = list(cts)
    cheat[5] = cts[5] * (1 + 2 * n) % (n * n)                                        # -1 + 2 = 1 is in the list; the proof is not for it
    cheat[6] = cts[6] * (1 + 5 * n) % (n * n)                                        # 0 + 5: no member of the list
    received = membership.MembershipProofs.from_ints(*cols, n, 3)
    assert membership.verify_batch(n, values, cheat, received, mc.LABEL, engine=eng) == [True] * 5 + [False, False, True]
    assert membership.verify_batch(n, values, cts, received, b"another session", engine=eng) == [False] * 8
