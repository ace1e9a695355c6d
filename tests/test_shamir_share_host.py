"""Host side of the device sharing of the prime candidates (no GPU): the model tools/share_model.py against a second,
straightforward implementation; the draw-order contract of shamir.generate_pq_batch on a model-backed engine double
(tests/share_engine.py); and ``patch.install(share_rng=...)`` on the real reference modules, where build() has copied
them into oracle/_ref."""

from __future__ import annotations

import asyncio
import json
import random
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import chacha_model as cm  # noqa: E402
import share_model as sm  # noqa: E402
from share_engine import ShareEngine  # noqa: E402

from protocols.distributed_keygen_amd import shamir  # noqa: E402
from protocols.distributed_keygen_amd.device_rng import DeviceRng  # noqa: E402

KEY = bytes(range(7, 39))
FIXTURES = json.loads((ROOT / "tests" / "golden" / "reconstruct.json").read_text())


def fixture_primes():
    return {label: int(case["prime"], 16) for label, case in FIXTURES.items()}


# ------------------------------------------------------------------ the model against a second implementation
def naive_share(secret, draws, prime, x):
    """The definition, term by term: s + sum_k (D_k mod P) x^k mod P."""
    total = secret
    for k, d in enumerate(draws, start=1):
        total += (d - (d // prime) * prime) * x**k
    return total - (total // prime) * prime


@pytest.mark.parametrize("label", sorted(FIXTURES))
def test_model_shares_equal_the_definition_term_by_term(label):
    prime = fixture_primes()[label]
    rng = random.Random(label)
    bits = sm.coefficient_bits(prime)
    assert bits == prime.bit_length() + 64 and sm.coefficient_words(prime) == (bits + 31) // 32
    for degree, points in ((1, [1, 2, 3]), (2, [1, 2, 3, 4, 5]), (4, [2, 5, 9, 65535, 7])):
        secrets = [0, prime - 1] + [rng.randrange(prime) for _ in range(3)]
        edge = [0, prime - 1, prime, prime + 1, (1 << bits) - 1]
        draws = [[rng.getrandbits(bits) for _ in secrets] for _ in range(degree)]
        draws[0][:5] = edge
        draws[-1][:5] = edge[::-1] if degree > 1 else edge
        got = sm.shamir_share(secrets, draws, prime, points)
        assert len(got) == len(points) and all(len(col) == len(secrets) for col in got)
        for j, x in enumerate(points):
            for e, s in enumerate(secrets):
                assert got[j][e] == naive_share(s, [draws[k][e] for k in range(degree)], prime, x)
                assert 0 <= got[j][e] < prime
        assert sm.shamir_share(None, draws, prime, points) == sm.shamir_share([0] * len(secrets), draws, prime, points)


def test_model_shares_reconstruct_the_secret_and_have_the_degree_asked_for():
    prime = fixture_primes()["k128_n5_t2"]
    rng = random.Random(5)
    secrets = [rng.randrange(prime) for _ in range(4)]
    draws = [[rng.getrandbits(sm.coefficient_bits(prime)) for _ in secrets] for _ in range(2)]
    points = [1, 2, 3, 4]
    cols = sm.shamir_share(secrets, draws, prime, points)
    for subset in ([0, 1, 2], [1, 2, 3], [0, 2, 3]):
        pts = [points[i] for i in subset]
        lam = shamir.lagrange_coefficients_at_zero(pts, prime)
        assert [sum(l * cols[i][e] for l, i in zip(lam, subset)) % prime for e in range(4)] == secrets


@pytest.mark.parametrize("prime_length", [8, 32, 35, 64, 67])
def test_model_candidates_have_the_length_and_the_residue_of_the_reference(prime_length):
    rows = cm.rows(KEY, 3, 20, prime_length - 3)
    for first in (True, False):
        got = sm.candidates(rows, prime_length, first)
        for row, c in zip(rows, got):
            r = sm.row_int(row)
            assert c == int("1" + format(r, f"0{prime_length - 3}b") + ("11" if first else "00"), 2)      # DK:874-875 as a bit string
            assert c.bit_length() == prime_length and c % 4 == (3 if first else 0)
    with pytest.raises(ValueError):
        sm.candidate(1 << (prime_length - 3), prime_length, True)
    with pytest.raises(ValueError):
        sm.candidate(0, 7, True)


# ------------------------------------------------------------------ generate_pq_batch: draw order and refusals
@pytest.mark.parametrize("index,label,batch,first_call", [(1, "k128_n5_t2", 3, 0), (4, "k128_n5_t2", 2, 1 << 40), (2, "k64_n3_t1", 5, 9)])
def test_generate_pq_batch_draws_in_the_documented_order(index, label, batch, first_call):
    case = FIXTURES[label]
    prime, n, t, length = int(case["prime"], 16), case["n_parties"], case["t"], case["key_length"] // 2
    eng, rng = ShareEngine(), DeviceRng(key=KEY, first_call=first_call)
    p_add, q_add, shares = shamir.generate_pq_batch(index, length, prime, n, t, batch, rng, engine=eng)
    assert rng.next_call == first_call + 5
    bits, cw, rw = sm.coefficient_bits(prime), sm.coefficient_words(prime), (length - 3 + 31) // 32
    limbs = (prime.bit_length() + 31) // 32
    points = tuple(range(1, n + 1))
    assert eng.share_calls == [
        ("chacha", first_call, batch, length - 3, rw), ("candidates", batch, length, index == 1, limbs),
        ("chacha", first_call + 1, batch, length - 3, rw), ("candidates", batch, length, index == 1, limbs),
        ("chacha", first_call + 2, t * batch, bits, cw), ("share", True, t, points, batch),
        ("chacha", first_call + 3, t * batch, bits, cw), ("share", True, t, points, batch),
        ("chacha", first_call + 4, 2 * t * batch, bits, cw), ("share", False, 2 * t, points, batch),
    ]
    assert (p_add, q_add, shares) == sm.generate_pq(KEY, first_call, index, length, prime, n, t, batch)
    assert all(v.bit_length() == length and v % 4 == (3 if index == 1 else 0) for v in p_add + q_add)
    assert sorted(shares) == ["p", "q", "zero"] and all(sorted(col) == list(points) for col in shares.values())
    # the shares are sharings of what was returned: degree t for p and q, 2t for zero
    for name, secrets, degree in (("p", p_add, t), ("q", q_add, t), ("zero", [0] * batch, 2 * t)):
        pts = list(points)[-(degree + 1):]
        lam = shamir.lagrange_coefficients_at_zero(pts, prime)
        assert [sum(l * shares[name][x][e] for l, x in zip(lam, pts)) % prime for e in range(batch)] == secrets
    # sums of received shares (DK:840-847) through the existing linear combination
    assert shamir.sum_shares_batch([shares["p"][x] for x in points], prime, engine=eng) == [
        sum(shares["p"][x][e] for x in points) % prime for e in range(batch)]


def test_generate_pq_batch_refuses_before_it_draws():
    prime = fixture_primes()["k128_n5_t2"]
    eng, rng = ShareEngine(), DeviceRng(key=KEY, first_call=11)
    bad = [
        dict(index=0), dict(index=6), dict(prime_length=7), dict(prime=prime + 1), dict(t=0), dict(t=3),      # 2t + 1 > 5 points
        dict(prime_length=prime.bit_length()), dict(batch_size=-1), dict(rng=None),
    ]
    for change in bad:
        args = dict(index=1, prime_length=64, prime=prime, n_parties=5, t=2, batch_size=3, rng=rng)
        args.update(change)
        with pytest.raises(ValueError):
            shamir.generate_pq_batch(engine=eng, **args)
    assert rng.next_call == 11 and eng.share_calls == []
    for points in ([1, 1, 2], [0, 1, 2], [1, 2, 1 << 16], [1, 2.0, 3], [1, 2]):
        with pytest.raises(ValueError):
            shamir.check_share_args(prime, 2, points)
    assert shamir.check_share_args(prime, 2, (3, 1, 65535)) == [3, 1, 65535]
    with pytest.raises(ValueError):
        shamir.check_share_args(prime, shamir.MAX_SHARE_DEGREE + 1, list(range(1, 40)))


def test_the_module_docstring_says_what_is_drawn():
    doc = " ".join(shamir.__doc__.split())
    assert "bias below 2^-64" in doc and "DETERMINISTIC EXPANSION" in doc and "device_rng" in doc and "Opt-in" in doc


# ------------------------------------------------------------------ patch.install(share_rng=...) on the real reference
REF = ROOT / "oracle" / "_ref" / "distributed_keygen"
NO_REF = "the reference modules are not in oracle/_ref (build() copies them where a checkout of the reference exists)"


@pytest.fixture(scope="module")
def ref():
    if not REF.exists():
        pytest.skip(NO_REF)
    import make_golden

    # a second load_reference() in one process would put new stand-in classes under the names the loaded reference has
    # bound already (tests/test_patch_reference.py builds its ciphertexts from them): load once per process
    dk = sys.modules.get("tno.mpc.protocols.distributed_keygen.distributed_keygen")
    if dk is None:
        _, dk = make_golden.load_reference()
    return dk, make_golden


def _round(dk, mg, batch, label):
    """Three in-process parties: _generate_pq, p * q + zero, exchange_reconstruct, reconstruct() (DK:1262-1284)."""
    DP = dk.DistributedPaillier
    names = ["p1", "p2", "p3"]
    hub = mg._Hub(names)
    record = {}

    async def party(i, me):
        pool = mg._MemPool(hub, me)
        party_indices = {("self" if n == me else n): k for k, n in enumerate(names, start=1)}
        _, prime_length, _, sh_t, sh_2t, _ = DP.setup_input(pool, 64, 200, 1)
        p_sh, q_sh, zero, p_add, q_add = await DP._generate_pq(
            pool, i, prime_length, party_indices, sh_t, sh_2t, 99, batch_size=batch, msg_id=f"pq_{label}")
        held = {name: [sorted(v.get_shares()) for v in var.variables] for name, var in (("p", p_sh), ("q", q_sh), ("zero", zero))}
        labels = [(var.label, var.owner, var.batch_size) for var in (p_sh, q_sh, zero)]
        candidate_n = p_sh * q_sh
        candidate_n += zero
        await dk.exchange_reconstruct(candidate_n, i, pool, party_indices, msg_id=f"n_{label}")
        record[i] = dict(moduli=candidate_n.reconstruct(), p=[int(v) for v in p_add], q=[int(v) for v in q_add],
                         held=held, labels=labels, prime=sh_t.modulus, prime_length=prime_length)

    async def run():
        await asyncio.gather(*[party(i, me) for i, me in enumerate(names, start=1)])

    asyncio.run(run())
    return record


def test_patched_generate_pq_is_a_drop_in_on_the_reference(ref):
    dk, mg = ref
    from protocols.distributed_keygen_amd import patch

    DP = dk.DistributedPaillier
    original = DP.__dict__["_generate_pq"]
    base = _round(dk, mg, 4, "reference")                     # the reference alone: the shape to reproduce

    eng, rng = ShareEngine(), DeviceRng(key=KEY, first_call=100)
    patch.install(engine=eng, share_rng=rng)
    try:
        assert DP.__dict__["_generate_pq"] is not original
        got = _round(dk, mg, 4, "patched")
    finally:
        patch.uninstall()
    assert DP.__dict__["_generate_pq"] is original

    assert rng.next_call == 100 + 3 * 5                       # three parties, five draws each
    assert [c[0] for c in eng.share_calls].count("share") == 9 and [c[0] for c in eng.share_calls].count("candidates") == 6
    length = got[1]["prime_length"]
    for i in (1, 2, 3):
        # every party reconstructed the product of the summed additive shares
        assert got[i]["moduli"] == [sum(got[j]["p"][k] for j in got) * sum(got[j]["q"][k] for j in got) for k in range(4)]
        assert all(v.bit_length() == length and v % 4 == (3 if i == 1 else 0) for v in got[i]["p"] + got[i]["q"])
        # the sums hold this party's share only, as in the reference; labels, owners and batch size are the reference's
        assert got[i]["held"] == base[i]["held"] == {name: [[i]] * 4 for name in ("p", "q", "zero")}
        assert got[i]["labels"] == base[i]["labels"]
    assert got[1]["prime"] == base[1]["prime"]


def test_the_reference_surface_the_share_path_relies_on(ref):
    """What the rebound `_generate_pq` takes from the reference besides the names tests/test_standin_drift.py lists:
    ``utils.exchange_shares`` with the call shape used, the containers' ``set_plaintexts`` / ``set_share`` and the
    ``_index`` that ``ShamirVariable.share`` leaves (utils.py:259-260); a package without them is refused whole."""
    import inspect
    import types

    dk, _ = ref
    from protocols.distributed_keygen_amd import patch

    utils = sys.modules["tno.mpc.protocols.distributed_keygen.utils"]
    assert dk.exchange_shares is utils.exchange_shares and dk.ShamirVariable is utils.ShamirVariable
    assert list(inspect.signature(utils.exchange_shares).parameters) == ["group", "index", "pool", "party_indices", "msg_id"]
    assert list(inspect.signature(utils.ShamirVariable.__init__).parameters) == ["self", "shamir", "label", "owner"]
    assert hasattr(utils.Batched, "set_plaintexts") and hasattr(utils.Batched, "set_share")
    scheme = sys.modules["tno.mpc.encryption_schemes.shamir"].ShamirSecretSharingScheme(101, 3, 1)
    assert utils.ShamirVariable(shamir=scheme, label="p_1", owner=1)._index == -1
    for name in ("modulus", "number_of_parties", "polynomial_degree"):
        assert hasattr(scheme, name)
    original = dk.DistributedPaillier.__dict__["_generate_pq"]
    sys.modules["no_utils_pkg"] = types.ModuleType("no_utils_pkg")
    sys.modules["no_utils_pkg"].__path__ = []
    for sub in ("paillier_shared_key", "distributed_keygen"):
        sys.modules["no_utils_pkg." + sub] = sys.modules["tno.mpc.protocols.distributed_keygen." + sub]
    try:
        with pytest.raises(ValueError):
            patch.install(engine=ShareEngine(), package="no_utils_pkg", share_rng=DeviceRng(key=KEY))
        assert dk.DistributedPaillier.__dict__["_generate_pq"] is original and not patch._saved
    finally:
        for name in [m for m in sys.modules if m.startswith("no_utils_pkg")]:
            del sys.modules[name]


def test_install_without_share_rng_leaves_generate_pq_alone(ref):
    dk, _ = ref
    from protocols.distributed_keygen_amd import patch

    original = dk.DistributedPaillier.__dict__["_generate_pq"]
    patch.install(engine=ShareEngine())
    try:
        assert dk.DistributedPaillier.__dict__["_generate_pq"] is original
    finally:
        patch.uninstall()
