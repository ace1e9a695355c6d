"""Host logic of the dealt threshold key (threshold.py) over the Python-int double of the engine (proof_engine.py),
bit-exact against the model (tools/proof_model.py).  No GPU."""

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
sys.path.insert(0, str(Path(__file__).resolve().parent))

import proof_model as pm  # noqa: E402
from crt_engine import MARKERS  # noqa: E402
from proof_engine import ProofEngine, tamperings  # noqa: E402

from protocols.distributed_keygen_amd import limbs, threshold  # noqa: E402
from protocols.distributed_keygen_amd.device_rng import DeviceRng  # noqa: E402
from protocols.distributed_keygen_amd.private_key import PaillierPrivateKey  # noqa: E402

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "threshold_keys.json").read_text())
P128, Q128 = (int(GOLDEN["keys"]["128"][k], 16) for k in "pq")
P32, Q32 = 65267, 65147            # 16-bit safe primes: N has 32 bits, rows of z need three pieces
KEY = bytes(range(32))


def dealt(p, q, parties, degree, seed=1):
    eng = ProofEngine()
    key = PaillierPrivateKey(p, q, engine=eng)
    pub, shares = threshold.deal(key, parties, degree, rng=random.Random(seed), check=False, engine=eng)
    mpub, mshares = pm.deal(p, q, parties, degree, random.Random(seed))
    return eng, pub, shares, mpub, mshares


def ciphertexts(n, count, seed=5):
    rnd = random.Random(seed)
    msgs = [0, 1, n - 1][:count] + [rnd.randrange(n) for _ in range(max(0, count - 3))]
    return msgs, [pm.encrypt(n, m, rnd.randrange(1, n)) for m in msgs]


def rho_rows(pub, count, call=3):
    """The rows a DeviceRng(KEY, first_call=call) draws, and the same as ints."""
    sys.path.insert(0, str(ROOT / "tools"))
    import chacha_model

    return chacha_model.row_ints(KEY, call, count, pub.rho_bits, pub.z_words)


def test_the_golden_primes_are_distinct_safe_primes_of_the_recorded_seed():
    assert GOLDEN["seed"] == 20261020
    for kl in (128, 1024, 2048):
        p, q = (int(GOLDEN["keys"][str(kl)][k], 16) for k in "pq")
        assert p != q and (p * q).bit_length() == kl
        for x in (p, q, (p - 1) // 2, (q - 1) // 2):
            assert pow(2, x - 1, x) == 1 and pow(3, x - 1, x) == 1
    assert pm.golden_keys(GOLDEN["seed"], (128,))["keys"]["128"] == GOLDEN["keys"]["128"]


@pytest.mark.parametrize("parties,degree", [(2, 1), (3, 1), (5, 2), (5, 4)])
def test_deal_partials_and_combination_equal_the_model(parties, degree):
    eng, pub, shares, mpub, mshares = dealt(P128, Q128, parties, degree)
    assert (pub.n, pub.v, pub.verification_keys, pub.x_bits, pub.theta_inv) == (mpub.n, mpub.v, mpub.vks, mpub.x_bits, mpub.theta_inv)
    assert [s.x for s in shares] == [s.x for s in mshares] and [s.index for s in shares] == list(range(1, parties + 1))
    assert (pub.pieces, pub.kw, pub.z_words, pub.rho_bits, pub.z_bits) == (mpub.pieces, mpub.kw, mpub.z_words, mpub.rho_bits, mpub.z_bits)
    msgs, cts = ciphertexts(pub.n, 4)
    cols = {s.index: s.partial_decrypt_batch(cts) for s in shares}
    for s, ms in zip(shares, mshares):
        assert cols[s.index] == [pm.partial(mpub, ms, c) for c in cts]
    subsets = list(itertools.combinations(range(1, parties + 1), degree + 1))
    if (parties, degree) != (5, 2):
        subsets = subsets[:1] + subsets[-1:]
    negative = 0
    for sub in subsets:
        negative += any(lam < 0 for lam in threshold.lagrange(pub.delta, sub).values())
        assert threshold.lagrange(pub.delta, sub) == pm.lagrange(mpub.delta, sub)
        assert pub.combine_batch({i: cols[i] for i in sub}) == msgs
    if (parties, degree) == (5, 2):
        assert negative >= 5 and len(subsets) == 10
        # more than t + 1 columns: the lowest t + 1 indices are used
        assert pub.combine_batch(cols) == msgs


def test_the_results_have_combine_ts_format():
    eng, pub, shares, _, _ = dealt(P128, Q128, 3, 1)
    msgs, cts = ciphertexts(pub.n, 3)
    cts_t = eng.to_device(limbs.pack(cts, pub.limbs2))
    rows, status = pub.combine_t({s.index: s.partial_decrypt_t(cts_t) for s in shares[1:]})
    assert rows.shape == (3, limbs.limbs_for(pub.n)) and status.dtype == np.uint8 and not status.any()
    assert limbs.unpack(rows) == msgs


@pytest.mark.parametrize("p,q,pieces", [(P128, Q128, 2), (P32, Q32, 3)])
def test_piece_split_and_proofs_equal_the_model(p, q, pieces):
    eng, pub, shares, mpub, mshares = dealt(p, q, 5, 2)
    assert pub.pieces == pieces == mpub.pieces and 32 * pub.kw <= 2 * pub.n.bit_length() + 64
    assert pub.z_words * 32 >= pub.z_bits and pm.split_shape(pub.n.bit_length(), pub.z_bits) == threshold.split_shape(pub.n.bit_length(), pub.z_bits)
    assert pub.v_bases == pm.piece_bases(mpub.v, pieces, pub.kw, pub.n_square)
    _, cts = ciphertexts(pub.n, 5)
    rhos = rho_rows(pub, len(cts))
    assert all(r < 1 << pub.rho_bits for r in rhos) and any(r >> (32 * pub.kw * (pieces - 1)) for r in rhos)      # the top piece is in use
    for s, ms in zip(shares[1:3], mshares[1:3]):
        col, proofs = s.partial_decrypt_batch(cts, prove=True, rng=DeviceRng(key=KEY, first_call=3))
        want = [pm.prove(mpub, ms, c, r) for c, r in zip(cts, rhos)]
        assert col == [w[0] for w in want]
        assert proofs.to_ints() == ([w[1] for w in want], [w[2] for w in want], [w[3] for w in want])
        assert proofs.z.shape == (len(cts), pub.z_words)
        assert pub.verify_batch(s.index, cts, col, proofs) == [True] * len(cts)
        assert all(pm.verify(mpub, s.index, c, *w) for c, w in zip(cts, want))
        # the proofs as they travel: ints, and rows again at the verifier
        again = threshold.DecryptionProofs.from_ints(*proofs.to_ints(), pub)
        assert pub.verify_batch(s.index, cts, col, again) == [True] * len(cts)
    # the multi-exponentiation got the exponent rows themselves: `pieces` terms of kw words
    assert ("multiexp_rows", pieces * len(cts), len(cts), pieces, 32 * pub.kw) in eng.calls


@pytest.mark.parametrize("p,q", [(P128, Q128), (P32, Q32)])
def test_every_single_tampering_is_false_for_that_row_only(p, q):
    eng, pub, shares, mpub, _ = dealt(p, q, 5, 2)
    _, cts = ciphertexts(pub.n, 4)
    col, proofs = shares[1].partial_decrypt_batch(cts, prove=True, rng=DeviceRng(key=KEY, first_call=3))
    other = pm.encrypt(pub.n, 77, 12345)
    for name, index, c, ci, a, b, z in tamperings(pub, cts, col, proofs, other):
        got = pub.verify_batch(index, c, ci, threshold.DecryptionProofs.from_ints(a, b, z, pub))
        assert got == [True, False, True, True], name
        fits = all(0 <= v < 1 << (32 * w) for vals, w in ((ci, pub.limbs2), (a, pub.limbs2), (b, pub.limbs2), (z, pub.z_words)) for v in vals)
        if fits:
            assert [pm.verify(mpub, index, *row) for row in zip(c, ci, a, b, z)] == got, name
    # another party's verification key: every row fails, nothing raises
    assert pub.verify_batch(3, cts, col, proofs) == [False] * 4
    # a lying party: partials made with a wrong exponent, proofs made honestly for that exponent
    liar = threshold.ThresholdKeyShare(pub, 2, shares[1].x ^ 1, engine=eng)
    lcol, lproofs = liar.partial_decrypt_batch(cts, prove=True, rng=DeviceRng(key=KEY, first_call=4))
    assert pub.verify_batch(2, cts, lcol, lproofs) == [False] * 4


def test_ctx_separates_parties_and_keys():
    _, pub, _, mpub, _ = dealt(P128, Q128, 5, 2)
    _, pub_b, _, _, _ = dealt(P128, Q128, 5, 2, seed=2)          # the same N, another v and other shares
    _, pub_c, _, _, _ = dealt(P128, Q128, 5, 3)
    _, pub_d, _, _, _ = dealt(P32, Q32, 5, 2)
    seen = {pub.ctx(i) for i in range(1, 6)} | {pub_b.ctx(1), pub_c.ctx(1), pub_d.ctx(1)}
    assert len(seen) == 8 and all(len(c) == 32 for c in seen)
    assert [pub.ctx(i) for i in range(1, 6)] == [mpub.ctx(i) for i in range(1, 6)]
    assert pub.ctx(2) == pm.context(pub.n, pub.v, pub.verification_keys[1], 2, 5, 2)


def test_a_proof_does_not_transfer_to_another_key():
    eng, pub, shares, _, _ = dealt(P128, Q128, 5, 2)
    _, pub_b, shares_b, _, _ = dealt(P128, Q128, 5, 2, seed=2)
    _, cts = ciphertexts(pub.n, 2)
    col, proofs = shares[0].partial_decrypt_batch(cts, prove=True, rng=DeviceRng(key=KEY, first_call=3))
    assert pub.verify_batch(1, cts, col, proofs) == [True, True]
    assert pub_b.verify_batch(1, cts, col, proofs) == [False, False]


def test_every_refusal_comes_before_an_engine_call():
    eng = ProofEngine()
    key = PaillierPrivateKey(P128, Q128, engine=eng)
    for parties, degree in ((1, 0), (1, 1), (3, 3), (3, 4), (3, 0), (3, -1)):
        with pytest.raises(ValueError):
            threshold.deal(key, parties, degree, rng=random.Random(1), check=False, engine=eng)
    with pytest.raises(ValueError, match="too many"):
        threshold.deal(key, 400, 2, rng=random.Random(1), check=False, engine=eng)      # 400! has 2887 bits: rows of nine pieces
    with pytest.raises(ValueError, match="safe primes"):
        threshold.deal(PaillierPrivateKey(13, 23, engine=eng), 3, 1, rng=random.Random(1), check=False, engine=eng)
    # check=True vets the key: a prime that is not safe is refused (decided on the host for one this small, on the engine otherwise)
    with pytest.raises(ValueError, match="safe primes"):
        threshold.deal(PaillierPrivateKey(65267, 65239, engine=eng), 3, 1, rng=random.Random(1), engine=eng)
    assert eng.calls == []
    pub, shares = threshold.deal(key, 5, 2, rng=random.Random(1), engine=eng)            # the golden primes pass the check
    assert [c[0] for c in eng.calls if c[0] in MARKERS] == ["safe_prime"]
    del eng.calls[:]
    _, cts = ciphertexts(pub.n, 2)
    with pytest.raises(KeyError):
        pub.combine_batch({1: [1, 2], 2: [3, 4]})
    with pytest.raises(ValueError, match="unknown party"):
        pub.combine_batch({1: [1, 2], 2: [3, 4], 6: [5, 6]})
    with pytest.raises(ValueError, match="unknown party"):
        pub.combine_batch({0: [1, 2], 2: [3, 4], 3: [5, 6]})
    with pytest.raises(ValueError, match="unknown party"):
        pub.verify_batch(9, cts, cts, threshold.DecryptionProofs.from_ints([1, 1], [1, 1], [1, 1], pub))
    with pytest.raises(ValueError):
        pub.verify_batch(1, cts, cts[:1], threshold.DecryptionProofs.from_ints([1, 1], [1, 1], [1, 1], pub))
    with pytest.raises(ValueError):
        pub.combine_batch({1: [1, 2], 2: [3, 4], 3: [5]})
    with pytest.raises(ValueError):
        threshold.DecryptionProofs.from_ints([1], [1, 2], [1], pub)
    with pytest.raises(ValueError):
        threshold.ThresholdKeyShare(pub, 6, 5)
    with pytest.raises(ValueError):
        threshold.ThresholdKeyShare(pub, 1, 1 << (pub.x_bits + 1))
    with pytest.raises(ValueError):
        threshold.ThresholdPublicKey(pub.n, 5, 2, pub.v, pub.verification_keys[:4], pub.x_bits)
    assert shares[0].partial_decrypt_batch([]) == [] and pub.combine_batch({1: [], 2: [], 3: []}) == []
    assert pub.verify_batch(1, [], [], shares[0].partial_decrypt_batch([], prove=True)[1]) == []
    assert eng.calls == []


def test_a_wrong_partial_without_proofs_is_the_references_error():
    eng, pub, shares, _, _ = dealt(P128, Q128, 3, 1)
    msgs, cts = ciphertexts(pub.n, 3)
    cols = {s.index: s.partial_decrypt_batch(cts) for s in shares}
    cols[2][1] = cols[2][1] * 3 % pub.n_square
    with pytest.raises(ValueError, match="not divisible by N"):
        pub.combine_batch({1: cols[1], 2: cols[2]})
    assert pub.combine_batch({1: cols[1], 3: cols[3]}) == msgs


def test_decrypt_verified_names_the_cheater_and_decrypts_from_the_rest():
    eng, pub, shares, _, _ = dealt(P128, Q128, 5, 2)
    msgs, cts = ciphertexts(pub.n, 4)
    sent = {s.index: s.partial_decrypt_batch(cts, prove=True, rng=DeviceRng(key=KEY, first_call=10 + s.index)) for s in shares}
    assert pub.decrypt_verified(cts, sent) == (msgs, [])
    bad = list(sent[2][0])
    bad[3] = bad[3] * 9 % pub.n_square
    sent[2] = (bad, sent[2][1])
    assert pub.decrypt_verified(cts, sent) == (msgs, [2])
    assert pub.decrypt_verified(cts, {i: sent[i] for i in (2, 3, 4, 5)}) == (msgs, [2])
    with pytest.raises(ValueError, match=r"invalid: \[2\]"):
        pub.decrypt_verified(cts, {i: sent[i] for i in (1, 2, 3)})
    with pytest.raises(ValueError, match="unknown party"):
        pub.decrypt_verified(cts, {7: sent[1]})
