"""The kernels of the decryption proofs (csrc/mx_sha256.hpp, csrc/mx_response.hpp) and the dealt threshold key over them on
the GPU — Engine.sha256_rows_t / dleq_response_t / multiexp_nsquare_rows_t / dleq_prove_t / dleq_verify_t and
threshold.py — bit for bit against hashlib, Python ints and tools/proof_model.py.

SHA-256: the message has 8 + sum limbs words, so one set of 5, 6, 7 or 8 limbs leaves 13, 14, 15 or 0 words in the last
block — at and around the point where the length field no longer fits; 1, 129 and 257 limbs, four sets of unequal
widths, eight sets and no set at all; counts around the wavefront (63, 64, 65) and beyond a workgroup (300)."""

from __future__ import annotations

import hashlib
import json
import random
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import chacha_model  # noqa: E402
import proof_model as pm  # noqa: E402

GOLDEN = json.loads((ROOT / "tests" / "golden" / "threshold_keys.json").read_text())
KEY = bytes(range(32))
COUNTS = (1, 63, 64, 65, 300)


def primes_of(key_length):
    return tuple(int(GOLDEN["keys"][str(key_length)][k], 16) for k in "pq")


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def rows_of(eng, values, width):
    from protocols.distributed_keygen_amd import limbs

    return eng.to_device(limbs.pack(values, width).reshape(len(values), width))


def ints_of(eng, rows_t):
    from protocols.distributed_keygen_amd import limbs

    return limbs.unpack(eng.to_host(rows_t))


def row_values(width, count, seed):
    """All-ones and zero rows first, rows of 0x80000000 words, then random ones."""
    rnd = random.Random(seed)
    special = [(1 << (32 * width)) - 1, 0, sum(0x80000000 << (32 * k) for k in range(width))]
    return (special + [rnd.getrandbits(32 * width) for _ in range(count)])[:count] if count >= 3 else [rnd.getrandbits(32 * width) | 1 for _ in range(count)]


def want_digests(prefix, sets):
    return pm.sha256_rows(prefix, sets)


# ------------------------------------------------------------------ SHA-256
@pytest.mark.parametrize("limbs_", [1, 5, 6, 7, 8, 129, 257])
def test_sha256_of_one_row_set_at_every_padding_case(eng, limbs_):
    prefix = hashlib.sha256(b"prefix %d" % limbs_).digest()
    vals = row_values(limbs_, max(COUNTS), limbs_)
    want = want_digests(prefix, [(vals, limbs_)])
    rows_t = rows_of(eng, vals, limbs_)
    for count in COUNTS:
        got_t = eng.sha256_rows_t(prefix, [rows_t[:count].contiguous()])
        assert tuple(got_t.shape) == (count, 8)
        assert ints_of(eng, got_t) == want[:count], (limbs_, count)
    # the bytes themselves, once: word 7 of the row holds the digest's first four bytes
    one = eng.to_host(eng.sha256_rows_t(prefix, [rows_t[:1].contiguous()]))[0]
    assert b"".join(int(w).to_bytes(4, "big") for w in one[::-1]) == hashlib.sha256(prefix + vals[0].to_bytes(4 * limbs_, "big")).digest()


@pytest.mark.parametrize("widths", [(3, 1, 17, 4), (1, 2, 3, 4, 5, 6, 7, 8), (128, 128, 128, 128), ()])
def test_sha256_of_several_row_sets_and_of_none(eng, widths):
    prefix = bytes(range(200, 232))
    for count in (1, 65, 300):
        sets = [(row_values(w, count, 31 * w + k), w) for k, w in enumerate(widths)]
        want = want_digests(prefix, sets) if widths else [int.from_bytes(hashlib.sha256(prefix).digest(), "big")] * count
        got_t = eng.sha256_rows_t(prefix, [rows_of(eng, v, w) for v, w in sets], count=None if widths else count)
        assert ints_of(eng, got_t) == want, (widths, count)


def test_sha256_refusals_launch_nothing(eng):
    rows_t = rows_of(eng, [1, 2], 3)
    with pytest.raises(ValueError):
        eng.sha256_rows_t(b"short", [rows_t])
    with pytest.raises(ValueError):
        eng.sha256_rows_t(bytes(32), [rows_t] * 9)
    with pytest.raises(ValueError):
        eng.sha256_rows_t(bytes(32), [rows_t, rows_of(eng, [1], 3)])
    with pytest.raises(ValueError):
        eng.sha256_rows_t(bytes(32), [])
    with pytest.raises(ValueError):
        eng.sha256_rows_t(bytes(32), [rows_t[:, :2]])              # not contiguous
    assert tuple(eng.sha256_rows_t(bytes(32), [rows_t[:0].contiguous()]).shape) == (0, 8)


# ------------------------------------------------------------------ the response
@pytest.mark.parametrize("wz,ew,wx", [(17, 4, 9), (12, 4, 8), (5, 1, 1), (140, 4, 131)])
def test_dleq_response_equals_python_ints(eng, wz, ew, wx):
    rnd = random.Random(wz * 1000 + wx)
    x = rnd.getrandbits(32 * wx) | 1 << (32 * wx - 1)
    x_t = rows_of(eng, [x], wx)
    for count in (1, 64, 65):
        # rho < 2^(32 wz - 1) and e x < 2^(32 wz - 1): the sum fits
        rho = [rnd.getrandbits(32 * wz - 1) for _ in range(count)]
        e = [rnd.getrandbits(32 * ew - (1 if wx + ew == wz else 0)) for _ in range(count)]
        want, status = pm.dleq_response(rho, e, x, wz)
        assert not any(status)
        z_t, status_t = eng.dleq_response_t(rows_of(eng, rho, wz), rows_of(eng, e, ew), x_t)
        assert ints_of(eng, z_t) == want and [int(s) for s in status_t.cpu()] == status


def test_dleq_response_directed_carries_and_the_forced_overflow(eng):
    wz, ew, wx = 12, 4, 8
    ones_x = (1 << (32 * wx)) - 1
    e_max = (1 << 128) - 1
    e_odd = random.Random(7).getrandbits(128) | 1
    x_inv = pow(e_odd, -1, 1 << (32 * wx))                 # e x = ...0001 in its low 32 wx bits
    assert e_odd * x_inv % (1 << (32 * wx)) == 1
    cases = [  # (rho, e, x)
        *[((1 << k) - 1, e_odd, x_inv) for k in (1, 32, 33, 64, 255, 256, 32 * wx, 32 * wz - 1)],      # a carry through k bits
        (0, e_max, ones_x), ((1 << (32 * wz - 1)) - 1, e_max, ones_x), (12345, 0, ones_x), ((1 << (32 * wz)) - 1, 0, ones_x),
        (12345, e_max, 0), ((1 << (32 * wz)) - 1, e_max, 0), (0, 0, 0),
    ]
    for rho, e, x in cases:
        want, status = pm.dleq_response([rho] * 3, [e] * 3, x, wz)
        z_t, status_t = eng.dleq_response_t(rows_of(eng, [rho] * 3, wz), rows_of(eng, [e] * 3, ew), rows_of(eng, [x], wx)[0])
        assert ints_of(eng, z_t) == want and [int(s) for s in status_t.cpu()] == status, (hex(rho), hex(e), hex(x))
    # the forced overflow: row 40 of 70 does not fit — through the last carry, and through a column above wz (wx + ew > wz)
    for wx2, x in ((8, ones_x), (10, (1 << 320) - 1)):
        rho = [random.Random(k).getrandbits(32 * wz - 2) for k in range(70)]
        e = [random.Random(100 + k).getrandbits(64 if wx2 == 8 else 30) for k in range(70)]
        rho[40], e[40] = (1 << (32 * wz)) - 1, (1 if wx2 == 8 else e_max)
        want, status = pm.dleq_response(rho, e, x, wz)
        assert status == [0] * 40 + [1] + [0] * 29
        z_t, status_t = eng.dleq_response_t(rows_of(eng, rho, wz), rows_of(eng, e, ew), rows_of(eng, [x], wx2))
        assert [int(s) for s in status_t.cpu()] == status and ints_of(eng, z_t) == want
    # in place
    rho_t = rows_of(eng, [5, 6], wz)
    z_t, _ = eng.dleq_response_t(rho_t, rows_of(eng, [2, 3], ew), rows_of(eng, [7], wx), out_t=rho_t)
    assert z_t is rho_t and ints_of(eng, rho_t) == [19, 27]


# ------------------------------------------------------------------ the thin multi-exponentiation
@pytest.mark.parametrize("terms", [1, 2, 3])
@pytest.mark.parametrize("rows", [1, 65])
def test_multiexp_rows_equals_the_planned_multiexp(eng, terms, rows):
    import torch

    p, q = primes_of(128)
    n = p * q
    n2 = n * n
    rnd = random.Random(terms * 100 + rows)
    weight_bits = 2 * n.bit_length() + 64 if terms == 2 else 100
    ww = (weight_bits + 31) // 32
    xs = [rnd.randrange(1, n2) for _ in range(rows * terms)]
    index = [[rnd.randrange(len(xs)) for _ in range(terms)] for _ in range(rows)]
    weights = [[rnd.getrandbits(weight_bits) for _ in range(terms)] for _ in range(rows)]
    weights[0][0] = 0
    inputs_t = rows_of(eng, xs, pm.limbs_for(n2))
    index_t = torch.tensor(index, dtype=torch.int32, device=eng.device)
    w_t = rows_of(eng, [w for row in weights for w in row], ww).view(rows, terms, ww)
    got = ints_of(eng, eng.multiexp_nsquare_rows_t(inputs_t, index_t, w_t, terms, weight_bits, n))
    dense = []
    for r in range(rows):
        row = {}
        for i, w in zip(index[r], weights[r]):
            row[i] = row.get(i, 0) + w
        dense.append(row)
    want = [1] * rows
    for r in range(rows):
        for i, w in zip(index[r], weights[r]):
            want[r] = want[r] * pow(xs[i], w, n2) % n2
    assert got == want
    if all(w < 1 << weight_bits for row in dense for w in row.values()):
        assert got == ints_of(eng, eng.multiexp_nsquare_t(inputs_t, dense, n))
    with pytest.raises(ValueError):
        eng.multiexp_nsquare_rows_t(inputs_t, index_t + len(xs), w_t, terms, weight_bits, n)
    with pytest.raises(ValueError):
        eng.multiexp_nsquare_rows_t(inputs_t, index_t, w_t, terms, 2 * n.bit_length() + 65, n)


# ------------------------------------------------------------------ prove / verify / combine
def dealt(eng, key_length, parties, degree, check):
    from protocols.distributed_keygen_amd import threshold
    from protocols.distributed_keygen_amd.private_key import PaillierPrivateKey

    p, q = primes_of(key_length)
    pub, shares = threshold.deal(PaillierPrivateKey(p, q, engine=eng), parties, degree, rng=random.Random(1), check=check, engine=eng)
    return pub, shares


def ciphertexts(n, count, seed=5):
    rnd = random.Random(seed)
    msgs = ([0, 1, n - 1] + [rnd.randrange(n) for _ in range(count)])[:count]
    return msgs, [pm.encrypt(n, m, rnd.randrange(1, n)) for m in msgs]


@pytest.fixture(scope="module")
def key128(eng):
    """The key of 128 bits dealt to five parties (the check of the primes runs on the device), seven ciphertexts, the
    model's proofs of every party and the engine's — computed once, left unchanged."""
    from protocols.distributed_keygen_amd.device_rng import DeviceRng

    pub, shares = dealt(eng, 128, 5, 2, check=True)
    mpub, mshares = pm.deal(*primes_of(128), 5, 2, random.Random(1))
    msgs, cts = ciphertexts(pub.n, 7)
    sent, want = {}, {}
    for s, ms in zip(shares, mshares):
        rhos = chacha_model.row_ints(KEY, 20 + s.index, len(cts), pub.rho_bits, pub.z_words)
        want[s.index] = [pm.prove(mpub, ms, c, r) for c, r in zip(cts, rhos)]
        sent[s.index] = s.partial_decrypt_batch(cts, prove=True, rng=DeviceRng(key=KEY, first_call=20 + s.index))
    return pub, shares, mpub, msgs, cts, sent, want


def test_every_proof_row_equals_the_models(key128):
    pub, shares, mpub, msgs, cts, sent, want = key128
    assert (pub.v, pub.verification_keys, pub.pieces, pub.kw) == (mpub.v, mpub.vks, 2, mpub.kw)
    for i in range(1, 6):
        col, proofs = sent[i]
        assert col == [w[0] for w in want[i]]
        assert proofs.to_ints() == ([w[1] for w in want[i]], [w[2] for w in want[i]], [w[3] for w in want[i]])
        assert pub.verify_batch(i, cts, col, proofs) == [True] * len(cts)


def test_every_tampering_is_false_for_its_row_only_on_the_device(key128):
    from proof_engine import tamperings

    from protocols.distributed_keygen_amd import threshold

    pub, shares, mpub, msgs, cts, sent, want = key128
    col, proofs = sent[2]
    other = pm.encrypt(pub.n, 77, 12345)
    for name, index, c, ci, a, b, z in tamperings(pub, cts, col, proofs, other):
        got = pub.verify_batch(index, c, ci, threshold.DecryptionProofs.from_ints(a, b, z, pub))
        assert got == [True, False] + [True] * 5, name
    assert pub.verify_batch(3, cts, col, proofs) == [False] * 7                      # another party's verification key
    assert pub.verify_batch(2, cts, sent[3][0], sent[3][1]) == [False] * 7


def test_any_subset_combines_and_the_cheater_is_named(key128):
    from protocols.distributed_keygen_amd import threshold

    pub, shares, mpub, msgs, cts, sent, want = key128
    for sub in ((1, 2, 3), (2, 4, 5), (1, 3, 5)):                                   # (2, 4, 5) and (1, 3, 5) have negative lambdas
        assert pub.combine_batch({i: sent[i][0] for i in sub}) == msgs
    assert any(v < 0 for v in threshold.lagrange(pub.delta, (2, 4, 5)).values())
    bad = list(sent[4][0])
    bad[6] = bad[6] * 9 % pub.n_square
    with pytest.raises(ValueError, match="not divisible by N"):
        pub.combine_batch({2: sent[2][0], 4: bad, 5: sent[5][0]})
    assert pub.decrypt_verified(cts, {2: sent[2], 4: (bad, sent[4][1]), 5: sent[5], 1: sent[1]}) == (msgs, [4])
    with pytest.raises(KeyError):
        pub.combine_batch({2: sent[2][0], 4: bad})
    with pytest.raises(ValueError, match="unknown party"):
        pub.combine_batch({2: sent[2][0], 4: bad, 9: bad})


@pytest.mark.parametrize("key_length", [1024, 2048])
def test_verified_decryption_end_to_end_at_real_key_lengths(eng, key_length):
    pub, shares = dealt(eng, key_length, 3, 1, check=False)
    assert pub.pieces == 2
    msgs, cts = ciphertexts(pub.n, 3)
    honest = {s.index: s.partial_decrypt_batch(cts, prove=True) for s in shares}     # rho from the shares' own generators
    assert honest[1][0] == [pow(c, 2 * shares[0].x, pub.n_square) for c in cts]
    a, b, z = honest[1][1].to_ints()
    mpub = pm.PublicKey(pub.n, 3, 1, pub.v, pub.verification_keys, pub.x_bits)
    assert pm.verify(mpub, 1, cts[0], honest[1][0][0], a[0], b[0], z[0])
    assert pub.verify_batch(1, cts, *honest[1]) == [True] * 3
    cheat = list(honest[2][0])
    cheat[1] = cheat[1] * cts[1] % pub.n_square
    assert pub.verify_batch(2, cts, cheat, honest[2][1]) == [True, False, True]
    assert pub.decrypt_verified(cts, {1: honest[1], 2: (cheat, honest[2][1]), 3: honest[3]}) == (msgs, [2])


# ------------------------------------------------------------------ the C ABI refuses by itself
def test_the_c_entry_points_refuse_bad_arguments_without_a_launch(eng):
    import ctypes

    lib, fake = eng.lib, 1 << 20
    prefix = bytes(32)
    ptrs, widths = (ctypes.c_void_p * 9)(*[fake] * 9), (ctypes.c_int * 9)(*[3] * 9)
    assert lib.mx_sha256_rows(None, ptrs, widths, 1, 4, fake, None) == -1
    assert lib.mx_sha256_rows(prefix, ptrs, widths, 1, 4, None, None) == -1
    assert lib.mx_sha256_rows(prefix, None, widths, 1, 4, fake, None) == -1
    assert lib.mx_sha256_rows(prefix, ptrs, None, 1, 4, fake, None) == -1
    assert lib.mx_sha256_rows(prefix, ptrs, widths, 9, 4, fake, None) == -1
    assert lib.mx_sha256_rows(prefix, ptrs, widths, -1, 4, fake, None) == -1
    assert lib.mx_sha256_rows(prefix, ptrs, widths, 1, -1, fake, None) == -1
    assert lib.mx_sha256_rows(prefix, ptrs, (ctypes.c_int * 2)(3, 0), 2, 4, fake, None) == -1
    assert lib.mx_sha256_rows(prefix, (ctypes.c_void_p * 2)(fake, None), widths, 2, 4, fake, None) == -1
    assert lib.mx_sha256_rows(prefix, ptrs, (ctypes.c_int * 1)(1 << 25), 1, 4, fake, None) == -2
    assert lib.mx_sha256_rows(prefix, ptrs, widths, 1, 1 << 62, fake, None) == -2
    assert lib.mx_sha256_rows(prefix, ptrs, widths, 8, 0, fake, None) == 0                # nothing to do
    assert lib.mx_sha256_rows(prefix, None, None, 0, 0, fake, None) == 0
    for bad in ((None, fake, fake, fake, fake), (fake, None, fake, fake, fake), (fake, fake, None, fake, fake),
                (fake, fake, fake, None, fake), (fake, fake, fake, fake, None)):
        assert lib.mx_dleq_response(*bad, 4, 1, 2, 8, None) == -1
    five = (fake,) * 5
    assert lib.mx_dleq_response(*five, 0, 1, 2, 8, None) == -1 and lib.mx_dleq_response(*five, 4, 0, 2, 8, None) == -1
    assert lib.mx_dleq_response(*five, 4, 1, 0, 8, None) == -1 and lib.mx_dleq_response(*five, 4, 1, 2, -1, None) == -1
    assert lib.mx_dleq_response(*five, (1 << 20) + 1, 1, 2, 8, None) == -2 and lib.mx_dleq_response(*five, 4, 1, 2, 1 << 62, None) == -2
    assert lib.mx_dleq_response(*five, 4, 1, 2, 0, None) == 0
