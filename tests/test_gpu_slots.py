"""The slot codec on the GPU (csrc/mx_slots.hpp, Engine.slots_encode_t / slots_decode_t, slots.py) against Python-int
arithmetic and packing.unpack(..., use_numpy=False), and slot-packed encryption, a linear map and threshold decryption end
to end.

The rows are the C ABI's number format: little-endian radix-2^32 words, ``limbs.limbs_for(n)`` of them (5 at key_length
128, 65 at 2048 — one more than a wavefront has lanes — and 129 at 4096).  The 29-bit limbs of the Montgomery kernels never
leave those kernels, so "bit for bit" below means equal to ``limbs.pack`` of the defining integer, which also bounds every
word and the residue (the residue is asserted below N on its own as well)."""

from __future__ import annotations

import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY_LENGTHS = (128, 2048, 4096)
SIGNED_BITS = (1, 7, 29, 30, 32, 58, 63, 64)          # 7, 30, 58, 63: k b leaves spare bits below bits(N) - 2 at every key
UNSIGNED_BITS = (1, 32, 63)
WIDTHS = [(b, True) for b in SIGNED_BITS] + [(b, False) for b in UNSIGNED_BITS]


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


@pytest.fixture(scope="module")
def keys():
    from protocols.distributed_keygen_amd import synthetic

    return {kl: synthetic.make_key(kl, 3, 1) for kl in KEY_LENGTHS}


def definition(values, n, b, k):
    return [sum(m << (b * i) for i, m in enumerate(values[j : j + k])) % n for j in range(0, len(values), k)]


def value_range(b, signed):
    return (-(1 << (b - 1)), (1 << (b - 1)) - 1) if signed else (0, (1 << b) - 1)


def fills(count, b, signed, rng):
    lo, hi = value_range(b, signed)
    yield [lo] * count                                   # signed: the most negative S, a borrow through every word, then + N
    yield [hi] * count
    yield [-1 if signed else hi >> 1] * count
    yield [0] * count
    yield [lo if i & 1 else hi for i in range(count)]
    yield [rng.randint(lo, hi) for _ in range(count)]


def counts_for(k, key_length, b):
    out = {0, 1, k - 1, k, k + 1, 3 * k + 5}
    if (key_length, b) in ((128, 7), (128, 32), (128, 64), (2048, 64), (4096, 63)):
        out.add(150 * k + max(k // 2, 1))                # 151 plaintexts: three workgroups of 64 rows, the last one ragged
    return sorted(c for c in out if c >= 0)


@pytest.mark.parametrize("b,signed", WIDTHS)
@pytest.mark.parametrize("key_length", KEY_LENGTHS)
def test_encode_and_decode_match_the_definition(eng, keys, key_length, b, signed):
    import torch

    from protocols.distributed_keygen_amd import limbs, packing

    n = keys[key_length].n
    k = packing.slots_per_ciphertext(n, b)
    ln = limbs.limbs_for(n)
    rng = random.Random(f"{key_length}/{b}/{signed}")
    for count in counts_for(k, key_length, b):
        for fill, vals in enumerate(fills(count, b, signed, rng)):
            want = definition(vals, n, b, k)
            v_np = np.array(vals, dtype=np.int64)
            stride = ln + (3 if fill == 1 else 0)        # wider rows: the extra words are zero
            src = torch.from_numpy(v_np).to(eng.device) if fill & 1 else v_np      # a device tensor, or an upload
            rows_t = eng.slots_encode_t(src, n, b, signed=signed, row_words=None if stride == ln else stride)
            assert tuple(rows_t.shape) == (-(-count // k), stride) and rows_t.dtype == torch.int32
            rows = eng.to_host(rows_t)
            assert np.array_equal(rows[:, :ln], limbs.pack(want, ln)), (key_length, b, signed, count, fill)
            assert not rows[:, ln:].any()
            assert all(v < n for v in limbs.unpack(rows[:, :ln]))
            got = eng.slots_decode_t(rows_t, n, b, count, signed=signed)
            assert got.dtype == torch.int64 and got.device == eng.device
            assert got.tolist() == vals, (key_length, b, signed, count, fill)


@pytest.mark.parametrize("key_length", KEY_LENGTHS)
def test_decode_of_arbitrary_residues_is_packing_unpack(eng, keys, key_length):
    import torch

    from protocols.distributed_keygen_amd import limbs, packing

    n = keys[key_length].n
    ln = limbs.limbs_for(n)
    rng = random.Random(key_length)
    for b, signed in WIDTHS:
        k = packing.slots_per_ciphertext(n, b)
        res = [0, 1, n - 1, n // 2, n // 2 + 1, (1 << (b * k)) - 1] + [rng.randrange(n) for _ in range(70)]
        count = len(res) * k - (k // 2)
        want = packing.unpack(res, b, count, n, signed=signed, use_numpy=False)
        rows = limbs.pack(res, ln)
        assert eng.slots_decode_t(eng.to_device(rows), n, b, count, signed=signed).tolist() == want, (b, signed)
        # the rows of combine_t(..., packed=True): one more word, here with something in it
        wide = np.concatenate([rows, np.full((len(res), 1), 0x80000001, dtype="<u4")], axis=1)
        assert eng.slots_decode_t(eng.to_device(wide), n, b, count, signed=signed).tolist() == want, (b, signed)
    with pytest.raises(ValueError):
        eng.slots_decode_t(eng.to_device(rows), n, 32, 1)                           # 76 rows for one value
    with pytest.raises(ValueError):
        eng.slots_decode_t(eng.to_device(rows[:1, : ln - 1]), n, 32, 1)             # rows narrower than N
    assert eng.slots_decode_t(torch.empty((0, ln), dtype=torch.int32, device=eng.device), n, 32, 0).tolist() == []


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("key_length", KEY_LENGTHS)
def test_out_of_range_values_are_refused_with_the_first_index(eng, keys, key_length, signed):
    from protocols.distributed_keygen_amd import packing

    n = keys[key_length].n
    b = 9
    k = packing.slots_per_ciphertext(n, b)
    lo, hi = value_range(b, signed)
    count = 70 * k + 3                                                              # 71 plaintexts, the last one ragged
    rng = random.Random(key_length + signed)
    base = [rng.randint(lo, hi) for _ in range(count)]
    for bad_at in (k - 1, 35 * k + 2, count - 1):                                   # first, a middle and the last plaintext
        for bad in (hi + 1, lo - 1):
            vals = list(base)
            vals[bad_at] = bad
            vals[-1] = bad if bad_at != count - 1 else vals[-1]                     # a later offender does not change the index
            with pytest.raises(ValueError, match=rf"value {bad_at} \({bad}\)"):
                eng.slots_encode_t(np.array(vals, dtype=np.int64), n, b, signed=signed)
    for width, sg in ((65, True), (64, False), (0, True)):
        with pytest.raises(ValueError):
            eng.slots_encode_t(np.array([0], dtype=np.int64), n, width, signed=sg)


def test_abi_refuses_bad_arguments_without_a_launch(eng, keys):
    import torch

    from protocols.distributed_keygen_amd import limbs

    n = keys[128].n
    ln = limbs.limbs_for(n)
    bits = n.bit_length()
    h_n = limbs.pack_one(n, ln)
    even = limbs.pack_one(n - 1, ln)
    vals = torch.arange(8, dtype=torch.int64, device=eng.device)
    out = torch.zeros((8, ln + 1), dtype=torch.int32, device=eng.device)
    st = torch.zeros(8, dtype=torch.uint8, device=eng.device)
    dec = torch.zeros(8, dtype=torch.int64, device=eng.device)
    lib, s = eng.lib, eng._stream_ptr()
    v, o, t, d, hn = vals.data_ptr(), out.data_ptr(), st.data_ptr(), dec.data_ptr(), h_n.ctypes.data
    enc = lambda *a: lib.mx_slots_encode(*a, s)                                     # noqa: E731
    assert enc(v, 8, hn, ln, 32, (bits - 2) // 32 + 1, 1, o, ln, t) == -1           # slots * slot_bits > bits(N) - 2
    assert enc(v, 8, hn, ln, 65, 1, 1, o, ln, t) == -1
    assert enc(v, 8, hn, ln, 64, 1, 0, o, ln, t) == -1                              # unsigned: 63 at the most
    assert enc(v, 8, hn, ln, 0, 1, 1, o, ln, t) == -1
    assert enc(v, 8, hn, ln, 8, 0, 1, o, ln, t) == -1
    assert enc(v, 8, hn, ln, 8, 4, 1, o, ln - 1, t) == -1                           # a stride narrower than N
    assert enc(v, -1, hn, ln, 8, 4, 1, o, ln, t) == -1
    assert enc(None, 8, hn, ln, 8, 4, 1, o, ln, t) == -1
    assert enc(v, 8, hn, ln, 8, 4, 1, None, ln, t) == -1
    assert enc(v, 8, hn, ln, 8, 4, 1, o, ln, None) == -1
    assert enc(v, 8, None, ln, 8, 4, 1, o, ln, t) == -1
    assert enc(v, 8, even.ctypes.data, ln, 8, 4, 1, o, ln, t) == -3
    assert lib.mx_slots_decode(o, ln - 1, 8, hn, ln, 8, 4, 1, d, s) == -1
    assert lib.mx_slots_decode(o, ln, 8, hn, ln, 64, 1, 0, d, s) == -1
    assert lib.mx_slots_decode(None, ln, 8, hn, ln, 8, 4, 1, d, s) == -1
    assert lib.mx_slots_decode(o, ln, 8, hn, ln, 8, 4, 1, None, s) == -1
    assert enc(v, 0, hn, ln, 8, 4, 1, o, ln, t) == 0                                # nothing to do: no launch
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0 and int(st.sum()) == 0 and int(dec.abs().sum()) == 0
    assert enc(v, 8, hn, ln, 8, 4, 1, o, ln + 1, t) == 0
    torch.cuda.synchronize()
    assert limbs.unpack(eng.to_host(out)[:2, :ln]) == definition(list(range(8)), n, 8, 4) and int(st.sum()) == 0


def paillier_decrypt(key, c):
    lam = (key.p - 1) * (key.q - 1)
    return (pow(c, lam, key.n_square) - 1) // key.n * pow(lam, -1, key.n) % key.n


def test_slot_packed_encryption_linear_map_and_threshold_decryption(eng, keys):
    import torch

    from protocols.distributed_keygen_amd import FastRandomizer, homomorphic, limbs, packing, slots

    key = keys[128]
    n, n2 = key.n, key.n_square
    rng = random.Random(53)
    y = rng.randrange(2, n)
    h_s = pow(-y * y % n, n, n2)
    value_bits, weight_bits, features, bias_bits = 8, 5, 3, 6
    b = slots.slot_bits_for(value_bits, weight_bits, features, bias_bits)
    k = packing.slots_per_ciphertext(n, b)
    count = k + 2                                                                   # samples across slots, a ragged second plaintext
    x = np.array([[rng.randint(-128, 127) for _ in range(count)] for _ in range(features)], dtype=np.int64)
    x[:, 0], x[:, 1] = -128, 127
    w = np.array([[31, -31, 31], [-31, -31, -31]], dtype=np.int64)
    beta = np.array([63, -63], dtype=np.int64)

    # 1. explicit exponents: the pow formula
    rz = FastRandomizer(n, h_s, engine=eng)
    exps = [rng.getrandbits(rz.exp_bits) for _ in range(2)]
    plain = definition(x[0].tolist(), n, b, k)
    assert slots.encrypt(x[0], rz, b, exponents=exps) == [(1 + p * n) * pow(h_s, a, n2) % n2 for p, a in zip(plain, exps)]
    # 2. exponents drawn on the device: fresh ciphertexts of the same plaintexts
    rz_dev = FastRandomizer(n, h_s, engine=eng, device_rng=True)
    cts = [slots.encrypt(torch.from_numpy(x[f]).to(eng.device), rz_dev, b) for f in range(features)]
    assert cts[0] != slots.encrypt(x[0], rz, b, exponents=exps)
    for f in range(features):
        assert [paillier_decrypt(key, c) for c in cts[f]] == definition(x[f].tolist(), n, b, k)
    # 3. W x + beta on every slot at once: one linear map per packed plaintext, the bias encoded once per slot
    bias = [slots.encode([int(bt)] * count, n, b, engine=eng) for bt in beta]
    outs = [homomorphic.linear_map([cts[f][j] for f in range(features)], w.tolist(), n, bias=[bias[r][j] for r in range(2)], engine=eng)
            for j in range(2)]
    # 4. partial decryptions with the key's shares -> combine_t -> slots_decode_t, on the device
    flat = [outs[j][r] for r in range(2) for j in range(2)]                         # row-major: the plaintexts of output row r in order
    l2 = limbs.limbs_for(n2)
    partials = []
    for i in (1, 2, 3):
        e = key.exponent(i)
        bases = flat if e >= 0 else eng.modinv_batch(flat, n2)
        partials.append(eng.powmod_nsquare_t(eng.to_device(limbs.pack_reduced(bases, l2, n2)), n, abs(e)))
    rows_t = eng.combine_t(torch.stack(partials), n, key.theta_inv, packed=True)
    got = [eng.slots_decode_t(rows_t[2 * r : 2 * r + 2], n, b, count) for r in range(2)]
    assert not eng.to_host(rows_t)[:, -1].any()                                     # every recombination divisible
    # 5. the slot-wise integer matrix product
    want = w @ x + beta[:, None]
    assert torch.stack(got).cpu().numpy().tolist() == want.tolist()
    assert slots.decode_t(rows_t[:2], n, b, count, engine=eng).tolist() == want[0].tolist()


def test_decode_behind_a_kernel_on_the_same_stream_needs_no_host_synchronisation(eng, keys):
    """The rows are written by a modular multiplication enqueued just before the decode, on a side stream; the only
    synchronisation is the fetch of the decoded values."""
    import torch

    from protocols.distributed_keygen_amd import limbs, packing

    n = keys[2048].n
    ln = limbs.limbs_for(n)
    b = 32
    k = packing.slots_per_ciphertext(n, b)
    rng = random.Random(59)
    res = [rng.randrange(n) for _ in range(3000)]
    count = len(res) * k - 7
    want = packing.unpack(res, b, count, n, use_numpy=False)
    a_t = eng.to_device(limbs.pack(res, ln))
    one_t = eng.to_device(limbs.pack([1] * len(res), ln))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rows_t = eng.mulmod_t(a_t, one_t, n)
        vals_t = eng.slots_decode_t(rows_t, n, b, count)
    torch.cuda.current_stream().wait_stream(side)
    assert vals_t.tolist() == want
