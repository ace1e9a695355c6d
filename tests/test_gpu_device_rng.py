"""Random rows drawn on the GPU (csrc/mx_chacha.hpp, Engine.chacha20_rows_t / random_rows_t, device_rng.DeviceRng):
the keystream bit for bit against tools/chacha_model.py, and everything that consumes it — FastRandomizer,
homomorphic.linear_map, packing.pack, encrypt_fresh_batch / randomize_fresh_batch — against CPython pow with the
model's rows."""

from __future__ import annotations

import ctypes
import random
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import chacha_model as cm  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes((11 * k + 5) & 0xFF for k in range(32))
RFC_KEY = bytes(range(32))
RFC_BLOCK = bytes.fromhex(
    "10f1e7e4d13b5915500fdd1fa32071c4" "c7d1f4c733c068030422aa9ac3d46c4e"
    "d2826446079faa0914c2d705d98b02a2" "b5129cd1de164eb9cbd083e8a2503c4e")


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def make_rng(first_call=0, key=KEY):
    from protocols.distributed_keygen_amd.device_rng import DeviceRng

    return DeviceRng(key=key, first_call=first_call)


def host_rows(eng, rows_t):
    return eng.to_host(rows_t).tolist()


SHAPES = [
    (1, 32, 1),
    (1, 512, 16),            # exactly one block
    (5, 96, 3),              # 15 words: a partial last block
    (7, 1026, 33),           # rows straddle blocks, top-word mask of 2 bits
    (3, 195, 9),             # zero padding beyond w
    (300, 1026, 33),         # 9 900 words = 619 blocks: more than one workgroup, a ragged last one
    (4097, 33, 2),           # mask of 1 bit on many short rows
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_keystream_matches_the_model(eng, shape):
    import torch

    count, bits, row_words = shape
    call = 1 + (count << 40)                     # a nonce with more than one word in use
    rows_t = make_rng(call).rows_t(eng, count, bits, row_words)
    assert rows_t.dtype == torch.int32 and tuple(rows_t.shape) == (count, row_words) and rows_t.device == eng.device
    assert host_rows(eng, rows_t) == cm.rows(KEY, call, count, bits, row_words)
    # the engine-side call and the default row width give the same rows
    w = -(-bits // 32)
    again = eng.random_rows_t(make_rng(call), count, bits)
    assert host_rows(eng, again) == [row[:w] for row in cm.rows(KEY, call, count, bits, row_words)]


def test_successive_calls_differ_and_each_equals_the_model_at_its_call_number(eng):
    rng = make_rng(first_call=(1 << 32) - 1)     # the second call carries into nonce word 14
    a = host_rows(eng, rng.rows_t(eng, 9, 100))
    b = host_rows(eng, rng.rows_t(eng, 9, 100))
    assert a != b and rng.next_call == (1 << 32) + 1
    assert a == cm.rows(KEY, (1 << 32) - 1, 9, 100) and b == cm.rows(KEY, 1 << 32, 9, 100)


def test_counter0_is_honoured_at_the_abi(eng):
    """A direct mx_chacha20_rows call with the key, nonce and counter of RFC 8439 §2.3.2 reproduces its block."""
    import torch

    key = (ctypes.c_uint32 * 8)(*cm.key_words(RFC_KEY))
    nonce = (ctypes.c_uint32 * 3)(0x09000000, 0x4A000000, 0)
    out_t = torch.zeros((1, 16), dtype=torch.int32, device=eng.device)
    with torch.cuda.device(eng.device):
        assert eng.lib.mx_chacha20_rows(key, nonce, 1, out_t.data_ptr(), 1, 16, 512, eng._stream_ptr()) == 0
    assert eng.to_host(out_t).astype("<u4").tobytes() == RFC_BLOCK
    # ... and through the engine: blocks 1 and 2 are rows 1 and 2 of a draw that starts at block 0
    three = host_rows(eng, eng.chacha20_rows_t(cm.key_words(KEY), [5, 6, 7], 0, 3, 512))
    assert host_rows(eng, eng.chacha20_rows_t(cm.key_words(KEY), [5, 6, 7], 1, 2, 512)) == three[1:]
    # the last block the counter can address
    last = eng.chacha20_rows_t(cm.key_words(KEY), [5, 6, 7], 0xFFFFFFFF, 16, 32)
    assert [r[0] for r in host_rows(eng, last)] == cm.block(cm.key_words(KEY), 0xFFFFFFFF, [5, 6, 7])


def test_refused_arguments_and_an_empty_request(eng):
    import torch

    lib, s = eng.lib, eng._stream_ptr()
    key, nonce = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 3)()
    out_t = torch.zeros((4, 2), dtype=torch.int32, device=eng.device)
    o = out_t.data_ptr()
    call = lib.mx_chacha20_rows
    assert call(None, nonce, 0, o, 4, 2, 64, s) == -1
    assert call(key, None, 0, o, 4, 2, 64, s) == -1
    assert call(key, nonce, 0, None, 4, 2, 64, s) == -1
    assert call(key, nonce, 0, o, -1, 2, 64, s) == -1
    assert call(key, nonce, 0, o, 4, 2, 0, s) == -1
    assert call(key, nonce, 0, o, 4, 2, 65, s) == -1                     # bits > 32 * row_words
    assert call(key, nonce, 0xFFFFFFFF, o, 17, 1, 32, s) == -1           # two blocks from the last counter value
    assert call(key, nonce, 1, o, 1 << 36, 1, 32, s) == -1               # 2^32 blocks from counter 1
    assert call(key, nonce, 0, o, (1 << 36) + 1, 1, 32, s) == -1
    assert call(key, nonce, 0, o, 0, 2, 64, s) == 0                      # count = 0: MX_OK, no launch
    torch.cuda.synchronize()
    assert int(out_t.abs().sum()) == 0                                   # nothing was launched
    rng = make_rng(3)
    empty = rng.rows_t(eng, 0, 70)
    assert tuple(empty.shape) == (0, 3) and empty.dtype == torch.int32 and rng.next_call == 4
    with pytest.raises(ValueError):
        rng.rows_t(eng, (1 << 36) + 1, 32)
    with pytest.raises(ValueError):
        eng.chacha20_rows_t(cm.key_words(KEY), [0, 0, 0], 0xFFFFFFFF, 17, 32)
    assert rng.next_call == 4


def test_default_keyed_generators_differ(eng):
    from protocols.distributed_keygen_amd.device_rng import DeviceRng

    a, b = DeviceRng(), DeviceRng()
    ra, rb = host_rows(eng, a.rows_t(eng, 4, 256)), host_rows(eng, b.rows_t(eng, 4, 256))
    assert ra != rb and a.next_call == b.next_call == 1
    assert any(v for row in ra for v in row)


# ---- FastRandomizer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_length", [128, 1024])
def test_fast_randomizer_with_a_device_generator(eng, key_length):
    from protocols.distributed_keygen_amd import randomizer, synthetic

    key = synthetic.make_key(key_length, 3, 1)
    n, n2 = key.n, key.n_square
    rnd = random.Random(key_length)
    h_s = randomizer.generate_base(n, rng=rnd, engine=eng)
    explicit = randomizer.FastRandomizer(n, h_s, engine=eng)
    call = 100
    fr = randomizer.FastRandomizer(n, h_s, engine=eng, device_rng=make_rng(call))
    eb = fr.exp_bits
    for count in (1, 5, 257):
        msgs = ([0, -1, n - 1] + [rnd.randrange(n) for _ in range(count)])[:count]
        cts = ([1, n2 - 1, n] + [rnd.randrange(n2) for _ in range(count)])[:count]
        a = cm.row_ints(KEY, call, count, eb)
        got = fr.encrypt(msgs)
        assert got == explicit.encrypt(msgs, exponents=a)
        assert got == [(1 + (m % n) * n) * pow(h_s, x, n2) % n2 for m, x in zip(msgs, a)]
        a = cm.row_ints(KEY, call + 1, count, eb)
        got = fr.randomize(cts)
        assert got == explicit.randomize(cts, exponents=a)
        assert got == [c * pow(h_s, x, n2) % n2 for c, x in zip(cts, a)]
        a = cm.row_ints(KEY, call + 2, count, eb)
        got = fr.randomizers(count)
        assert got == explicit.randomizers(count, exponents=a)
        assert got == [pow(h_s, x, n2) for x in a]
        call += 3
    assert fr.device_rng.next_call == call
    # explicit exponents win and spend no call number
    assert fr.encrypt([5], exponents=[3]) == [(1 + 5 * n) * pow(h_s, 3, n2) % n2] and fr.device_rng.next_call == call
    # device rows of the wrong shape, type or device are refused
    import torch

    with pytest.raises(ValueError):
        eng.fixed_base_exponent_rows(torch.zeros((2, -(-eb // 32) + 1), dtype=torch.int32, device=eng.device), eb)
    with pytest.raises(ValueError):
        eng.fixed_base_exponent_rows(torch.zeros((2, -(-eb // 32)), dtype=torch.int64, device=eng.device), eb)
    with pytest.raises(ValueError):
        eng.fixed_base_exponent_rows(torch.zeros((2, -(-eb // 32)), dtype=torch.int32), eb)          # host memory


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


def test_linear_map_and_pack_are_freshened_with_device_drawn_exponents(eng):
    from protocols.distributed_keygen_amd import homomorphic, packing, randomizer, synthetic

    key = synthetic.make_key(1024, 3, 1)
    n, n2 = key.n, key.n_square
    rnd = random.Random(77)
    h_s = randomizer.generate_base(n, rng=rnd, engine=eng)
    fr = randomizer.FastRandomizer(n, h_s, engine=eng, device_rng=make_rng(500))
    eb = fr.exp_bits
    x = [rnd.randrange(-1000, 1000) for _ in range(12)]
    W = [[rnd.randrange(-50, 50) for _ in x] for _ in range(7)]
    b = [rnd.randrange(-10**6, 10**6) for _ in W]
    cts = fr.encrypt(x)                                                            # call 500
    plain = homomorphic.linear_map(cts, W, n=n, bias=b, engine=eng)
    fresh = homomorphic.linear_map(cts, W, n=n, bias=b, engine=eng, randomizer=fr)   # call 501
    assert fresh == [c * pow(h_s, a, n2) % n2 for c, a in zip(plain, cm.row_ints(KEY, 501, len(W), eb))]
    want = [(sum(w * v for w, v in zip(row, x)) + bj) % n for row, bj in zip(W, b)]
    assert threshold_decrypt(eng, key, fresh) == want

    vals = [rnd.randrange(1 << 16) for _ in range(100)]
    cts = fr.encrypt(vals)                                                         # call 502
    packed_plain = packing.pack(cts, 16, n=n, engine=eng)
    packed = packing.pack(cts, 16, n=n, engine=eng, randomizer=fr)                 # call 503
    assert len(packed) == -(-len(vals) // packing.slots_per_ciphertext(n, 16)) >= 2
    assert packed == [c * pow(h_s, a, n2) % n2 for c, a in zip(packed_plain, cm.row_ints(KEY, 503, len(packed), eb))]
    assert packing.unpack(threshold_decrypt(eng, key, packed), 16, len(vals), n, signed=False) == vals      # vals fill [0, 2^16)
    assert fr.device_rng.next_call == 504


# ---- reference-style randomness r^N -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key_length", [128, 1024])
def test_fresh_batches_use_device_drawn_randomness(eng, key_length):
    from protocols.distributed_keygen_amd import limbs, synthetic

    key = synthetic.make_key(key_length, 3, 1)
    n, n2 = key.n, key.n_square
    rnd = random.Random(key_length + 1)
    rng = make_rng(900)
    r_bits, l2 = n.bit_length() + 64, limbs.limbs_for(n2)
    msgs = [0, 1, n - 1, -7, 424242] + [rnd.randrange(n) for _ in range(60)]
    out, r = eng.encrypt_fresh_batch(msgs, n, rng, return_randomness=True)
    assert r == cm.row_ints(KEY, 900, len(msgs), r_bits, l2)
    assert any(v >= n for v in r) and all(v < 1 << r_bits for v in r)
    assert out == [(1 + (m % n) * n) * pow(v % n, n, n2) % n2 for m, v in zip(msgs, r)]
    assert threshold_decrypt(eng, key, out[:5]) == [m % n for m in msgs[:5]]
    plain = eng.encrypt_fresh_batch(msgs, n, rng)                                  # call 901
    assert plain == [(1 + (m % n) * n) * pow(v % n, n, n2) % n2 for m, v in zip(msgs, cm.row_ints(KEY, 901, len(msgs), r_bits, l2))]
    # the same randomness through the entry point that takes r as ints
    assert plain == eng.encrypt_batch(msgs, [v % n for v in cm.row_ints(KEY, 901, len(msgs), r_bits, l2)], n)
    cts = [out[0], n2 + 5, -3] + out[3:20]
    again, r2 = eng.randomize_fresh_batch(cts, n, rng, return_randomness=True)      # call 902
    assert r2 == cm.row_ints(KEY, 902, len(cts), r_bits, l2)
    assert again == [c % n2 * pow(v % n, n, n2) % n2 for c, v in zip(cts, r2)]
    assert eng.randomize_fresh_batch(cts, n, rng) != again and rng.next_call == 904
    assert eng.encrypt_fresh_batch([], n, rng) == [] and eng.randomize_fresh_batch([], n, rng, return_randomness=True) == ([], [])
    assert rng.next_call == 904


def test_a_modulus_too_small_for_64_extra_bits_is_refused(eng):
    rng = make_rng()
    for bits in (20, 40, 64):
        n = random.Random(bits).getrandbits(bits) | (1 << (bits - 1)) | 1
        assert n.bit_length() + 64 > (n * n).bit_length() - 1
        with pytest.raises(ValueError):
            eng.encrypt_fresh_batch([1, 2], n, rng)
        with pytest.raises(ValueError):
            eng.randomize_fresh_batch([1, 2], n, rng)
    assert rng.next_call == 0
