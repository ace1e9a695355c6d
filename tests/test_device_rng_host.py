"""Host logic of the device random-row generator on the CPU: the model of the kernel (tools/chacha_model.py) against
RFC 8439, the nonce discipline of device_rng.DeviceRng against a recording engine, and what FastRandomizer does with and
without a device generator (the recording pure-Python engine of tests/rng_engine.py)."""

from __future__ import annotations

import ctypes
import os
import select
import signal
import threading

import numpy as np
import pytest

from rng_engine import ByteSource, DeviceRows, RecordingEngine, cm, exponent_ints

from protocols.distributed_keygen_amd import device_rng, homomorphic, packing, randomizer, synthetic
from protocols.distributed_keygen_amd.device_rng import DeviceRng

RFC_KEY = bytes(range(32))
RFC_NONCE = bytes.fromhex("000000090000004a00000000")
# RFC 8439 §2.3.2, "Serialized Block"
RFC_BLOCK = bytes.fromhex(
    "10f1e7e4d13b5915500fdd1fa32071c4" "c7d1f4c733c068030422aa9ac3d46c4e"
    "d2826446079faa0914c2d705d98b02a2" "b5129cd1de164eb9cbd083e8a2503c4e")
KEY = bytes((7 * k + 3) & 0xFF for k in range(32))


def call_number(nonce):
    return nonce[0] | nonce[1] << 32 | nonce[2] << 64


def test_model_block_is_the_rfc_8439_vector():
    assert cm.block_bytes(RFC_KEY, 1, RFC_NONCE) == RFC_BLOCK
    assert RFC_BLOCK[:16].hex() == "10f1e7e4d13b5915500fdd1fa32071c4" and RFC_BLOCK[-4:].hex() == "a2503c4e"
    # §2.3.2's state after the rounds and the addition, first and last word
    words = cm.block(cm.key_words(RFC_KEY), 1, [0x09000000, 0x4A000000, 0])
    assert (words[0], words[15]) == (0xE4E7F110, 0x4E3C50A2)


@pytest.mark.parametrize("shape", [(1, 32, 1), (1, 512, 16), (5, 96, 3), (7, 1026, 33), (3, 195, 9), (40, 33, 2)])
def test_model_rows_follow_the_mapping(shape):
    count, bits, row_words = shape
    w = -(-bits // 32)
    rows = cm.rows(KEY, 5, count, bits, row_words)
    stream = [v for b in range(-(-count * w // 16)) for v in cm.block(cm.key_words(KEY), b, cm.nonce_words(5))]
    for r, row in enumerate(rows):
        assert len(row) == row_words and row[w:] == [0] * (row_words - w)
        for j in range(w):
            mask = (1 << (bits % 32)) - 1 if j == w - 1 and bits % 32 else 0xFFFFFFFF
            assert row[j] == stream[r * w + j] & mask
    assert cm.row_ints(KEY, 5, count, bits, row_words) == [int.from_bytes(np.array(r, dtype="<u4").tobytes(), "little") for r in rows]
    assert all(v < 1 << bits for v in cm.row_ints(KEY, 5, count, bits, row_words))
    assert cm.nonce_words((3 << 64) | (2 << 32) | 1) == [1, 2, 3]


def test_successive_calls_take_successive_nonces_and_start_at_block_zero():
    eng = RecordingEngine()
    first = (1 << 64) - 2                       # the counter carries into the third nonce word
    rng = DeviceRng(key=KEY, first_call=first)
    outs = [rng.rows_t(eng, 3, 70), rng.rows_t(eng, 3, 70), rng.rows_t(eng, 2, 40, row_words=4), rng.rows_t(eng, 0, 8)]
    calls = eng.chacha_calls()
    assert [call_number(c[2]) for c in calls] == [first, first + 1, first + 2, first + 3]
    assert calls[2][2] == (0, 0, 1)
    assert all(c[1] == tuple(cm.key_words(KEY)) and c[3] == 0 for c in calls)
    assert [c[4:] for c in calls] == [(3, 70, 3), (3, 70, 3), (2, 40, 4), (0, 8, 1)]
    assert rng.next_call == first + 4
    assert outs[0].tolist() == cm.rows(KEY, first, 3, 70) and outs[1].tolist() == cm.rows(KEY, first + 1, 3, 70)
    assert outs[0].tolist() != outs[1].tolist()
    assert outs[2].tolist() == cm.rows(KEY, first + 2, 2, 40, 4) and outs[3].shape == (0, 1)


def test_threads_never_share_a_nonce():
    eng = RecordingEngine()
    rng = DeviceRng(key=KEY, first_call=1000)

    def work():
        for _ in range(50):
            rng.rows_t(eng, 1, 32)

    threads = [threading.Thread(target=work) for _ in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    nonces = [call_number(c[2]) for c in eng.chacha_calls()]
    assert len(nonces) == 400 and sorted(nonces) == list(range(1000, 1400))


def test_a_changed_pid_draws_a_new_key(monkeypatch):
    eng = RecordingEngine()
    rng = DeviceRng(key=KEY)
    rng.rows_t(eng, 1, 32)
    pid = os.getpid()
    monkeypatch.setattr(os, "getpid", lambda: pid + 1)          # "the forked child"
    rng.rows_t(eng, 1, 32)
    rng.rows_t(eng, 1, 32)
    keys = [c[1] for c in eng.chacha_calls()]
    assert keys[0] == tuple(cm.key_words(KEY))
    assert keys[1] != keys[0] and keys[2] == keys[1]            # one new key, kept from then on
    assert [call_number(c[2]) for c in eng.chacha_calls()] == [0, 1, 2]


@pytest.mark.skipif(not hasattr(os, "register_at_fork"), reason="no fork on this platform")
def test_a_forked_child_gets_a_new_key_and_a_free_lock():
    """A real fork taken while the generator's lock is held, as by another thread of the parent inside rows_t: the child
    re-keys at the fork and its first call neither blocks nor repeats the parent's stream."""
    rng = DeviceRng(key=KEY, first_call=5)
    parent_key = tuple(cm.key_words(KEY))
    rd, wr = os.pipe()
    rng._lock.acquire()
    try:
        pid = os.fork()
        if pid == 0:                                            # the child: report (key words, nonce) and leave
            try:
                eng = RecordingEngine()
                rng.rows_t(eng, 1, 32)
                call = eng.chacha_calls()[0]
                os.write(wr, repr((call[1], call[2])).encode())
            finally:
                os._exit(0)
    finally:
        rng._lock.release()
    os.close(wr)
    ready, _, _ = select.select([rd], [], [], 20)
    if not ready:
        os.kill(pid, signal.SIGKILL)
    os.waitpid(pid, 0)
    assert ready, "the child blocked on the lock it inherited"
    child_key, child_nonce = eval(os.read(rd, 4096).decode())
    os.close(rd)
    assert len(child_key) == 8 and child_key != parent_key and child_nonce == (5, 0, 0)
    eng = RecordingEngine()                                     # the parent goes on with its own key and counter
    rng.rows_t(eng, 1, 32)
    assert eng.chacha_calls()[0][1:3] == (parent_key, (5, 0, 0))


def test_collected_generators_leave_the_fork_hook():
    before = len(device_rng._live)
    rng = DeviceRng()
    assert len(device_rng._live) == before + 1
    del rng
    assert len(device_rng._live) == before


def test_default_keys_differ_between_objects():
    eng = RecordingEngine()
    DeviceRng().rows_t(eng, 1, 32)
    DeviceRng().rows_t(eng, 1, 32)
    a, b = eng.chacha_calls()
    assert a[1] != b[1] and a[2] == b[2] == (0, 0, 0)


def test_refused_requests_raise_before_anything_is_launched():
    eng = RecordingEngine()
    for bad in (b"", bytes(31), bytes(33)):
        with pytest.raises(ValueError):
            DeviceRng(key=bad)
    with pytest.raises(ValueError):
        DeviceRng(key=KEY, first_call=-1)
    with pytest.raises(ValueError):
        DeviceRng(key=KEY, first_call=1 << 96)
    rng = DeviceRng(key=KEY, first_call=9)
    for count, bits, row_words in (((1 << 36) + 1, 32, None), ((1 << 31) + 1, 1024, None), (-1, 32, None), (1, 0, None), (1, 65, 2)):
        with pytest.raises(ValueError):
            rng.rows_t(eng, count, bits, row_words)
    assert eng.calls == [] and rng.next_call == 9                # nothing launched, no call number spent


def test_repr_and_errors_do_not_show_the_key():
    secret = bytes.fromhex("a1b2c3d4e5f60718293a4b5c6d7e8f90" "0f1e2d3c4b5a69788796a5b4c3d2e1f0")
    rng = DeviceRng(key=secret, first_call=41)
    shown = [repr(rng), str(rng)]
    with pytest.raises(ValueError) as err:
        rng.rows_t(RecordingEngine(), (1 << 36) + 1, 32)
    shown.append(str(err.value))
    words = cm.key_words(secret)
    for text in shown:
        low = text.lower()
        assert secret.hex()[:8] not in low and secret.hex()[-8:] not in low
        assert not any(f"{w:x}" in low or str(w) in low for w in words)
    assert "41" in repr(rng)


def _operations(fr):
    return [fr.randomizers(5), fr.encrypt([1, 2, 3]), fr.randomize([4, 5]), list(fr.spec(fr.n, 4)[4].tolist())]


def test_without_a_device_generator_the_randomizer_issues_the_calls_it_issues_today():
    key = synthetic.make_key(128)
    runs = []
    for kwargs in ({}, {"device_rng": None}):
        eng, src = RecordingEngine(), ByteSource(3)
        fr = randomizer.FastRandomizer(key.n, 5, engine=eng, urandom=src, **kwargs)
        assert fr.device_rng is None
        runs.append((_operations(fr), eng.calls, eng.exponent_kinds, src.asked))
    assert runs[0] == runs[1]
    nbytes = -(-((key.n.bit_length() + 1) // 2) // 8)
    assert runs[0][3] == [5 * nbytes, 3 * nbytes, 2 * nbytes, 4 * nbytes]
    assert [c[0] for c in runs[0][1]] == ["power", "encrypt", "randomize"] and runs[0][2] == ["host"] * 3


def test_with_a_device_generator_exponents_are_drawn_on_the_engine_and_nothing_is_uploaded():
    key = synthetic.make_key(128)
    n, n2 = key.n, key.n_square
    eng, src = RecordingEngine(), ByteSource(4)
    fr = randomizer.FastRandomizer(n, 5, engine=eng, urandom=src, device_rng=DeviceRng(key=KEY, first_call=7))
    eb = fr.exp_bits
    assert fr.randomizers(5) == [pow(5, a, n2) for a in cm.row_ints(KEY, 7, 5, eb)]
    assert fr.encrypt([1, 2, -3]) == [(1 + (m % n) * n) * pow(5, a, n2) % n2 for m, a in zip([1, 2, -3], cm.row_ints(KEY, 8, 3, eb))]
    assert fr.randomize([4, 5]) == [c * pow(5, a, n2) % n2 for c, a in zip([4, 5], cm.row_ints(KEY, 9, 2, eb))]
    spec = fr.spec(n, 4)
    assert spec[:4] == (n, 5, eb, 0) and isinstance(spec[4], DeviceRows) and exponent_ints(spec[4]) == cm.row_ints(KEY, 10, 4, eb)
    assert src.asked == []                                       # no host bytes
    assert eng.exponent_kinds == ["device"] * 3                  # no rows to upload
    assert [c[0] for c in eng.calls] == ["chacha", "power", "chacha", "encrypt", "chacha", "randomize", "chacha"]
    assert [c[4:] for c in eng.chacha_calls()] == [(k, eb, -(-eb // 32)) for k in (5, 3, 2, 4)]
    # the path of homomorphic.* and packing.pack
    cts = [synthetic.encrypt(key, m, __import__("random").Random(1)) for m in (3, 4, 5, 6)]
    plain = homomorphic.linear_map(cts, [[1, 2, 0, 0], [0, 0, 3, -1]], n=n, engine=eng)
    fresh = homomorphic.linear_map(cts, [[1, 2, 0, 0], [0, 0, 3, -1]], n=n, engine=eng, randomizer=fr)
    assert fresh == [c * pow(5, a, n2) % n2 for c, a in zip(plain, cm.row_ints(KEY, 11, 2, eb))]
    packed = packing.pack(cts, 20, n=n, engine=eng, randomizer=fr)
    assert packed == [c * pow(5, a, n2) % n2 for c, a in zip(packing.pack(cts, 20, n=n, engine=eng), cm.row_ints(KEY, 12, len(packed), eb))]
    assert src.asked == [] and set(eng.exponent_kinds) == {"device"}
    # draw() stays the host draw
    assert fr.draw(2).shape == (2, -(-eb // 32)) and src.asked == [2 * -(-eb // 8)]


def test_explicit_exponents_bypass_the_generator():
    key = synthetic.make_key(128)
    n, n2 = key.n, key.n_square
    eng = RecordingEngine()
    rng = DeviceRng(key=KEY)
    fr = randomizer.FastRandomizer(n, 5, engine=eng, device_rng=rng)
    assert fr.encrypt([9, 8], exponents=[3, 4]) == [(1 + 9 * n) * 125 % n2, (1 + 8 * n) * 625 % n2]
    assert fr.randomizers(1, exponents=[2]) == [25] and fr.randomize([7], exponents=[1]) == [35]
    assert fr.spec(n, 2, exponents=[1, 2])[4] == [1, 2]
    assert eng.chacha_calls() == [] and rng.next_call == 0 and eng.exponent_kinds == ["ints"] * 3
    with pytest.raises(ValueError):
        fr.encrypt([1], exponents=[1 << fr.exp_bits])


def test_device_rng_true_makes_a_generator_of_its_own():
    key = synthetic.make_key(128)
    a = randomizer.FastRandomizer(key.n, 5, engine=RecordingEngine(), device_rng=True)
    b = randomizer.FastRandomizer(key.n, 5, engine=RecordingEngine(), device_rng=True)
    assert isinstance(a.device_rng, DeviceRng) and a.device_rng is not b.device_rng
    assert a.randomizers(2) != b.randomizers(2)


def test_abi_refuses_bad_arguments_without_a_launch():
    """mx_chacha20_rows validates before it touches the runtime: every refusal, and count = 0, on a machine without a GPU."""
    from protocols.distributed_keygen_amd import _lib

    lib = _lib.lib()
    key, nonce = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 3)()
    out = (ctypes.c_uint32 * 4)()                                # never written: every call below returns before a launch
    ok = (key, nonce, 0, out, 1, 1, 32, None)
    refused = [
        (None, *ok[1:]), (key, None, *ok[2:]), (*ok[:3], None, *ok[4:]),
        (*ok[:4], -1, 1, 32, None),                              # count < 0
        (*ok[:4], 1, 1, 0, None), (*ok[:4], 1, 1, -5, None),     # bits < 1
        (*ok[:4], 1, 1, 33, None), (*ok[:4], 1, 2, 65, None),    # bits > 32 * row_words
        (key, nonce, 1, out, 1 << 36, 1, 32, None),              # counter0 + blocks > 2^32
        (key, nonce, 0xFFFFFFFF, out, 17, 1, 32, None),
        (key, nonce, 0, out, (1 << 36) + 1, 1, 32, None),
        (key, nonce, 0, out, 1 << 62, 64, 2048, None),           # count * w overflows 64 bits' worth of words
    ]
    for args in refused:
        assert lib.mx_chacha20_rows(*args) == -1, args[2:]
    assert lib.mx_chacha20_rows(key, nonce, 0xFFFFFFFF, out, 0, 1, 32, None) == 0          # count = 0: MX_OK, no launch
    assert lib.mx_version() == 404
