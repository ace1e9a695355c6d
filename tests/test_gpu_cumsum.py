"""Encrypted prefix sums on the GPU (csrc/mx_scan_n2.hpp, Engine.cumsum_nsquare_t, homomorphic.cumsum), bit-exact
against a Python loop of ``acc = acc * c % n2``."""

from __future__ import annotations

import ctypes
import itertools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 16, 17, 0, 33, 10]          # 77 ciphertexts; the library's chunk for them is their mean, 11: one to three pieces
FORMS = list(itertools.product((False, True), (False, True)))


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


def odd_modulus(bits: int, rng: random.Random) -> int:
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def key_n(key_length: int) -> int:
    from protocols.distributed_keygen_amd import synthetic

    return synthetic.make_key(key_length, 3, 1).n


def want_cumsum(cts, lengths, n, exclusive=False, reverse=False):
    n2 = n * n
    out, lo = [], 0
    for k in lengths:
        seg = [c % n2 for c in cts[lo : lo + k]]
        lo += k
        if reverse:
            seg.reverse()
        res, acc = [], 1
        for c in seg:
            if exclusive:
                res.append(acc)
            acc = acc * c % n2
            if not exclusive:
                res.append(acc)
        if reverse:
            res.reverse()
        out += res
    return out


_cases = {}


def parity_case(key_length):
    """77 ciphertexts in segments of LENGTHS.  A 0 in the middle of the 33-segment (prefixes before it are not zero, after
    it zero), 1, N^2 - 1, a multiple of N (no inverse), a value >= N^2 (reduced on upload) and a duplicate.  The four
    references are computed once per modulus and shared by the tests below."""
    if key_length not in _cases:
        rng = random.Random(f"cumsum {key_length}")
        n = key_n(key_length) if key_length != "odd" else odd_modulus(1531, rng)
        n2 = n * n
        cts = [rng.randrange(1, n2) for _ in range(77)]
        cts[34 + 12] = 0                                               # the 33-segment is elements 34 .. 66
        cts[2], cts[5], cts[20], cts[40] = 1, n2 - 1, 12345 * n, n2 + 99
        cts[70] = cts[69]
        want = {form: want_cumsum(cts, LENGTHS, n, *form) for form in FORMS}
        _cases[key_length] = (n, cts, want)
    return _cases[key_length]


@pytest.mark.parametrize("key_length", [128, 2048, "odd"])
def test_matches_a_loop_of_plain_products(eng, key_length):
    n, cts, want = parity_case(key_length)
    inc = want[(False, False)]
    assert inc[34 + 11] != 0 and inc[34 + 12 : 67] == [0] * 21 and inc[67] != 0       # the zero is in the case, and stays in its segment
    for exclusive, reverse in FORMS:
        assert eng.ciphertext_cumsum_batch(cts, LENGTHS, n, exclusive=exclusive, reverse=reverse) == want[(exclusive, reverse)]
    assert eng.ciphertext_cumsum_batch(cts, np.array(LENGTHS), n) == inc
    for exclusive, reverse in FORMS:                                   # lengths=None: one series of 77
        assert eng.ciphertext_cumsum_batch(cts, None, n, exclusive=exclusive, reverse=reverse) == want_cumsum(cts, [77], n, exclusive, reverse)


@pytest.mark.parametrize("key_length", [128, 2048, "odd"])
def test_chunk_and_budget_overrides_change_nothing(eng, key_length):
    from protocols.distributed_keygen_amd import limbs

    n, cts, want = parity_case(key_length)
    n2 = n * n
    x_t = eng.to_device(limbs.pack_reduced(cts, limbs.limbs_for(n2), n2))

    def run(form, **kw):
        return limbs.unpack(eng.to_host(eng.cumsum_nsquare_t(x_t, LENGTHS, n, exclusive=form[0], reverse=form[1], **kw)))

    for chunk in (1, 2, 0, 1000):
        for form in FORMS:
            assert run(form, chunk=chunk) == want[form], (chunk, form)
    row_bytes = eng.histogram_nsquare_shape(n, 77, 7, 77)[3]
    budget = 5 * (row_bytes + 4)                                       # five rows a stage: stages end inside the segments
    for form in FORMS:
        assert run(form, table_budget_bytes=budget) == want[form], form
        assert run(form, chunk=3, table_budget_bytes=budget) == want[form], form
    assert run(FORMS[0], table_budget_bytes=1) == want[FORMS[0]]       # every element a stage of its own


def test_every_instance_has_a_parity_case(eng):
    from protocols.distributed_keygen_amd import limbs

    lib = eng.lib
    cnt = lib.mx_scan_nsquare_instances(None, None, 0)
    lanes, lpls = (ctypes.c_int * cnt)(), (ctypes.c_int * cnt)()
    assert lib.mx_scan_nsquare_instances(lanes, lpls, cnt) == cnt
    want = {(lanes[i], lpls[i]) for i in range(cnt)}
    rng = random.Random(19)
    seen = set()
    lengths = [13, 7]
    for bits in (130, 200, 400, 900, 2000, 3000, 4000, 6000, 8000):
        n = odd_modulus(bits, rng)
        n2 = n * n
        seen.add(eng.histogram_nsquare_shape(n, 20, 2, 20)[:2])
        cts = [rng.randrange(n2) for _ in range(18)] + [n2 + 3, 7 * n]
        x_t = eng.to_device(limbs.pack_reduced(cts, limbs.limbs_for(n2), n2))
        for exclusive, reverse in ((False, False), (True, True)):
            got = limbs.unpack(eng.to_host(eng.cumsum_nsquare_t(x_t, lengths, n, exclusive=exclusive, reverse=reverse, chunk=3)))
            assert got == want_cumsum(cts, lengths, n, exclusive, reverse), (bits, exclusive, reverse)
    assert seen == want


def test_device_resident_form_and_two_streams(eng):
    import torch

    from protocols.distributed_keygen_amd import limbs

    n, cts, want = parity_case(2048)
    n2 = n * n
    x_t = eng.to_device(limbs.pack_reduced(cts, limbs.limbs_for(n2), n2))
    y_t = eng.to_device(limbs.pack_reduced(cts[::-1], limbs.limbs_for(n2), n2))   # other inputs: the series turned round
    lengths_t = torch.tensor(LENGTHS, dtype=torch.int32, device=eng.device)
    out_t = eng.cumsum_nsquare_t(x_t, lengths_t, n)
    assert out_t.is_cuda and out_t.dtype == torch.int32 and tuple(out_t.shape) == tuple(x_t.shape)
    assert torch.equal(out_t, eng.to_device(limbs.pack(want[(False, False)], x_t.shape[1])))      # canonical residues
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    a_t = eng.cumsum_nsquare_t(x_t, lengths_t, n, chunk=2)                        # several levels in flight on this stream ...
    with torch.cuda.stream(side):
        b_t = eng.cumsum_nsquare_t(y_t, None, n, reverse=True, chunk=2)           # ... while the side stream runs its own
    cur.wait_stream(side)
    assert limbs.unpack(eng.to_host(a_t)) == want[(False, False)]
    assert limbs.unpack(eng.to_host(b_t)) == want_cumsum(cts[::-1], [77], n, reverse=True)


def test_refusals_and_empty_shapes(eng):
    import torch

    from protocols.distributed_keygen_amd import limbs

    n = key_n(128)
    n2 = n * n
    cts = [3, 5, 7]
    x_t = eng.to_device(limbs.pack(cts, limbs.limbs_for(n2)))
    for lengths in ([2, 2], [4, -1], [1.5, 1.5], [[3]], torch.ones(3, device=eng.device), torch.tensor([[3]], device=eng.device)):
        with pytest.raises(ValueError):
            eng.ciphertext_cumsum_batch(cts, lengths, n)
        with pytest.raises(ValueError):
            eng.cumsum_nsquare_t(x_t, lengths, n)
    with pytest.raises(ValueError):
        eng.ciphertext_cumsum_batch(cts, None, n + 1)                             # an even modulus
    with pytest.raises(ValueError):
        eng.cumsum_nsquare_t(x_t, None, n, chunk=1 << 20)
    assert eng.ciphertext_cumsum_batch([], [], n) == [] and eng.ciphertext_cumsum_batch([], [0, 0], n) == []
    assert tuple(eng.cumsum_nsquare_t(x_t[:0], [0], n).shape) == (0, x_t.shape[1])
    assert eng.ciphertext_cumsum_batch(cts, [0, 3, 0], n) == [3, 15, 105]
    assert eng.ciphertext_cumsum_batch([5, 7 * n, 0, 9], [4], n, exclusive=True) == [1, 5, 35 * n % n2, 0]   # no inverse needed


def test_cumsum_of_histogram_rows(eng):
    """The split sums of a boosted tree: G_L and G_R of every threshold from the histogram's own output, as a nested call."""
    from protocols.distributed_keygen_amd import homomorphic

    n = key_n(2048)
    n2 = n * n
    rng = random.Random(47)
    cts = [rng.randrange(1, n2) for _ in range(60)]
    bins = [[rng.randrange(-1, 8) for _ in cts] for _ in range(3)]
    hist = homomorphic.histogram(cts, bins, 8, n=n, engine=eng)
    left = homomorphic.cumsum(hist, n, engine=eng)
    right = homomorphic.cumsum(hist, n, reverse=True, engine=eng)
    assert left == [want_cumsum(row, [8], n) for row in hist]
    assert right == [want_cumsum(row, [8], n, reverse=True) for row in hist]
    assert all(l[-1] == r[0] for l, r in zip(left, right))                        # both ends hold the feature's total
    totals = [1, 1, 1]
    for f, row in enumerate(bins):
        for c, b in zip(cts, row):
            if b >= 0:
                totals[f] = totals[f] * c % n2
    assert [l[-1] for l in left] == totals


class _Given:
    """A FastRandomizer whose next draw is a given list of exponents."""

    def __init__(self, fr, exps):
        self.fr, self.exps = fr, list(exps)

    def spec(self, n, count):
        return self.fr.spec(n, count, exponents=self.exps)


def _decryptor(key, eng):
    from protocols.distributed_keygen_amd.shared_key import GpuPaillierSharedKey, PlainCiphertext, ShareView

    n = key.n
    keys = {i: GpuPaillierSharedKey(n, key.t, i, ShareView({i: key.shares[i]}, key.degree, key.n_fac), key.theta, engine=eng)
            for i in (1, 2, 3)}

    def decrypt(values):
        parts = {i: k.partial_decrypt_batch([PlainCiphertext(c, n) for c in values]) for i, k in keys.items()}
        return keys[1].decrypt_batch([{i: parts[i][e] for i in keys} for e in range(len(values))])
    return decrypt


def test_running_totals_round_trip_and_randomizer(eng):
    """Small ints under a 128-bit key: encrypt, cumsum, threshold decryption by three parties, against numpy.cumsum; then
    with a randomiser: other residues, the same plaintexts."""
    from protocols.distributed_keygen_amd import homomorphic, randomizer, synthetic

    key = synthetic.make_key(128, 3, 1)
    n = key.n
    n2 = n * n
    rng = random.Random(53)
    lengths = [40, 0, 23, 1]
    values = np.random.default_rng(53).integers(0, 1000, size=sum(lengths))
    decrypt = _decryptor(key, eng)
    cts = eng.encrypt_batch([int(v) for v in values], [rng.randrange(1, n) for _ in values], n)
    nested, lo = [], 0
    for k in lengths:
        nested.append(cts[lo : lo + k])
        lo += k
    want = [int(v) for a, b in ((0, 40), (40, 63), (63, 64)) for v in np.cumsum(values[a:b])]
    plain = homomorphic.cumsum(nested, n, engine=eng)
    assert [len(p) for p in plain] == lengths
    flat = [v for p in plain for v in p]
    assert decrypt(flat) == want
    back = homomorphic.cumsum(cts, n, reverse=True, exclusive=True, engine=eng)
    assert decrypt(back) == [int(values[j + 1 :].sum()) for j in range(len(values))]
    h_s = randomizer.generate_base(n, rng=rng, engine=eng)
    fr = randomizer.FastRandomizer(n, h_s, engine=eng)
    exps = [rng.getrandbits(fr.exp_bits) for _ in flat]
    fresh = homomorphic.cumsum(nested, n, engine=eng, randomizer=_Given(fr, exps))
    assert [v for p in fresh for v in p] == [v * pow(h_s, a, n2) % n2 for v, a in zip(flat, exps)]
    drawn = [v for p in homomorphic.cumsum(nested, n, engine=eng, randomizer=fr) for v in p]
    assert all(u != v for u, v in zip(drawn, flat))
    assert decrypt(drawn) == want
