"""Private-key (CRT) decryption on the GPU (csrc/mx_crt.hpp, Engine.crt_split_t / crt_recombine_t / private_decrypt_t,
private_key.PaillierPrivateKey), every stage bit for bit against Python ints: the split against ``%``, the recombination
against the formulas on GIVEN x rows, and the whole route against known plaintexts and ``pow(c, lambda, N^2)``.

Keys: synthetic.make_key at 128 (p > q), 1024 and 2048 (p < q) and 4096 (8 rows) — the primes of the three long ones are
kept in tests/golden/private_key_primes.json, finding them again costs ten seconds — and one hand-made key with primes of 64
and 67 bits (limbs(p^2) = 4, limbs(q^2) = 5); every key also with (q, p) swapped.  Batches of 1, 2, 63, 64, 65 and 151 rows
are prefixes of one list of 151 rows per stage, so the reference of a stage is computed once.  Invalid ciphertexts are
ordinary data with a status."""

from __future__ import annotations

import importlib.util
import json
import math
import random
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import crt_model as cm  # noqa: E402

BATCHES = (1, 2, 63, 64, 65, 151)
NAMES = ("k128", "k1024", "k2048", "k4096", "k64_67")
CASES = [(name, swapped) for name in NAMES for swapped in (False, True)]


class Key:
    """p, q and one randomiser s = r^N mod N^2 (the one full-length pow per key: other randomisers are its powers)."""

    def __init__(self, p, q, seed):
        self.p, self.q, self.n = p, q, p * q
        self.n2 = self.n * self.n
        self.rng = random.Random(seed)
        self.s = pow(self.rng.randrange(2, self.n), self.n, self.n2)
        self.rows = 8 if self.n.bit_length() > 4000 else 151
        self.batches = (8,) if self.rows == 8 else BATCHES

    def encrypt_all(self, msgs):
        out, r = [], 1
        for m in msgs:
            r = r * self.s % self.n2
            out.append((1 + m * self.n) * r % self.n2)
        return out

    def primes(self, swapped):
        return (self.q, self.p) if swapped else (self.p, self.q)


@pytest.fixture(scope="module")
def eng():
    from protocols.distributed_keygen_amd import Engine

    return Engine(0)


@pytest.fixture(scope="module")
def keys():
    from protocols.distributed_keygen_amd import synthetic

    gold = json.loads((ROOT / "tests" / "golden" / "private_key_primes.json").read_text())["keys"]
    k128 = synthetic.make_key(128)
    out = {"k128": Key(k128.p, k128.q, 1), "k64_67": Key(*cm.key_of_bits(64, 67), 5)}
    for kl in (1024, 2048, 4096):
        out[f"k{kl}"] = Key(int(gold[str(kl)]["p"], 16), int(gold[str(kl)]["q"], 16), kl)
    assert out["k128"].p > out["k128"].q and out["k1024"].p < out["k1024"].q
    assert (out["k64_67"].p.bit_length(), out["k64_67"].q.bit_length()) == (64, 67)
    return out


def rows_of(eng, values, width):
    from protocols.distributed_keygen_amd import limbs

    return eng.to_device(limbs.pack(values, width))


def ints_of(eng, rows_t):
    from protocols.distributed_keygen_amd import limbs

    return limbs.unpack(eng.to_host(rows_t))


def fill(values, count, make):
    return (values + [make() for _ in range(max(0, count - len(values)))])[:count]


# ------------------------------------------------------------------ the split
@pytest.mark.parametrize("name,swapped", CASES)
def test_split_against_percent(eng, keys, name, swapped):
    from protocols.distributed_keygen_amd import limbs

    key = keys[name]
    p, q = key.primes(swapped)
    rng = random.Random(7)
    l2 = limbs.limbs_for(key.n2)
    top = 1 << (32 * l2)
    edge = [0, 1, key.n2 - 1, top - 1, rng.getrandbits(31), 5, 3 * p * p, (top - 1) // (p * p) * (p * p), 2 * q * q + 1,
            (top - 1) // (q * q) * (q * q) + 1, key.n2, rng.getrandbits(32 * l2)]
    if key.rows == 8:
        edge = [edge[k] for k in (0, 2, 3, 4, 7, 9, 11)]
    cts = fill(edge, key.rows, lambda: rng.randrange(key.n2))
    want = [[c % (p * p) for c in cts], [c % (q * q) for c in cts]]
    half = max(limbs.limbs_for(p * p), limbs.limbs_for(q * q))
    for b in key.batches:
        out_t = eng.crt_split_t(rows_of(eng, cts[:b], l2), p, q)
        assert tuple(out_t.shape) == (2, b, half)
        assert out_t[0].is_contiguous() and out_t[1].is_contiguous()
        assert [ints_of(eng, out_t[0]), ints_of(eng, out_t[1])] == [want[0][:b], want[1][:b]], b
    # rows three words wider than N^2, any value of that width
    wide = [rng.getrandbits(32 * (l2 + 3)) for _ in range(5)] + [(1 << (32 * (l2 + 3))) - 1]
    out_t = eng.crt_split_t(rows_of(eng, wide, l2 + 3), p, q)
    assert [ints_of(eng, out_t[0]), ints_of(eng, out_t[1])] == [[c % (p * p) for c in wide], [c % (q * q) for c in wide]]


# ------------------------------------------------------------------ the recombination, on given x rows
def x_for(m_r, r, h_r):
    """An x below r^2 with L_r(x) h_r = m_r modulo r."""
    return 1 + r * (m_r * pow(h_r, -1, r) % r)


@pytest.mark.parametrize("name,swapped", CASES)
def test_recombine_against_the_formulas(eng, keys, name, swapped):
    from protocols.distributed_keygen_amd import limbs
    from protocols.distributed_keygen_amd.private_key import crt_constants

    key = keys[name]
    p, q = key.primes(swapped)
    n = p * q
    h_p, h_q, p_inv = crt_constants(p, q)
    rng = random.Random(8)
    # (m_p, m_q): equal, m_q below m_p mod q, m_p >= q where p > q, the extremes
    pairs = [(0, 0), (5, 5), (min(p, q) - 1, min(p, q) - 1), (p - 1, q - 1), (p - 1, 0), (0, q - 1), (7, 3), (1, 0),
             (p - 1, (p - 1) % q), (max(p - 1, q) % p, 1), (rng.randrange(p), rng.randrange(q))]
    xs = [(x_for(a, p, h_p), x_for(b, q, h_q)) for a, b in pairs]
    xs += [(1, 1), (1 + p * (p - 1), 1), (1, 1 + q * (q - 1)), (1 + p * (p - 1), 1 + q * (q - 1))]
    bad = {3: (2, None), 6: (None, q + 2), 9: (0, 0), 12: (p * p - 1, None), 13: (None, 0), 70: (p, q)}      # row -> replaced halves
    if key.rows == 8:
        xs = [xs[k] for k in (1, 3, 4, 8, 10, 12, 14, 0)]
        bad = {2: (2, None), 5: (None, q + 2), 6: (0, 0)}
    xs = fill(xs, key.rows, lambda: (1 + p * rng.randrange(p), 1 + q * rng.randrange(q)))
    for row, (a, b) in bad.items():
        xs[row] = (xs[row][0] if a is None else a, xs[row][1] if b is None else b)
    want, status = [], []
    for xp, xq in xs:
        st = (0 if xp % p == 1 else 1) | (0 if xq % q == 1 else 2)
        m_p, m_q = (xp - 1) // p * h_p % p, (xq - 1) // q * h_q % q
        want.append(0 if st else m_p + p * ((m_q - m_p) * p_inv % q))
        status.append(st)
    assert {1, 2, 3} <= set(status) and all(0 <= m < n for m in want)
    half = max(limbs.limbs_for(p * p), limbs.limbs_for(q * q))
    xp_t, xq_t = rows_of(eng, [x[0] for x in xs], half), rows_of(eng, [x[1] for x in xs], half)
    for b in key.batches:
        rows_t, status_t = eng.crt_recombine_t(xp_t[:b], xq_t[:b], p, q)
        assert tuple(rows_t.shape) == (b, limbs.limbs_for(n))
        assert ints_of(eng, rows_t) == want[:b] and status_t.cpu().tolist() == status[:b], b
    packed = eng.to_host(eng.crt_recombine_t(xp_t, xq_t, p, q, packed=True))
    assert packed.shape == (key.rows, limbs.limbs_for(n) + 1)
    assert limbs.unpack(packed[:, :-1]) == want and packed[:, -1].tolist() == status


# ------------------------------------------------------------------ end to end
def messages(key, p, q, rng):
    n = key.n
    fixed = [0, 1, n - 1, p, q, p - 1, q - 1, n - p, n - q, n // 2, n // 2 + 1]
    if key.rows == 8:
        fixed = [0, n - 1, p, q - 1, n - p, n - q]
    return fill(fixed, key.rows, lambda: rng.randrange(n))


@pytest.mark.parametrize("name,swapped", CASES)
def test_decrypt_known_plaintexts_every_batch_size(eng, keys, name, swapped):
    from protocols.distributed_keygen_amd import limbs

    key = keys[name]
    p, q = key.primes(swapped)
    rng = random.Random(9)
    msgs = messages(key, p, q, rng)
    cts = key.encrypt_all(msgs)
    invalid = {4: 0, key.rows - 2: 7 * p} if key.rows > 8 else {3: 0, 6: 7 * p}
    status = [0] * key.rows
    for row, c in invalid.items():
        cts[row], msgs[row], status[row] = c, 0, 3 if c == 0 else 1
    msgs[1], cts[1] = 0, key.n2 - 1                                    # N^2 - 1 = -1 decrypts to 0, like c = 1
    l2 = limbs.limbs_for(key.n2)
    cts_t = rows_of(eng, cts, l2)
    for b in key.batches:
        rows_t, status_t = eng.private_decrypt_t(cts_t[:b], p, q)
        assert ints_of(eng, rows_t) == msgs[:b] and status_t.cpu().tolist() == status[:b], b
    # the same rows as one packed tensor, with the modexps one after the other and side by side, fixed window on and off
    ref = eng.to_host(eng.private_decrypt_t(cts_t, p, q, packed=True))
    assert limbs.unpack(ref[:, :-1]) == msgs and ref[:, -1].tolist() == status
    for side in (False, True):
        assert (eng.to_host(eng.private_decrypt_t(cts_t, p, q, packed=True, side_by_side=side)) == ref).all()
    eng.set_fixed_window(True)
    try:
        assert (eng.to_host(eng.private_decrypt_t(cts_t, p, q, packed=True)) == ref).all()
        assert (p, p - 1, True) in eng._n2_plans and (q, q - 1, True) in eng._n2_plans       # the setting reached both plans
    finally:
        eng.set_fixed_window(False)
    # int level
    got, ok = eng.private_decrypt_batch([c + key.n2 for c in cts], p, q)
    assert got == msgs and ok == [not s for s in status]


@pytest.mark.parametrize("name", NAMES)
def test_random_ciphertexts_against_the_lambda_route(eng, keys, name):
    from protocols.distributed_keygen_amd import synthetic

    key = keys[name]
    lam = (key.p - 1) * (key.q - 1)
    shim = synthetic.SharedKey(0, 3, 1, key.n, key.p, key.q, 6, 2, 1)
    cts = synthetic.random_ciphertexts(shim, 1 if key.rows == 8 else 3)
    assert all(math.gcd(c, key.n) == 1 for c in cts)
    want = [(pow(c, lam, key.n2) - 1) // key.n * pow(lam, -1, key.n) % key.n for c in cts]
    assert eng.private_decrypt_batch(cts, key.p, key.q) == (want, [True] * len(cts))
    assert eng.private_decrypt_batch(cts, key.q, key.p) == (want, [True] * len(cts))
    assert eng.private_decrypt_batch([], key.p, key.q) == ([], [])


def test_private_key_object_on_the_engine(eng, keys):
    from protocols.distributed_keygen_amd import PaillierPrivateKey
    from protocols.distributed_keygen_amd.shared_key import PlainCiphertext

    key = keys["k1024"]
    n = key.n
    priv = PaillierPrivateKey(key.p, key.q, engine=eng)
    msgs = [0, 1, n - 1, n // 2 + 1, 123456789]
    cts = key.encrypt_all(msgs)
    assert priv.decrypt_batch(cts) == msgs
    assert priv.decrypt_batch(cts, signed=True) == [0, 1, -1, n // 2 + 1 - n, 123456789]
    assert priv.decrypt_sequence([PlainCiphertext(c, n) for c in cts[:2]]) == msgs[:2]
    with pytest.raises(ValueError, match="valid ciphertext"):
        priv.decrypt_batch(cts + [7 * key.p])
    assert priv.decrypt_batch([cts[2], 3 * key.q, 0], return_ok=True, signed=True) == ([-1, 0, 0], [True, False, False])
    with pytest.raises(ValueError):
        eng.crt_plan(key.p, key.p)
    with pytest.raises(ValueError):
        eng.crt_split_t(eng._empty_rows(3, 2), key.p, key.q)            # rows narrower than N^2


def test_slots_chain_of_the_example_at_key_length_128(eng, keys):
    """slots.encrypt -> homomorphic.matmul -> private decrypt -> slots.decode_t: the rows of the private decryption go into
    the slot codec unchanged (examples/private_key_decrypt.py), and packing.unpack reads them too."""
    from protocols.distributed_keygen_amd import PaillierPrivateKey, limbs, packing
    from protocols.distributed_keygen_amd.randomizer import FastRandomizer, generate_base

    spec = importlib.util.spec_from_file_location("private_key_decrypt_example", ROOT / "examples" / "private_key_decrypt.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    key = keys["k128"]
    priv = PaillierPrivateKey(key.p, key.q, engine=eng)
    rng = np.random.default_rng(4)
    B, I, R = 23, 5, 3
    x = rng.integers(-128, 128, size=(B, I))
    W = rng.integers(-255, 256, size=(R, I))
    bias = rng.integers(-1023, 1024, size=R)
    fr = FastRandomizer(key.n, generate_base(key.n, rng=random.Random(1), engine=eng), engine=eng, device_rng=True)
    scores, b, n_dec = example.private_scores(eng, priv, fr, x, W, bias)
    assert (scores.cpu().numpy() == x @ W.T + bias).all() and n_dec == R * -(-B // packing.slots_per_ciphertext(key.n, b))
    # packing.unpack on the same format: unsigned slots of 16 bits
    k = packing.slots_per_ciphertext(key.n, 16)
    vals = [int(v) for v in rng.integers(0, 1 << 16, size=3 * k)]
    plain = [sum(v << (16 * i) for i, v in enumerate(vals[j : j + k])) for j in range(0, len(vals), k)]
    rows_t, status_t = priv.decrypt_t(rows_of(eng, key.encrypt_all(plain), limbs.limbs_for(key.n2)))
    assert not status_t.any()
    assert packing.unpack(ints_of(eng, rows_t), 16, len(vals), key.n, signed=False) == vals
