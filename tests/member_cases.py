"""Keys, value lists, statements and directed challenge rows the membership-proof tests share
(test_membership_host.py, test_gpu_membership.py): the golden safe-prime keys as N and the model
(tools/member_model.py) as the oracle."""

from __future__ import annotations

import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "tools"))
sys.path.insert(0, str(HERE))

import member_model as mm  # noqa: E402
from range_cases import KEY, modulus  # noqa: E402,F401

from protocols.distributed_keygen_amd import slots  # noqa: E402

LABEL = b"voter 7 / ballot 2026-10-21"
M128 = (1 << 128) - 1


def value_sets(n):
    return {"bit": [0, 1], "signed": [0, 1, n - 1], "one_hot": slots.one_hot_values(n, 16, 5), "k16": list(range(3, 19))}


def statements(n, values, count, seed=5):
    """(real slots, messages, randomness, ciphertexts): slot r mod k, so every slot is the real one somewhere when
    count >= k."""
    rnd = random.Random(seed)
    index = [r % len(values) for r in range(count)]
    msgs = [values[i] for i in index]
    rands = [rnd.randrange(1, n) for _ in msgs]
    return index, msgs, rands, [mm.encrypt(n, m, r) for m, r in zip(msgs, rands)]


def model_proofs(n, values, label, index, rands, call):
    """The model's proofs for the draws of DeviceRng(KEY, first_call=call): (a, e, z), a list of k ints per row each."""
    zt, et = mm.device_draws(KEY, call, len(index), n, len(values))
    rows = [mm.prove(n, values, label, i, r, zt[row], et[row]) for row, (i, r) in enumerate(zip(index, rands))]
    return tuple([list(row[j]) for row in rows] for j in range(3))


def equations_hold(n, values, label, c, proof):
    """The verifier's equations written out once more, independently of the model's verify."""
    a, es, zs = proof
    e = mm.challenge(mm.context(n, values, label), c, a, mm.limbs_for(n * n))
    us = [c * pow(1 + n, -s, n * n) % (n * n) for s in values]
    return sum(es) % (1 << 128) == e and all(pow(z, n, n * n) == aj * pow(u, ej, n * n) % (n * n) for z, aj, u, ej in zip(zs, a, us, es))


def directed_challenges(k):
    """(e, sims, index) rows that drive the carries and borrows of csrc/mx_member.hpp through all four words, with the
    real slot first and last: all-ones sims (the sum wraps through every word), e = 0 (the borrow runs through every
    word), e = 2^128 - 1, a carry out of each word in turn, and sims whose sum is exactly 2^128."""
    rows = []
    for index in (0, k - 1):
        rows += [(0, [M128] * k, index), (M128, [M128] * k, index), (0, [0] * (k - 1) + [1], index), (0, [1] + [0] * (k - 1), index),
                 (M128, [0] * k, index), (0, [0] * k, index), (1, [1 << 127] * k, index)]
        for word in range(4):
            top = (1 << (32 * (word + 1))) - 1
            rows.append((top, [top] + [1] * (k - 1), index))              # a carry out of word `word`
            rows.append((0, [1 << (32 * word)] * k, index))               # a borrow from word `word` up
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def random_challenges(k, count, seed):
    rnd = random.Random(seed)
    sims = [[rnd.getrandbits(128) for _ in range(k)] for _ in range(count)]
    return [rnd.getrandbits(128) for _ in range(count)], sims, [rnd.randrange(k) for _ in range(count)]
