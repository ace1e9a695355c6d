"""Keys, parameters and draws the range-proof tests share (test_range_proof_host.py, test_gpu_range_proofs.py): the
golden safe-prime keys as N, another of them or the 128-bit parameters of golden/range_params.json as the auxiliary
modulus, and the model (tools/range_model.py) as the oracle.  The statement needs l + 258 <= bits(N) - 1, so the
smallest golden key that can carry a proof at all is the 1024-bit one; the 128-bit key is the one every entry point
must refuse."""

from __future__ import annotations

import json
import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "tools"))
sys.path.insert(0, str(HERE))

import range_model as rm  # noqa: E402

from protocols.distributed_keygen_amd import range_proof  # noqa: E402

KEYS = json.loads((HERE / "golden" / "threshold_keys.json").read_text())["keys"]
PARAMS128 = json.loads((HERE / "golden" / "range_params.json").read_text())
KEY = bytes(range(32))
LABEL = b"sender 7 / session 2026-10-20"


def primes(key_length):
    return tuple(int(KEYS[str(key_length)][k], 16) for k in "pq")


def modulus(key_length):
    p, q = primes(key_length)
    return p * q


def secrets128():
    return tuple(int(PARAMS128[k], 16) for k in ("p", "q", "lambda", "tau"))


def parameters(aux_bits, seed=11):
    """(RangeParameters, (lambda, ph, qh), the model's Parameters) over the golden primes of `aux_bits` bits."""
    if aux_bits == 128:
        ph, qh, lam, tau = secrets128()
    else:
        ph, qh = primes(aux_bits)
        rnd = random.Random(seed)
        lam = rnd.randrange(((ph - 1) // 2) * ((qh - 1) // 2))
        tau = rnd.randrange(2, ph * qh)
    params, secret = range_proof.RangeParameters.from_primes(ph, qh, lam, tau)
    return params, secret, rm.make_parameters(ph, qh, lam, tau)


def statements(n, bits, count, seed=5):
    """(messages, randomness, ciphertexts): 0, 2^bits - 1, 1, then random messages below 2^bits."""
    rnd = random.Random(seed)
    msgs = ([0, (1 << bits) - 1, 1] + [rnd.randrange(1 << bits) for _ in range(max(0, count - 3))])[:count]
    rands = [rnd.randrange(1, n) for _ in msgs]
    return msgs, rands, [rm.encrypt(n, m, r) for m, r in zip(msgs, rands)]


def model_proofs(n, mpar, bits, label, msgs, rands, call):
    """The model's proofs for the draws of DeviceRng(KEY, first_call=call), as six columns."""
    draws = rm.device_draws(KEY, call, len(msgs), n, mpar, bits)
    rows = [rm.prove(n, mpar, bits, label, m, r, *(d[k] for d in draws)) for k, (m, r) in enumerate(zip(msgs, rands))]
    return tuple([row[j] for row in rows] for j in range(6))


# ---- the cases of Engine.multiexp_mod_t (test_gpu_range_proofs.py runs them; test_range_proof_host.py checks that every
# instance mx_multiexp_instances reports is among them) ----------------------------------------------------------------------
def _odd(bits, seed, top_ones=0):
    rnd = random.Random(seed)
    m = rnd.getrandbits(bits) | (1 << (bits - 1)) | 1
    if top_ones:
        m |= ((1 << top_ones) - 1) << (bits - top_ones)
    return m


# (name, modulus, row counts, terms, window, weight_bits, shared bases).  Groups of K lanes: 64 / K rows fill a wavefront, so
# the row counts are 1, 7, 64 / K - 1, 64 / K, 64 / K + 1 and 65 where the modulus is small enough for Python pow to follow.
MULTIEXP_CASES = [
    ("64 bits", _odd(64, 1), (1, 7, 63, 64, 65), 2, 4, 31, False),
    ("64 bits, long weights", _odd(64, 2), (7,), 3, 5, 64 + 385, True),
    ("30 bits: one over a limb", _odd(30, 3), (7,), 1, 5, 33, False),
    ("65 bits: one over two words", _odd(65, 4), (7,), 2, 8, 33, True),
    ("128 bits", _odd(128, 5), (65,), 3, 1, 128, False),
    ("128 bits, one-bit weights", _odd(128, 6), (7,), 2, 8, 1, False),
    ("258 bits: one over a lane", _odd(258, 7), (1, 31, 32, 33, 65), 2, 5, 258 + 385, False),
    ("1015 bits, top limb all ones", _odd(1015, 8, top_ones=29), (7,), 2, 4, 128, False),
    ("1024 bits", modulus(1024), (7, 15, 16, 17), 2, 4, 128, False),
    ("1024 bits, shared, long weights", modulus(1024), (7,), 2, 5, 1024 + 385, True),
    ("2048 bits", modulus(2048), (7, 8, 9), 2, 5, 2048 + 385, True),
    ("2048 bits, per-row", modulus(2048), (9,), 3, 4, 33, False),
    ("4096 bits", _odd(4096, 9), (3, 4, 5, 9), 1, 4, 128, False),
    ("4096 bits, long weights", _odd(4096, 10), (5,), 1, 5, 4096 + 385, True),
    ("8192 bits", _odd(8192, 11), (1, 2, 3), 2, 4, 33, False),
    ("16384 bits", _odd(16384, 12), (1, 2), 1, 1, 31, False),
]


def multiexp_case(name):
    """(modulus, inputs, index rows, weight rows, terms, window, weight_bits, row counts) of a case: bases 0, 1 and M - 1
    and the weights 0 (on the base 0: 0^0), 1, all ones and top bit only in the first rows; two rows index the same
    inputs."""
    _, mod, counts, terms, window, wbits, shared = next(c for c in MULTIEXP_CASES if c[0] == name)
    rnd = random.Random(name)
    rows = max(counts)
    n_inputs = max(3, terms) if shared else rows * terms
    inputs = [rnd.randrange(mod) for _ in range(n_inputs)]
    for k, v in enumerate((0, 1, mod - 1)[:n_inputs]):
        inputs[k] = v
    index = [[(j if shared else r * terms + j) for j in range(terms)] for r in range(rows)]
    for k in range(terms, n_inputs if shared else 0):
        index[-1 - (k - terms)][0] = k                  # (fewer terms than special bases: the last rows read the others)
    if shared and rows > 1:
        index[1] = list(index[0])
    elif rows > 1 and (rows - 1) * terms >= 3:
        index[-1] = list(index[0])                      # (the LAST row: the first rows read the special bases 0, 1, M - 1)
    weights = [[rnd.getrandbits(wbits) for _ in range(terms)] for _ in range(rows)]
    flat = [(r, j) for r in range(rows) for j in range(terms)]
    for (r, j), w in zip(flat, (0, 1, (1 << wbits) - 1, 1 << (wbits - 1))):
        weights[r][j] = w
    return mod, inputs, index, weights, terms, window, wbits, counts
