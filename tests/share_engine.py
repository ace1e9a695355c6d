"""A model-backed double of the engine's candidate and sharing calls: "device rows" are numpy uint32 arrays, the
generator's rows come from tools/chacha_model.py (through ``DeviceRng.rows_t``, whose raw call the double implements),
candidates and shares from tools/share_model.py, and the refusals are the product's own checks (shamir.check_*).  Every
call is recorded, so the tests can read the order and the sizes of the draws.  Everything else is FakeEngine's.  Lives in
tests/ only; the product never imports it."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import chacha_model as cm  # noqa: E402
import share_model as sm  # noqa: E402

from fake_engine import FakeEngine  # noqa: E402
from protocols.distributed_keygen_amd import shamir  # noqa: E402


def rows_of(values, words):
    return np.array([sm.int_row(v, words) for v in values], dtype="<u4").reshape(len(values), words)


def ints_of(rows):
    return [sm.row_int(r) for r in np.asarray(rows).reshape(-1, np.asarray(rows).shape[-1]).tolist()]


class ShareEngine(FakeEngine):
    """``share_calls`` records ("chacha", call number, count, bits, row_words), ("candidates", count, prime_length,
    first_party, row_words) and ("share", has secrets, degree, points, batch) in the order they were made."""

    def __init__(self) -> None:
        super().__init__()
        self.share_calls = []

    def chacha20_rows_t(self, key, nonce, counter0, count, bits, row_words=None):
        row_words = -(-bits // 32) if row_words is None else row_words
        call = sum(int(w) << (32 * k) for k, w in enumerate(nonce))
        self.share_calls.append(("chacha", call, count, bits, row_words))
        return np.array(cm.rows_words(list(key), list(nonce), counter0, count, bits, row_words), dtype="<u4").reshape(count, row_words)

    def prime_candidates_t(self, count, prime_length, first_party, rng=None, random_t=None, row_words=None):
        in_words, row_words = shamir.check_candidate_args(count, prime_length, row_words)
        if (rng is None) == (random_t is None):
            raise ValueError("exactly one of rng and random_t expected")
        if random_t is not None and tuple(random_t.shape) != (count, in_words):
            raise ValueError("random_t of another shape")
        if random_t is None:
            random_t = rng.rows_t(self, count, prime_length - 3)
        self.share_calls.append(("candidates", count, prime_length, bool(first_party), row_words))
        return rows_of(sm.candidates(random_t.tolist(), prime_length, first_party), row_words)

    def shamir_share_t(self, secrets_t, prime, degree, points, batch=None, rng=None, draws_t=None, out_t=None):
        points = shamir.check_share_args(prime, degree, points)
        limbs = -(-prime.bit_length() // 32)
        if secrets_t is not None:
            batch = secrets_t.shape[0]
        elif batch is None:
            raise ValueError("a sharing of zero needs batch=")
        bits, cw = sm.coefficient_bits(prime), sm.coefficient_words(prime)
        if (rng is None) == (draws_t is None):
            raise ValueError("exactly one of rng and draws_t expected")
        if draws_t is not None and tuple(draws_t.shape) != (degree, batch, cw):
            raise ValueError("draws_t of another shape")
        if draws_t is None:
            draws_t = rng.rows_t(self, degree * batch, bits, cw).reshape(degree, batch, cw)
        self.share_calls.append(("share", secrets_t is not None, degree, tuple(points), batch))
        draws = [ints_of(draws_t[k]) for k in range(degree)]
        secrets = ints_of(secrets_t) if secrets_t is not None else None
        out = sm.shamir_share(secrets, draws, prime, points)
        return np.stack([rows_of(col, limbs) for col in out]) if batch else np.zeros((len(points), 0, limbs), dtype="<u4")

    def _download_ints(self, rows_t):
        return ints_of(rows_t)
