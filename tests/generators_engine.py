"""Model-backed doubles of the engine's generator calls: "device rows" are tagged Python lists (FakeEngine's _Handle),
the generator's rows come from tools/chacha_model.py (through ``DeviceRng.rows_t``, whose raw call the doubles implement),
shares and sums from tools/generators_model.py, and the refusals are the product's own checks.  Every call is recorded,
so the tests can read the order and the sizes of the draws and whether a party's own rows were taken "from the device".
Everything else is FakeEngine's.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import chacha_model as cm  # noqa: E402
import generators_model as gm  # noqa: E402

from fake_engine import FakeEngine, _Handle  # noqa: E402
from protocols.distributed_keygen_amd import biprime  # noqa: E402


def row_int(words):
    return sum(int(v) << (32 * j) for j, v in enumerate(words))


class DrawEngine(FakeEngine):
    """An engine WITHOUT the generator forms: it only draws rows (numpy) and turns them into ints, so the module-level
    functions of biprime.py run the step through Python.  ``gen_calls`` records ("chacha", call number, count, bits,
    row_words)."""

    def __init__(self) -> None:
        super().__init__()
        self.gen_calls = []

    def chacha20_rows_t(self, key, nonce, counter0, count, bits, row_words=None):
        row_words = -(-bits // 32) if row_words is None else row_words
        call = sum(int(w) << (32 * k) for k, w in enumerate(nonce))
        self.gen_calls.append(("chacha", call, count, bits, row_words))
        return np.array(cm.rows_words(list(key), list(nonce), counter0, count, bits, row_words), dtype="<u4").reshape(count, row_words)

    def _download_ints(self, rows_t):
        return [row_int(r) for r in np.asarray(rows_t).tolist()]


class _RowsHandle(_Handle):
    """generator rows of the double with the one tensor method the product calls on the real rows"""

    def repeat(self, times, _one):
        return _RowsHandle(self[0], list(self[1]) * times)


class GeneratorsEngine(DrawEngine):
    """... and one WITH them: ("shares", groups, group_size), ("sum", parties, groups, group_size), ("own_share_rows_from_device",
    rows) and ("v_from_generator_rows", groups) are recorded next to the draws."""

    def generator_shares_batch(self, mods, group_size, rng, mods_rows=None, keep_rows=False):
        biprime._check_generator_args(mods, group_size)
        if mods_rows is not None:
            assert mods_rows[0] == "mods_rows" and mods_rows[1] == list(mods), "kept moduli rows of other candidates"
        if not mods:
            return ([], None) if keep_rows else []
        bits, words = gm.draw_bits(mods), gm.draw_words(mods)
        draws = self._download_ints(rng.rows_t(self, len(mods) * group_size, bits, words))
        self.gen_calls.append(("shares", len(mods), group_size))
        lists = gm.shares_of_draws(draws, mods, group_size)
        return (lists, _Handle("share_rows", [list(r) for r in lists])) if keep_rows else lists

    def generator_sum_batch(self, shares, mods, group_size, mods_rows=None, keep_rows=False):
        biprime._check_generator_args(mods, group_size)
        if mods_rows is not None:
            assert mods_rows[0] == "mods_rows" and mods_rows[1] == list(mods)
        cols = {}
        for j, col in enumerate(shares):
            if isinstance(col, _Handle):
                assert col[0] == "share_rows"
                self.gen_calls.append(("own_share_rows_from_device", len(col[1])))
                col = col[1]
            cols[j] = col
        self.gen_calls.append(("sum", len(shares), len(mods), group_size))
        lists = gm.generators(cols, mods, group_size)
        return _RowsHandle("generator_rows", lists) if keep_rows else lists

    def _fetched_ints(self, which, rows_t, groups=None):
        assert rows_t[0] == "generator_rows"
        return [list(r) for r in rows_t[1]]

    def biprime_v_batch(self, g_values, exps, mods, keep, mods_rows=None, keep_rows=False, g_rows=None):
        if g_rows is not None:
            handle, group_size = g_rows
            assert handle[0] == "generator_rows" and len(handle[1]) == len(mods) and all(len(r) == group_size for r in handle[1])
            self.gen_calls.append(("v_from_generator_rows", len(mods)))
            g_values = handle[1]
        return super().biprime_v_batch(g_values, exps, mods, keep, mods_rows=mods_rows, keep_rows=keep_rows)


def split_shares(generators, modulus, n_parties, rnd, unreduced_below=None):
    """{party: shares} of one candidate's recorded generators: n_parties additive shares each, the last one chosen so
    that the sum is the generator modulo N.  Generator 0 gets one share equal to N itself; generator 1 an unreduced
    one (a residue plus N, where that stays below `unreduced_below` — the width of a device row — or, with None, a
    negative one and one far wider than N: the int level reduces those on the host)."""
    cols = {j: [] for j in range(1, n_parties + 1)}
    for k, g in enumerate(generators):
        parts = [rnd.randrange(modulus) for _ in range(n_parties - 1)]
        if k == 0 and n_parties > 1:
            parts[0] = modulus
        if k == 1 and n_parties > 1:
            if unreduced_below is None:
                parts[0] = parts[0] - 3 * modulus
                if n_parties > 2:
                    parts[1] = parts[1] + (modulus << 70)
            elif parts[0] + modulus < unreduced_below:
                parts[0] += modulus
        parts.append((g - sum(parts)) % modulus)
        for j, s in enumerate(parts, start=1):
            cols[j].append(s)
    return cols
