"""A Python-int double of what hist_plan.py drives: a backend whose "rows" are lists of Python ints (a row set is the
rows followed by the value 1), products by plain ``%``, and an engine with the two histogram calls of the real one.
Every launch is recorded, so the tests can count pieces, levels, stages and padding.  Lives in tests/ only; the product
never imports it."""

from __future__ import annotations

from protocols.distributed_keygen_amd import hist_plan as hp
from protocols.distributed_keygen_amd.engine import _check_modulus


def default_chunk(n_rows, n_segments, total_terms):
    """A stand-in for the library's choice, small enough that tiny cases take several levels."""
    return 4


class HistBackend:
    def __init__(self, n, row_bytes=72, chunk_fn=default_chunk):
        self.n2 = n * n
        self.row_bytes = row_bytes
        self.chunk_fn = chunk_fn
        self.converts = []          # (lo, hi)
        self.runs = []              # (n_rows, pieces, chunk, pair_out, terms that are not the one row)

    def chunk(self, n_rows, n_segments, total_terms, chunk):
        return chunk if chunk > 0 else self.chunk_fn(n_rows, n_segments, total_terms)

    def convert(self, cts, lo, hi):
        self.converts.append((lo, hi))
        return [c % self.n2 for c in cts[lo:hi]] + [1]

    def run(self, rows, n_rows, index, pair_out):
        assert len(rows) == n_rows + 1 and rows[n_rows] == 1
        assert str(index.dtype) == "torch.int32" and index.dim() == 2 and index.shape[0] >= 1 and index.shape[1] >= 1
        idx = index.tolist()
        assert all(0 <= i <= n_rows for row in idx for i in row)
        self.runs.append((n_rows, len(idx), len(idx[0]), bool(pair_out), sum(i != n_rows for row in idx for i in row)))
        out = []
        for row in idx:
            acc = 1
            for i in row:
                acc = acc * rows[i] % self.n2
            out.append(acc)
        return out + [1] if pair_out else out

    def join(self, row_sets, rows):
        assert all(len(s) == rows + 1 for s in row_sets)
        return [v for s in row_sets for v in s[:rows]] + [1]

    def concat(self, results):
        return [v for r in results for v in r]

    def ones(self, count):
        return [1] * count


class HistEngine:
    """ciphertext_histogram_batch / histogram_nsquare_t of the engine over HistBackend (cts: ints)."""

    def __init__(self, **backend):
        self.backend_args = backend
        self.calls = []             # (cts, fixed_base)
        self.backend = None

    def histogram_nsquare_t(self, cts, bins, n_bins, n, chunk=0, table_budget_bytes=0):
        _check_modulus(n)                                   # the engine's own refusal
        bins_t = hp.as_bins(bins, len(cts))
        hp.check_bins(bins_t, len(cts), n_bins)
        self.backend = HistBackend(n, **self.backend_args)
        return hp.histogram(self.backend, list(cts), bins_t, n_bins, chunk, table_budget_bytes)

    def ciphertext_histogram_batch(self, cts, bins, n_bins, n, fixed_base=None, chunk=0, table_budget_bytes=0):
        flat = self.histogram_nsquare_t(cts, bins, n_bins, n, chunk, table_budget_bytes)
        self.calls.append((list(cts), fixed_base))          # (a refused call is not recorded)
        feats = len(flat) // n_bins
        return [flat[f * n_bins : (f + 1) * n_bins] for f in range(feats)]
