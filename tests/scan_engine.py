"""A Python-int double of what scan_plan.py drives: the histogram double's backend (rows are lists of Python ints, a row
set is the rows followed by the value 1, products by plain ``%``) with the scan, store and pick of the real one, and an
engine with the two cumsum calls.  Every launch is recorded, so the tests can count conversions, levels, stages and
stores.  Lives in tests/ only; the product never imports it."""

from __future__ import annotations

from hist_engine import HistBackend

from protocols.distributed_keygen_amd import scan_plan as sp
from protocols.distributed_keygen_amd.engine import _check_modulus


class ScanBackend(HistBackend):
    def __init__(self, n, **kw):
        super().__init__(n, **kw)
        self.inputs = None          # the list the engine was called with: conversions of anything else are not inputs
        self.input_converts = []    # (lo, hi) of the conversions of the inputs
        self.scans = []             # (n_rows, pieces, chunk, with carry, exclusive, rows stored in order)
        self.stores = []            # n_rows
        self.picks = 0

    def convert(self, cts, lo, hi):
        if cts is self.inputs:
            self.input_converts.append((lo, hi))
        return super().convert(cts, lo, hi)

    def scan(self, rows, n_rows, index, carry, exclusive):
        assert len(rows) == n_rows + 1 and rows[n_rows] == 1
        assert str(index.dtype) == "torch.int32" and index.dim() == 2 and index.shape[0] >= 1 and index.shape[1] >= 1
        idx = index.tolist()
        assert all(0 <= i <= n_rows for row in idx for i in row)
        starts = [1] * len(idx)
        if carry is not None:
            carry_rows, n_carry, carry_index = carry
            assert len(carry_rows) == n_carry + 1 and carry_rows[n_carry] == 1
            assert str(carry_index.dtype) == "torch.int32" and tuple(carry_index.shape) == (len(idx),)
            picks = carry_index.tolist()
            assert all(0 <= i <= n_carry for i in picks)
            starts = [carry_rows[i] for i in picks]
        out = [None] * n_rows + [1]
        stored = []
        for row, acc in zip(idx, starts):
            for i in row:
                if i == n_rows:
                    continue                         # padding: multiplies by one, stores nothing
                if not exclusive:
                    acc = acc * rows[i] % self.n2
                assert out[i] is None, "an output row is stored twice"
                out[i] = acc
                stored.append(i)
                if exclusive:
                    acc = acc * rows[i] % self.n2
        self.scans.append((n_rows, len(idx), len(idx[0]), carry is not None, bool(exclusive), stored))
        return out

    def store(self, rows, n_rows):
        assert len(rows) == n_rows + 1 and all(v is not None for v in rows)
        self.stores.append(n_rows)
        return list(rows[:n_rows])

    def pick(self, rows, n_rows, row):
        assert 0 <= row < n_rows and rows[row] is not None
        self.picks += 1
        return [rows[row], 1]


class ScanEngine:
    """ciphertext_cumsum_batch / cumsum_nsquare_t of the engine over ScanBackend (cts: ints)."""

    def __init__(self, **backend):
        self.backend_args = backend
        self.calls = []             # (cts, lengths, exclusive, reverse, fixed_base)
        self.backend = None

    def cumsum_nsquare_t(self, cts, lengths, n, exclusive=False, reverse=False, chunk=0, table_budget_bytes=0):
        _check_modulus(n)                                   # the engine's own refusal
        if not 0 <= chunk <= sp.MAX_CHUNK:
            raise ValueError("chunk")
        lengths_t = sp.as_lengths(lengths, len(cts))
        self.backend = ScanBackend(n, **self.backend_args)
        self.backend.inputs = list(cts)
        return sp.cumsum(self.backend, self.backend.inputs, lengths_t, exclusive, reverse, chunk, table_budget_bytes)

    def ciphertext_cumsum_batch(self, cts, lengths, n, exclusive=False, reverse=False, fixed_base=None, chunk=0, table_budget_bytes=0):
        out = self.cumsum_nsquare_t(cts, lengths, n, exclusive, reverse, chunk, table_budget_bytes)
        self.calls.append((list(cts), lengths, exclusive, reverse, fixed_base))      # (a refused call is not recorded)
        return out
