"""A Python-int double of what spmm_plan.py drives: the histogram double of tests/hist_engine.py with the table, pool,
bias and Horner steps of the sparse matrix product over Python ints, and an engine with the two calls of the real one.
Every launch is recorded.  The window is the library's own (mx_spmm_nsquare_shape needs no GPU).  Lives in tests/ only;
the product never imports it."""

from __future__ import annotations

import ctypes

from hist_engine import HistBackend, default_chunk
from protocols.distributed_keygen_amd import spmm_plan as sp
from protocols.distributed_keygen_amd.engine import _check_modulus


def library_shape(bits, n_tables, n_rows, nnz, weight_bits, window=0):
    """(status, window, positions) of mx_spmm_nsquare_shape for a modulus of `bits` bits."""
    from protocols.distributed_keygen_amd import _lib

    k, l, w, d = (ctypes.c_int() for _ in range(4))
    rc = _lib.lib().mx_spmm_nsquare_shape(bits, n_tables, n_rows, nnz, weight_bits, 0, window, k, l, w, d, ctypes.c_int64())
    return rc, w.value, d.value


class SpmmBackend(HistBackend):
    def __init__(self, n, row_bytes=72, chunk_fn=default_chunk):
        super().__init__(n, row_bytes, chunk_fn)
        self.n = n
        self.shapes = []            # (n_tables, n_rows, nnz, weight_bits, window asked for) -> what the library said
        self.pools = []             # (plus, minus) column lists
        self.table_calls = []       # (lo, hi, window)
        self.horners = []           # (n_rows, positions, window, with bias)

    def shape(self, n_tables, n_rows, nnz, weight_bits, window):
        rc, w, d = library_shape(self.n.bit_length(), n_tables, n_rows, nnz, weight_bits, window)
        assert rc == 0
        self.shapes.append(((n_tables, n_rows, nnz, weight_bits, window), (w, d)))
        return w, d

    def pool(self, cts, plus, minus):
        plus, minus = plus.tolist(), minus.tolist()
        self.pools.append((plus, minus))
        return [cts[i] % self.n2 for i in plus] + [pow(cts[i], -1, self.n2) for i in minus]      # ValueError without an inverse

    def tables(self, pool, lo, hi, window):
        self.table_calls.append((lo, hi, window))
        return [pow(x, d, self.n2) for x in pool[lo:hi] for d in range(1, 1 << window)] + [1]

    def bias(self, values):
        return [(1 + (int(b) % self.n) * self.n) % self.n2 for b in values]

    def horner(self, rows, n_rows, positions, window, bias_rows):
        assert len(rows) == n_rows * positions + 1 and rows[-1] == 1
        assert bias_rows is None or len(bias_rows) == n_rows + 1
        self.horners.append((n_rows, positions, window, bias_rows is not None))
        out = []
        for r in range(n_rows):
            acc = rows[r * positions + positions - 1]
            for p in range(positions - 2, -1, -1):
                for _ in range(window):
                    acc = acc * acc % self.n2
                acc = acc * rows[r * positions + p] % self.n2
            if bias_rows is not None:
                acc = acc * bias_rows[r] % self.n2
            out.append(acc)
        return out


class SpmmEngine:
    """ciphertext_spmm_batch / spmm_nsquare_t of the engine over SpmmBackend (cts: ints)."""

    def __init__(self, **backend):
        self.backend_args = backend
        self.calls = []             # (cts, fixed_base)
        self.backend = None

    def spmm_nsquare_t(self, cts, crow, col, val, n, bias=None, window=0, chunk=0, table_budget_bytes=0):
        _check_modulus(n)                                   # the engine's own refusals
        if not 0 <= window <= sp.MAX_WINDOW:
            raise ValueError("window")
        crow_t, col_t, val_t = sp.as_matrix((crow, col, val), len(cts))
        sp.check_bias(bias, crow_t.numel() - 1)
        sp.check_matrix(crow_t, col_t, val_t, len(cts))
        self.backend = SpmmBackend(n, **self.backend_args)
        return sp.spmm(self.backend, list(cts), len(cts), crow_t, col_t, val_t, bias, window, chunk, table_budget_bytes)

    def ciphertext_spmm_batch(self, cts, crow, col, val, n, bias=None, fixed_base=None, **overrides):
        out = self.spmm_nsquare_t(cts, crow, col, val, n, bias, **overrides)
        self.calls.append((list(cts), fixed_base))          # (a refused call is not recorded)
        return out
