"""Host-side planning of encrypted sparse matrix products (csrc/mx_spmm_n2.hpp).

    y_r = (1 + (bias_r mod N) N) * prod_{t in [crow[r], crow[r+1])} x_{col[t]} ^ val[t]   mod N^2

for a PUBLIC sparse matrix in CSR form (``crow[R + 1]``, ``col[nnz]``, signed ``val[nnz]``).  A negative weight uses the
inverse of its input, duplicate (row, column) entries are terms of their own, a stored 0 is no term and an empty row
gives 1 (or its bias factor).

The weights are cut into w-bit digits: with b = bits(max |val|) there are D = ceil(b / w) digit positions, and every
NON-ZERO digit d at position p of a term of row r is a weight-1 term of the SEGMENT r * D + p that names row
``table_row(column or its inverse, d)`` of a table of small powers.  The segment products are then a histogram
(hist_plan.reduce_segments: one stable sort, bincount, cumsum and one scatter into pieces pre-filled with the one
row, levels of ``mx_histogram_nsquare_run`` in pair form), and Horner's rule over the positions of a row — w squarings
and one product per position — gives y_r.  Everything here is array operations on whichever device the index arrays
live on; there is no Python loop over terms, rows, digits or pieces.

  * TABLES: a column that occurs with a positive weight gets the table x^1 .. x^(2^w - 1) of its input; a column that
    occurs with a negative weight gets a second one, of its inverse (one product tree for all of them: a
    non-invertible input under a negative weight is a ValueError, under positive weights it is a legal input).  Table
    t holds the rows t * (2^w - 1) .. (t + 1) * (2^w - 1) - 1 of a histogram row set, digit d at row d - 1;
  * STAGES: a table costs (2^w - 1) rows, so the tables are cut into stages whose rows and index arrays stay under the
    budget; the stage partials of a segment enter one more run of levels like pieces, as hist_plan.histogram does.
    Every input is converted once, whatever the slicing.

``spmm`` runs all of it against a backend: what hist_plan.py asks of one (``row_bytes``, ``chunk``, ``convert``, ``run``,
``join``, ``ones``) and
  ``shape(n_tables, n_rows, nnz, weight_bits, window)``: (window, positions) of mx_spmm_nsquare_shape (``window`` > 0 overrides);
  ``pool(cts, plus, minus)``: the inputs named by the index tensor `plus`, followed by the INVERSES of those named by `minus`;
  ``tables(pool, lo, hi, window)``: the row set of the tables of pool[lo .. hi - 1];
  ``bias(values)``: canonical rows of the bias factors 1 + (b mod N) N;
  ``horner(rows, n_rows, positions, window, bias_rows)``: the result rows from the row set of segment products and the
    converted bias rows (a row set, or None).
The engine's device form is engine._SpmmBackend; tests/spmm_engine.py has one over Python ints.
"""

from __future__ import annotations

from typing import Any, Optional, Sequence, Tuple

from . import hist_plan as hp

TABLE_BUDGET_BYTES = hp.TABLE_BUDGET_BYTES
INDEX_BYTES = hp.INDEX_BYTES
MAX_WINDOW = 8            # what the library takes (include/mxpaillier.h)
MAX_VALUE = (1 << 63) - 1


def _as_vector(x: Any, what: str) -> Any:
    """Nested lists, a numpy array or a torch tensor -> a one-dimensional torch tensor of an integer dtype."""
    import numpy as np
    import torch

    if not isinstance(x, torch.Tensor):
        try:
            arr = np.asarray(x)
        except (ValueError, OverflowError) as exc:
            raise ValueError(f"{what} must be a flat array of integers") from exc
        if arr.dtype == object:
            raise ValueError(f"{what} must be a flat array of integers in [-(2^63 - 1), 2^63 - 1]")
        if arr.dtype.kind not in "iu":
            if arr.size:
                raise ValueError(f"{what} must be an integer array, not {arr.dtype}")
            arr = arr.astype(np.int64)               # (an empty list has no dtype of its own)
        if arr.dtype.kind == "u" and arr.dtype.itemsize > 1:
            if arr.size and int(arr.max()) > MAX_VALUE:
                raise ValueError(f"{what} must lie in [-(2^63 - 1), 2^63 - 1]")
            arr = arr.astype(np.int64)
        x = torch.from_numpy(np.ascontiguousarray(arr))
    if x.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"{what} must be an integer tensor, not {x.dtype}")
    if x.dim() != 1:
        raise ValueError(f"{what} must be one-dimensional, not {x.dim()}-dimensional")
    return x


def as_matrix(matrix: Any, n_inputs: int) -> Tuple[Any, Any, Any]:
    """(crow, col, val) as one-dimensional integer torch tensors from a ``(crow, col, val)`` triple (nested lists, numpy
    arrays or torch tensors) or a two-dimensional torch sparse CSR or COO tensor of an integer dtype with `n_inputs`
    columns (converted by torch's own ``to_sparse_csr``).  ValueError for anything else: shapes and dtypes only, the
    values are check_matrix's."""
    import torch

    if isinstance(matrix, torch.Tensor):
        if matrix.layout not in (torch.sparse_csr, torch.sparse_coo):
            raise ValueError("matrix must be a (crow, col, val) triple or a torch sparse CSR or COO tensor")
        if matrix.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError(f"matrix must be of an integer dtype, not {matrix.dtype}")
        if matrix.dim() != 2:
            raise ValueError(f"matrix must be two-dimensional, not {matrix.dim()}-dimensional")
        if matrix.shape[1] != n_inputs:
            raise ValueError(f"matrix has {matrix.shape[1]} columns for {n_inputs} ciphertexts")
        csr = matrix if matrix.layout == torch.sparse_csr else matrix.to_sparse_csr()
        return csr.crow_indices(), csr.col_indices(), csr.values()
    try:
        crow, col, val = matrix
    except (TypeError, ValueError) as exc:
        raise ValueError("matrix must be a (crow, col, val) triple or a torch sparse CSR or COO tensor") from exc
    crow, col, val = _as_vector(crow, "crow"), _as_vector(col, "col"), _as_vector(val, "val")
    if crow.numel() < 1:
        raise ValueError("crow must hold R + 1 entries")
    if col.numel() != val.numel():
        raise ValueError(f"col has {col.numel()} entries, val has {val.numel()}")
    return crow, col, val


def check_bias(bias: Optional[Sequence[int]], n_rows: int) -> None:
    if bias is not None and len(bias) != n_rows:
        raise ValueError(f"bias has {len(bias)} entries for {n_rows} rows")


def check_matrix(crow: Any, col: Any, val: Any, n_inputs: int) -> None:
    """ValueError — before any launch — for the values of a matrix as_matrix has passed: crow[0] != 0, crow[-1] != nnz,
    a crow that decreases, a column outside [0, n_inputs), a value of -2^63.  A few reductions where the tensors live."""
    import torch

    nnz = col.numel()
    if int(crow[0]) != 0 or int(crow[-1]) != nnz:
        raise ValueError(f"crow must run from 0 to the number of stored values, {nnz}")
    if crow.numel() > 1 and bool((crow[1:] < crow[:-1]).any()):
        raise ValueError("crow must not decrease")
    if nnz and bool(((col < 0) | (col >= int(n_inputs))).any()):
        raise ValueError(f"columns must lie in [0, {int(n_inputs)})")
    if nnz and val.dtype == torch.int64 and bool((val == -MAX_VALUE - 1).any()):
        raise ValueError("values must lie in [-(2^63 - 1), 2^63 - 1]")


def staging(n_tables: int, digit_terms: int, window: int, row_bytes: int, budget: int) -> int:
    """Tables per stage: as many as fit the budget with their (2^w - 1) rows each and one index word per digit term, the
    terms taken as spread evenly over the tables.  At least 1: a budget below one table is exceeded rather than
    refused.  The accounting is nominal (hist_plan.TABLE_BUDGET_BYTES)."""
    per_table = ((1 << window) - 1) * row_bytes + INDEX_BYTES * -(-digit_terms // max(1, n_tables))
    return min(max(1, n_tables), max(1, max(1, int(budget)) // per_table))


def digit_terms(crow: Any, col: Any, val: Any, n_inputs: int, window: int, positions: int) -> Tuple[Any, Any, Any, Any, Any]:
    """(key, table, digit, plus, minus) of every non-zero digit, in term order: the segment r * positions + p, the table
    of the term's column — its number in `plus`, the ascending columns with a positive weight, or len(plus) + its number
    in `minus`, those with a negative one — and the digit itself."""
    import torch

    dev = col.device
    n_rows = crow.numel() - 1
    val = val.to(torch.int64)
    col = col.to(torch.int64)
    mag = val.abs()
    neg = val < 0
    plus_mask = torch.zeros(n_inputs, dtype=torch.bool, device=dev)
    minus_mask = torch.zeros(n_inputs, dtype=torch.bool, device=dev)
    plus_mask[col[val > 0]] = True
    minus_mask[col[neg]] = True
    plus, minus = torch.nonzero(plus_mask).reshape(-1), torch.nonzero(minus_mask).reshape(-1)
    slot_plus = torch.cumsum(plus_mask, 0) - 1
    slot_minus = torch.cumsum(minus_mask, 0) - 1 + plus.numel()
    table = torch.where(neg, slot_minus[col], slot_plus[col])
    row = torch.repeat_interleave(torch.arange(n_rows, device=dev), (crow[1:] - crow[:-1]).to(torch.int64))
    pos = torch.arange(positions, device=dev)
    digit = (mag[:, None] >> (pos * window)[None, :]) & ((1 << window) - 1)
    keep = digit != 0
    key = (row[:, None] * positions + pos[None, :])[keep]
    return key, table[:, None].expand(-1, positions)[keep], digit[keep], plus, minus


def stage_terms(key: Any, src: Any, n_segments: int) -> Tuple[Any, Any]:
    """(counts, src) of one stage for hist_plan.reduce_segments: the terms sorted by segment, in their own order inside
    one (a stable sort)."""
    import torch

    if n_segments < 1 << 31:
        key = key.to(torch.int32)                    # half the bytes of the sort and of its temporaries
    key, order = torch.sort(key, stable=True)
    return torch.bincount(key, minlength=n_segments), src[order]


def spmm(be: Any, cts: Any, n_inputs: int, crow: Any, col: Any, val: Any, bias: Optional[Sequence[int]] = None,
         window: int = 0, chunk: int = 0, table_budget_bytes: int = 0) -> Any:
    """The result rows ``[R]`` of the product of the checked matrix (as_matrix, check_matrix, check_bias) with `cts`
    (whatever ``be.pool`` takes, `n_inputs` of them).  `window`, `chunk` and `table_budget_bytes` > 0 override the
    library's window and chunk and TABLE_BUDGET_BYTES."""
    import torch

    n_rows = crow.numel() - 1
    if n_rows == 0:
        return be.ones(0)
    top = int(val.to(torch.int64).abs().max()) if val.numel() else 0
    bits = top.bit_length()
    if bits == 0:                                    # no term at all: every row is 1, or its bias factor
        return be.ones(n_rows) if bias is None else be.bias(bias)
    nnz = int((val != 0).sum())
    inverted = int(torch.unique(col[val < 0]).numel())
    w, positions = be.shape(n_inputs + inverted, n_rows, nnz, bits, int(window))
    key, table, digit, plus, minus = digit_terms(crow, col, val, n_inputs, w, positions)
    entries = (1 << w) - 1
    n_tables = plus.numel() + minus.numel()
    segs = n_rows * positions
    pool = be.pool(cts, plus, minus)
    t_stage = staging(n_tables, key.numel(), w, be.row_bytes, table_budget_bytes or TABLE_BUDGET_BYTES)
    stages = [(lo, min(n_tables, lo + t_stage)) for lo in range(0, n_tables, t_stage)]
    parts = []
    for lo, hi in stages:
        rows = be.tables(pool, lo, hi, w)
        if len(stages) == 1:
            counts, src = stage_terms(key, table * entries + (digit - 1), segs)
        else:
            mine = (table >= lo) & (table < hi)
            counts, src = stage_terms(key[mine], (table[mine] - lo) * entries + (digit[mine] - 1), segs)
        parts.append(hp.reduce_segments(be, rows, (hi - lo) * entries, counts, src, False, chunk))
    if len(stages) == 1:
        products = parts[0]
    else:
        # the partial of stage t for segment s is row t * segs + s of the joined set: segment s takes one from every stage
        counts = torch.full((segs,), len(stages), dtype=torch.int64, device=col.device)
        src = (torch.arange(segs, device=col.device)[:, None] + torch.arange(len(stages), device=col.device)[None, :] * segs).reshape(-1)
        products = hp.reduce_segments(be, be.join(parts, segs), len(stages) * segs, counts, src, False, chunk)
    bias_rows = None if bias is None else be.convert(be.bias(bias), 0, n_rows)
    return be.horner(products, n_rows, positions, w, bias_rows)
