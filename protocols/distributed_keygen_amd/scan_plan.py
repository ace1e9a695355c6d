"""Host-side planning of encrypted prefix sums (csrc/mx_scan_n2.hpp).

    out[j] = c_first(j) * ... * c_j   mod N^2        over the SEGMENT that holds j (inclusive, forward)

— the running totals of series of ciphertexts laid one behind the other; ``exclusive`` leaves c_j itself out (the first
output of a segment is 1), ``reverse`` runs every segment from its end.  Reduce-then-scan over levels, on the rows and
the index arrays of the histogram (hist_plan.py), as array operations on whichever device the lengths live on and
never with a Python loop over elements, terms, pieces or segments:

  * every ciphertext is converted into its pair-form row once (``convert``);
  * a segment of ``len`` rows is cut into ``max(1, ceil(len / chunk))`` PIECES of consecutive rows, the last one padded
    with the one row (hist_plan.piece_index; for ``reverse`` the rows of a segment are listed from its end);
  * where every segment is one piece, a level is ONE ``scan`` launch; otherwise the piece totals (``run`` of the
    histogram over the same index array) are scanned EXCLUSIVELY one level up — the same procedure, with the pieces of a
    segment as its rows — and the result is the carry every piece starts from;
  * the last step writes the pair-form products as canonical residues (``store``);
  * STAGES: rows cost ``row_bytes`` per element, so the elements are cut in order into stages under the budget
    (from the end for ``reverse``).  The segment that crosses into the next stage hands its running total on as the
    carry of its first piece there: the pair-form output row of the stage's last element, times that element for an
    exclusive scan (one product).

``cumsum`` runs all of it against a backend — the engine's device tensors (engine._ScanBackend) or the test double's
Python ints (tests/scan_engine.py) — which has the histogram backend's ``row_bytes``, ``chunk``, ``convert``, ``run``,
``join``, ``concat`` and ``ones`` (hist_plan.py) and
  ``scan(rows, n_rows, index, carry, exclusive)``: the row set of `n_rows` prefix products, row i the product stored for
    input row i; ``carry`` is None or (row set, its rows, int32 tensor [pieces] of the row every piece starts from);
  ``store(rows, n_rows)``: the rows of a row set as canonical result rows;
  ``pick(rows, n_rows, row)``: the row set of that one row.
"""

from __future__ import annotations

from typing import Any, Optional, Tuple

from . import hist_plan as hp

TABLE_BUDGET_BYTES = hp.TABLE_BUDGET_BYTES
MAX_CHUNK = hp.MAX_CHUNK


def as_lengths(lengths: Any, count: int, device: Any = None) -> Any:
    """The checked int64 tensor of segment lengths (on `device` if given); None is one series of `count`.  ValueError —
    before any launch — for more than one dimension, a dtype that is not an integer, a negative length, or lengths
    that do not sum to `count`."""
    import numpy as np
    import torch

    if lengths is None:
        lengths = torch.tensor([int(count)], dtype=torch.int64)
    elif not isinstance(lengths, torch.Tensor):
        arr = np.asarray(lengths)
        if arr.dtype == object or (arr.dtype.kind not in "iu" and arr.size):
            raise ValueError(f"lengths must be integers, not {arr.dtype}")
        if arr.ndim != 1:
            raise ValueError(f"lengths must be one-dimensional, not {arr.ndim}-dimensional")
        lengths = torch.from_numpy(np.ascontiguousarray(arr.astype(np.int64)))
    if lengths.dim() != 1:
        raise ValueError(f"lengths must be one-dimensional, not {lengths.dim()}-dimensional")
    if lengths.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"lengths must be an integer tensor, not {lengths.dtype}")
    lengths = lengths.to(torch.int64)
    if lengths.numel() and bool((lengths < 0).any()):
        raise ValueError("a segment length is negative")
    if int(lengths.sum()) != int(count):
        raise ValueError(f"lengths sum to {int(lengths.sum())} for {int(count)} ciphertexts")
    return lengths if device is None else lengths.to(device)


def segment_order(counts: Any, total: int, reverse: bool) -> Any:
    """The rows 0 .. total - 1 (total = sum(counts)) listed segment after segment in scan order: ascending, or every segment from its
    end for `reverse` (the segments themselves stay where they are)."""
    import torch

    pos = torch.arange(total, device=counts.device)
    if not reverse:
        return pos
    first = torch.cumsum(counts, 0) - counts
    seg = torch.repeat_interleave(torch.arange(counts.numel(), device=counts.device), counts)
    return 2 * first[seg] + counts[seg] - 1 - pos


def scan_segments(be: Any, rows: Any, n_rows: int, counts: Any, src: Any, exclusive: bool, chunk: int = 0,
                  carry: Optional[Tuple[Any, int, Any]] = None, level: int = 0) -> Any:
    """The row set of the prefix products of the row set `rows` (`n_rows` rows and the one row): ``counts[s]`` terms
    belong to segment s, ``src`` lists the rows of all terms in scan order, ``carry`` is None or (row set, its rows,
    int32 index per SEGMENT of the row the segment starts from).  `chunk` > 0 overrides the library's chunk (from the
    second level on at least 2: a level has to shrink)."""
    import torch

    n_segments = counts.numel()
    c = int(be.chunk(n_rows, n_segments, int(src.numel()), chunk))
    if level:
        c = max(2, c)
    index, pieces = hp.piece_index(counts, src, c, n_rows)
    n_pieces = index.shape[0]
    if n_pieces != n_segments:                                        # some segment has more than one piece
        totals = be.run(rows, n_rows, index, True)
        order = torch.arange(n_pieces, device=counts.device)
        ups = scan_segments(be, totals, n_pieces, pieces, order, True, chunk, carry, level + 1)
        carry = (ups, n_pieces, order.to(torch.int32))                # piece p starts from the product of the pieces before it
    return be.scan(rows, n_rows, index, carry, exclusive)


def cumsum(be: Any, cts: Any, lengths: Any, exclusive: bool = False, reverse: bool = False, chunk: int = 0,
           table_budget_bytes: int = 0) -> Any:
    """The result rows, one per element, of the segmented prefix products of `cts` (whatever ``be.convert`` takes) by the
    checked `lengths` (as_lengths).  `chunk` and `table_budget_bytes` > 0 override the library's chunk and
    TABLE_BUDGET_BYTES."""
    import torch

    count = int(lengths.sum()) if lengths.numel() else 0
    if count == 0:
        return be.ones(0)
    dev = lengths.device
    budget = max(1, int(table_budget_bytes or TABLE_BUDGET_BYTES))
    per_stage = min(count, max(1, budget // (be.row_bytes + hp.INDEX_BYTES)))
    stages = [(lo, min(count, lo + per_stage)) for lo in range(0, count, per_stage)]
    ends = torch.cumsum(lengths, 0)
    starts = ends - lengths
    results = []
    total = None                                                      # the row set of the running total handed on
    for lo, hi in (reversed(stages) if reverse else stages):
        counts = torch.clamp(torch.clamp(ends, max=hi) - torch.clamp(starts, min=lo), min=0)
        here = counts > 0
        counts = counts[here]
        carry = None
        if total is not None:
            # only the segment that began in the stage before continues: it starts from row 0 of `total`, the others from its one row
            crossing = (ends[here] > hi) if reverse else (starts[here] < lo)
            carry = (total, 1, torch.where(crossing, 0, 1).to(torch.int32))
        rows = be.convert(cts, lo, hi)
        out = scan_segments(be, rows, hi - lo, counts, segment_order(counts, hi - lo, reverse), exclusive, chunk, carry)
        results.append(be.store(out, hi - lo))
        if len(stages) > 1:
            edge = 0 if reverse else hi - lo - 1                      # the stage's last element in scan order
            total = be.pick(out, hi - lo, edge)
            if exclusive:
                both = be.join([total, be.pick(rows, hi - lo, edge)], 1)
                total = be.run(both, 2, torch.tensor([[0, 1]], dtype=torch.int32, device=dev), True)
    return be.concat(results[::-1] if reverse else results)
