"""Host-side planning of encrypted histograms (csrc/mx_hist_n2.hpp).

    H[f][b] = prod_{i : bins[f][i] == b} c_i   mod N^2          (an empty bin gives 1; bins[f][i] == -1 skips sample i)

A call is turned into launches of ``mx_histogram_nsquare_convert`` (every ciphertext into its pair-form row, once) and
``mx_histogram_nsquare_run`` (one group of lanes per PIECE: the product of ``chunk`` rows named by an index array).  This
module builds the index arrays, as array operations on whichever device the bin tensor lives on — so the CPU tests hold
it against plain ``%`` products — and never with a Python loop over samples, terms, bins or pieces:

  * a (feature, bin) pair is a SEGMENT; the terms of a stage are sorted by segment (one stable sort), counted
    (bincount) and placed (cumsum): a segment of ``len`` terms is cut into ``max(1, ceil(len / chunk))`` pieces, and one
    scatter writes every term's row into a ``[pieces][chunk]`` int32 array pre-filled with the index of the one row.
    Ragged bins, empty bins and skipped samples are all in that array; the kernel's trip count is the launch's chunk;
  * LEVELS: while a segment has more than one piece, the pieces of a level are the rows of the next, chunked again
    (the term of piece p is row p: the arrays come from the piece counts alone).  The last level writes canonical
    residues, the others pair-form rows;
  * STAGES: the converted rows cost ``row_bytes`` per sample (576 B at key_length 2048), so the samples are cut into
    stages whose rows and index arrays stay under the budget; the stage partials of a segment enter one more run of
    levels like pieces;
  * SLICES: where the index array of all features alone would not fit beside the rows, the features are cut likewise;
    slices share nothing but the converted rows and their results lie one behind the other.

``histogram`` runs all of it against a backend (the engine's device tensors, or the test double's Python ints):
  ``row_bytes``: bytes of one pair-form row;
  ``chunk(n_rows, n_segments, total_terms, chunk)``: terms per piece (mx_histogram_nsquare_shape; ``chunk`` > 0 overrides);
  ``convert(cts, lo, hi)``: the pair-form rows of samples lo .. hi - 1, followed by the one row;
  ``run(rows, n_rows, index, pair_out)``: per row of the ``[pieces][chunk]`` index tensor the product of the rows it
    names (``n_rows`` names the one row) — in pair form followed by the one row (a row set again), or as canonical
    result rows;
  ``join(row_sets, rows)``: row sets of `rows` rows each laid one behind the other (every set without its one row),
    then the one row;  ``concat(results)``: result rows one behind the other;  ``ones(count)``: `count` result rows of the value 1.
The engine's device form is engine._HistogramBackend; tests/hist_engine.py has one over Python ints.
"""

from __future__ import annotations

from typing import Any, List, Tuple

# Bytes one stage may take for its converted rows and index arrays (the budget of the other planners' tables).  NOMINAL:
# it counts the rows and one int32 per (feature, sample); the padding of the pieces (at most one more word per term and
# segment under the library's chunk, which never exceeds the mean segment), the piece rows of the levels and torch's
# temporaries while the arrays are built (stage_terms, piece_index: a few tens of bytes per term, freed level by level) lie on top.
TABLE_BUDGET_BYTES = 256 << 20
INDEX_BYTES = 4           # one int32 per (feature, sample) of a stage
MAX_CHUNK = 1 << 16       # terms per piece the library takes (include/mxpaillier.h)


def check_bins(bins: Any, n_samples: int, n_bins: int, values: bool = True) -> None:
    """ValueError — before any launch — for bins that are not a two-dimensional integer tensor with `n_samples` columns
    and values in [-1, n_bins), or n_bins < 1.  The values are checked where the tensor lives, with one reduction;
    ``values=False`` leaves that pass to a later call (shape, dtype and n_bins only)."""
    import torch

    if int(n_bins) < 1:
        raise ValueError("n_bins must be at least 1")
    if bins.dim() != 2:
        raise ValueError(f"bins must be two-dimensional [features][samples], not {bins.dim()}-dimensional")
    if bins.shape[1] != n_samples:
        raise ValueError(f"bins has {bins.shape[1]} columns for {n_samples} ciphertexts")
    if bins.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"bins must be an integer tensor, not {bins.dtype}")
    if values and bins.numel() and bool(((bins < -1) | (bins >= int(n_bins))).any()):
        raise ValueError(f"bin values must lie in [-1, {int(n_bins)})")


def as_bins(bins: Any, n_samples: int, device: Any = None) -> Any:
    """Nested lists, a numpy array or a torch tensor -> a torch tensor (on `device` if given); no feature at all is
    ``[0][n_samples]``.  ValueError for ragged rows or values that are not integers."""
    import numpy as np
    import torch

    if not isinstance(bins, torch.Tensor):
        try:
            arr = np.asarray(bins)
        except ValueError as exc:                    # ragged rows
            raise ValueError("bins must be a rectangular [features][samples] array") from exc
        if arr.dtype == object:
            raise ValueError("bins must be a rectangular [features][samples] array of integers")
        if arr.dtype.kind not in "iu":
            if arr.size:
                raise ValueError(f"bins must be an integer array, not {arr.dtype}")
            arr = arr.astype(np.int64)               # (an empty list has no dtype of its own)
        if arr.ndim == 1 and arr.shape[0] == 0:
            arr = arr.reshape(0, n_samples)
        if arr.dtype.kind == "u" and arr.dtype.itemsize > 1:
            arr = arr.astype(np.int64)
        bins = torch.from_numpy(np.ascontiguousarray(arr))
    return bins if device is None else bins.to(device)


def staging(n_samples: int, n_features: int, row_bytes: int, budget: int) -> Tuple[int, int]:
    """(samples per stage, features per slice).  The rows get at least half of the budget; the features are sliced only
    where the index array of all of them does not fit the other half; then a stage takes as many samples as fit with
    the slice's index array beside their rows.  Both are at least 1: a budget below one row and one index word is
    exceeded rather than refused.  The accounting is nominal (TABLE_BUDGET_BYTES)."""
    budget = max(1, int(budget))
    s_half = min(max(1, n_samples), max(1, (budget // 2) // row_bytes))
    f_slice = min(max(1, n_features), max(1, (budget // 2) // (INDEX_BYTES * s_half)))
    s_stage = min(max(1, n_samples), max(1, budget // (row_bytes + INDEX_BYTES * f_slice)))
    return s_stage, f_slice


def piece_index(counts: Any, src: Any, chunk: int, one: int) -> Tuple[Any, Any]:
    """(index, pieces): the ``[sum(pieces)][chunk]`` int32 array of one level and the pieces of every segment.
    ``counts[s]`` terms belong to segment s; ``src`` lists the rows of all terms, segment after segment.  Segment s
    gets ``max(1, ceil(counts[s] / chunk))`` consecutive pieces, its terms fill them in order, and what is left of its
    last piece — the whole piece of an empty segment — names the row `one`."""
    import torch

    pieces = torch.clamp((counts + (chunk - 1)) // chunk, min=1)
    ends = torch.cumsum(pieces, 0)
    total = int(ends[-1]) if ends.numel() else 0
    index = torch.full((total, chunk), int(one), dtype=torch.int32, device=counts.device)
    if src.numel():
        first_term = torch.cumsum(counts, 0) - counts                     # of every segment
        seg = torch.repeat_interleave(torch.arange(counts.numel(), device=counts.device), counts)
        slot = (ends - pieces)[seg] * chunk + (torch.arange(src.numel(), device=counts.device) - first_term[seg])
        index.view(-1)[slot] = src.to(torch.int32)
    return index, pieces


def reduce_segments(be: Any, rows: Any, n_rows: int, counts: Any, src: Any, final: bool, chunk: int = 0) -> Any:
    """One product per segment from the row set `rows` (`n_rows` rows and the one row): levels of piece_index / be.run
    until every segment has one piece.  `final`: canonical result rows; otherwise a row set of one row per segment.
    `chunk` > 0 overrides the library's chunk (from the second level on at least 2: a level has to shrink)."""
    import torch

    n_segments = counts.numel()
    level = 0
    while True:
        total = int(src.numel())
        c = int(be.chunk(n_rows, n_segments, total, chunk))
        if level:
            c = max(2, c)
        index, pieces = piece_index(counts, src, c, n_rows)
        last = index.shape[0] == n_segments
        out = be.run(rows, n_rows, index, not (last and final))
        if last:
            return out
        rows, n_rows = out, index.shape[0]
        counts, src = pieces, torch.arange(n_rows, device=counts.device)
        level += 1


def stage_terms(bins: Any, n_bins: int) -> Tuple[Any, Any]:
    """(counts, src) of one stage and slice: ``bins`` is its ``[features][samples]`` block; segment f * n_bins + b
    holds the samples with bins[f] == b in ascending order (a stable sort), -1 entries hold none."""
    import torch

    feats, samples = bins.shape
    # int32 keys and sample numbers wherever they fit: half the bytes of the sort and of its temporaries
    kt = torch.int32 if feats * n_bins < 1 << 31 else torch.int64
    key = bins.to(kt) + torch.arange(feats, device=bins.device, dtype=kt)[:, None] * n_bins
    keep = (bins >= 0).reshape(-1)
    key = key.reshape(-1)[keep]
    src = torch.arange(samples, device=bins.device, dtype=torch.int32).repeat(feats)[keep]
    key, order = torch.sort(key, stable=True)
    return torch.bincount(key, minlength=feats * n_bins), src[order]


def histogram(be: Any, cts: Any, bins: Any, n_bins: int, chunk: int = 0, table_budget_bytes: int = 0) -> Any:
    """The result rows ``[F * n_bins]`` (row f * n_bins + b) of the histogram of `cts` (whatever ``be.convert`` takes,
    ``bins.shape[1]`` samples) by the checked bin tensor `bins` (check_bins).  `chunk` and `table_budget_bytes` > 0
    override the library's chunk and TABLE_BUDGET_BYTES."""
    import torch

    feats, samples = bins.shape
    n_bins = int(n_bins)
    if feats == 0:
        return be.ones(0)
    if samples == 0:
        return be.ones(feats * n_bins)
    s_stage, f_slice = staging(samples, feats, be.row_bytes, table_budget_bytes or TABLE_BUDGET_BYTES)
    slices = [(lo, min(feats, lo + f_slice)) for lo in range(0, feats, f_slice)]
    stages = [(lo, min(samples, lo + s_stage)) for lo in range(0, samples, s_stage)]
    partials: List[List[Any]] = [[] for _ in slices]
    for lo, hi in stages:
        rows = be.convert(cts, lo, hi)
        for k, (f0, f1) in enumerate(slices):
            counts, src = stage_terms(bins[f0:f1, lo:hi], n_bins)
            partials[k].append(reduce_segments(be, rows, hi - lo, counts, src, len(stages) == 1, chunk))
    if len(stages) == 1:
        return be.concat([p[0] for p in partials])
    results = []
    for (f0, f1), parts in zip(slices, partials):
        segs = (f1 - f0) * n_bins
        # the partial of stage t for segment s is row t * segs + s of the joined set: segment s takes one from every stage
        counts = torch.full((segs,), len(stages), dtype=torch.int64, device=bins.device)
        src = (torch.arange(segs, device=bins.device)[:, None] + torch.arange(len(stages), device=bins.device)[None, :] * segs).reshape(-1)
        results.append(reduce_segments(be, be.join(parts, segs), len(stages) * segs, counts, src, True, chunk))
    return be.concat(results)
