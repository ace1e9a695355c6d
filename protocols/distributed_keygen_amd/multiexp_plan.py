"""Host-side planning of the multi-exponentiation modulo N^2 (csrc/mx_multiexp_n2.hpp).

    y_j = (1 + (b_j mod N) N) * prod_i c_i^(W_ji)   mod N^2

A call is turned into launches of ``mx_multiexp_nsquare_run``, which takes non-negative weights and one padded
``[rows][terms]`` block per launch.  This module decides, in plain Python (no GPU, so the CPU tests hold it against
``pow``):

  * sign splitting: an input used with a negative weight gets a table of its own, built from its inverse (computed once
    on the device); the term then carries ``|w|``;
  * the bias as one more weight-1 input ``1 + (b mod N) N``;
  * split-K: rows with more terms than the library's chunk are cut into pieces that run on groups of their own, and a
    second pass multiplies the partial products with weight-1 terms (one window of one bit: no squarings);
  * bucketing: rows are launched in buckets of similar length (powers of two), so that one long row does not pad every
    other row to its length;
  * stages: consecutive pass-1 rows are cut into stages whose tables fit the workspace budget;
  * dense rows of int64 weights (plan_dense) are planned as array operations on the [rows][inputs] block instead of
    term by term.

``execute`` runs a plan against a backend (the engine's device tensors, or the test double's Python ints).

``plan_matmul`` / ``execute_matmul`` (at the end) are the batched form, csrc/mx_matmul_n2.hpp: one public W applied to a
batch of ciphertext vectors, planned once per call whatever the batch.

The rules that the three planners (plan_multiexp, plan_matmul, conv_plan.plan_conv) follow alike have one home each, here:
``check_weights`` and ``bias_residues`` (the refusals and the bias), ``sign_split`` (which users get an inverted table),
``split_k`` / ``combine_launches`` (the pieces of a long row and the pass that multiplies them) and ``TwoPassPlan`` (the
fields of a plan of shared weight rows, and where in its launches every result lies).
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

# Weights must satisfy |w| < 2^(bits(N^2) + WEIGHT_MARGIN_BITS) (include/mxpaillier.h: mx_multiexp_nsquare_run).
WEIGHT_MARGIN_BITS = 64
# Workspace of one stage's tables (bytes): larger problems run as several stages.
TABLE_BUDGET_BYTES = 256 << 20

Term = Tuple[int, int]          # (input index, weight)


def weight_bound(n: int) -> int:
    """Smallest |weight| that is refused for the modulus N."""
    return 1 << ((n * n).bit_length() + WEIGHT_MARGIN_BITS)


def check_weights(ws: Sequence[int], bound: int, what: str, k: int) -> None:
    """ValueError if a weight of row / kernel `k` is not inside (-bound, bound)."""
    if ws and (min(ws) <= -bound or max(ws) >= bound):
        raise ValueError(f"{what} {k}: |weight| >= 2^(bits(N^2) + {WEIGHT_MARGIN_BITS})")


def bias_residues(bias: Optional[Sequence[int]], count: int, n: int, what: str) -> Dict[int, int]:
    """output -> b mod N for the non-zero residues of a bias of `count` values (None: no bias).  ValueError for another
    length."""
    if bias is None:
        return {}
    if len(bias) != count:
        raise ValueError(f"{len(bias)} bias values for {count} {what}")
    residues = ((j, int(b) % n) for j, b in enumerate(bias))
    return {j: b for j, b in residues if b}


def sign_split(pos: Set[int], neg: Set[int]) -> Tuple[List[int], List[int], Dict[int, int]]:
    """(plain, inverted, slot) for the users (columns, channels) met with a positive and with a negative weight: the
    plain tables come first, then the inverted ones, each ascending; ``slot[i]`` is the table of user i as it is and
    ``slot[~i]`` that of its inverse."""
    plain, inverted = sorted(pos), sorted(neg)
    slot = {i: c for c, i in enumerate(plain)}
    slot.update({~i: len(plain) + c for c, i in enumerate(inverted)})
    return plain, inverted, slot


def normalize_rows(weights: Sequence[Any], n_inputs: int, n: int) -> List[List[Term]]:
    """Rows of a linear map -> lists of (input, weight) with the zero weights dropped.  A row is a dense sequence of
    ``n_inputs`` weights or a sparse mapping ``{input: weight}``.  Raises ValueError for a bad index, a row of the wrong
    length or a weight out of bounds — before anything is launched."""
    bound = weight_bound(n)
    rows: List[List[Term]] = []
    for r, row in enumerate(weights):
        if isinstance(row, dict):
            items = sorted((int(i), int(w)) for i, w in row.items())
            for i, _ in items:
                if not 0 <= i < n_inputs:
                    raise ValueError(f"row {r}: input index {i} out of range [0, {n_inputs})")
        else:
            vals = list(row)
            if len(vals) != n_inputs:
                raise ValueError(f"row {r} has {len(vals)} weights for {n_inputs} inputs")
            items = [(i, int(w)) for i, w in enumerate(vals)]
        out = [(i, w) for i, w in items if w]
        check_weights([w for _, w in out], bound, "row", r)
        rows.append(out)
    return rows


@dataclass
class Launch:
    """One mx_multiexp_nsquare_run: rows of a bucket, padded to `terms`."""
    rows: List[int]              # pass-level row ids, in launch order
    index: np.ndarray            # [len(rows), terms] int32, table row of every term
    weights: np.ndarray          # [len(rows), terms, wwords] uint32
    weight_bits: int


@dataclass
class Stage:
    """One table set (its sources, in table order) and the launches that read it."""
    sources: List[Tuple[str, int]]        # ("x", input) | ("inv", input) | ("bias", output) | ("part", pass-1 row)
    window: int
    launches: List[Launch] = field(default_factory=list)


@dataclass
class Plan:
    n_outputs: int
    stages: List[Stage]                   # pass 1 (one or more stages), then pass 2 (at most one stage)
    pass1_rows: int
    combine_from: int                     # index of the first pass-2 stage (== len(stages) if none)
    result: List[Tuple[str, int]]         # per output: ("one", 0) | ("p1", pass-1 row) | ("p2", pass-2 row)
    inverted: List[int]                   # inputs whose inverse is needed
    bias: Dict[int, int]                  # output -> b mod N (non-zero)


def _pack_weights(ws: List[List[int]], terms: int) -> Tuple[np.ndarray, int]:
    bits = max((w.bit_length() for row in ws for w in row), default=0)
    wwords = max(1, (bits + 31) // 32)
    rows = len(ws)
    if bits <= 64:
        flat = np.zeros((rows, terms), dtype=np.uint64)
        for r, row in enumerate(ws):
            flat[r, : len(row)] = row
        arr = flat.view(np.uint32).reshape(rows, terms, 2)[:, :, :wwords]
        return np.ascontiguousarray(arr), bits
    arr = np.zeros((rows, terms, wwords), dtype=np.uint32)
    for r, row in enumerate(ws):
        for t, w in enumerate(row):
            arr[r, t] = np.frombuffer(w.to_bytes(4 * wwords, "little"), dtype="<u4")
    return arr, bits


def _bucket_launches(rows: List[List[Term]], ids: List[int]) -> List[Launch]:
    """Launches of buckets of rows with lengths in (2^(k-1), 2^k]; rows keep their order inside a bucket."""
    buckets: Dict[int, List[int]] = {}
    for k, row in enumerate(rows):
        buckets.setdefault(max(0, (len(row) - 1).bit_length()), []).append(k)
    out = []
    for _, members in sorted(buckets.items()):
        terms = max(len(rows[k]) for k in members)
        index = np.zeros((len(members), terms), dtype=np.int32)
        ws = []
        for r, k in enumerate(members):
            index[r, : len(rows[k])] = [t for t, _ in rows[k]]
            ws.append([w for _, w in rows[k]])
        weights, bits = _pack_weights(ws, terms)
        out.append(Launch([ids[k] for k in members], index, weights, bits))
    return out


def split_k(term_rows: List[List[Any]], chunk: int) -> Tuple[List[List[Any]], List[Tuple[str, int]], List[List[int]]]:
    """(pass-1 rows, result, split): a row of more than `chunk` terms is cut into pieces, which are pass-1 rows of their
    own; ``result`` says per row where its value is — ("one", 0) for a row of no terms, ("p1", pass-1 row), or
    ("p2", r) for the r-th split row, whose pieces are the pass-1 rows ``split[r]``."""
    p1: List[List[Any]] = []
    result: List[Tuple[str, int]] = []
    split: List[List[int]] = []
    for terms in term_rows:
        if not terms:
            result.append(("one", 0))
            continue
        ks = []
        for lo in range(0, len(terms), chunk):
            ks.append(len(p1))
            p1.append(terms[lo : lo + chunk])
        if len(ks) == 1:
            result.append(("p1", ks[0]))
        else:
            result.append(("p2", len(split)))
            split.append(ks)
    return p1, result, split


def combine_launches(split: List[List[int]]) -> List[Launch]:
    """The second pass over ``part_rows = [k for ks in split for k in ks]`` as its tables: pass-2 row r multiplies the
    pieces of split row r with weight 1 (run with window 1: no squarings)."""
    local, at = [], 0
    for ks in split:
        local.append([(at + t, 1) for t in range(len(ks))])
        at += len(ks)
    return _bucket_launches(local, list(range(len(split))))


def plan_multiexp(rows: List[List[Term]], n_inputs: int, n: int, bias: Optional[Sequence[int]],
                  shape: Callable[[int, int, int, int], Tuple[int, int, int]], table_budget: int = TABLE_BUDGET_BYTES,
                  window: int = 0) -> Plan:
    """The launches of one linear map.  `rows` as normalize_rows returns them; `shape(n_tables, n_rows, terms,
    weight_bits) -> (window, chunk_terms, table_bytes_per_input_per_entry)` is the library's choice
    (mx_multiexp_nsquare_shape); `window` > 0 overrides the window of the first pass."""
    n_out = len(rows)
    bias_res = bias_residues(bias, n_out, n, "outputs")
    inverted = sorted({i for row in rows for i, w in row if w < 0})
    # pass-1 terms over SOURCES (global source keys; tables are numbered per stage below)
    src_rows: List[List[Tuple[Tuple[str, int], int]]] = []
    for j, row in enumerate(rows):
        terms = [(("x", i) if w > 0 else ("inv", i), abs(w)) for i, w in row]
        if j in bias_res:
            terms.append((("bias", j), 1))
        src_rows.append(terms)
    max_terms = max((len(r) for r in src_rows), default=0)
    max_bits = max((w.bit_length() for r in src_rows for _, w in r), default=0)
    n_sources = len({s for r in src_rows for s, _ in r})
    win, chunk, entry_bytes = shape(n_sources, n_out, max_terms, max_bits)
    if window:
        win = window
    chunk = max(1, chunk)
    p1, result, split = split_k(src_rows, chunk)
    # stages: consecutive pass-1 rows whose distinct sources fit the budget
    per_source = entry_bytes << win
    max_sources = max(1, table_budget // max(1, per_source))
    stages: List[Stage] = []
    k = 0
    while k < len(p1):
        seen: Dict[Tuple[str, int], int] = {}
        members: List[int] = []
        while k < len(p1):
            new = {s for s, _ in p1[k] if s not in seen}
            if members and len(seen) + len(new) > max_sources:
                break
            for s, _ in p1[k]:
                if s not in seen:
                    seen[s] = len(seen)
            members.append(k)
            k += 1
        stage = Stage(sources=list(seen), window=win)
        local = [[(seen[s], w) for s, w in p1[m]] for m in members]
        stage.launches = _bucket_launches(local, members)
        stages.append(stage)
    combine_from = len(stages)
    if split:
        stages.append(Stage(sources=[("part", m) for ks in split for m in ks], window=1, launches=combine_launches(split)))
    return Plan(n_out, stages, len(p1), combine_from, result, inverted, bias_res)


def _dense_block(weights: Sequence[Any], n_inputs: int) -> Optional[np.ndarray]:
    """The rows as one int64 block [rows, n_inputs] when they are all dense sequences of that length and every weight
    fits int64 above -2^63 (so that |w| fits too); None otherwise (the general path then checks and plans them)."""
    if not len(weights) or n_inputs == 0 or isinstance(weights[0], dict):
        return None
    if isinstance(weights, np.ndarray):
        if weights.ndim != 2 or weights.shape[1] != n_inputs or weights.dtype.kind not in "iu":
            return None
        block = weights
    else:
        if any(isinstance(r, dict) or len(r) != n_inputs for r in weights):
            return None
        try:
            block = np.array(weights, dtype=np.int64)
        except (OverflowError, TypeError, ValueError):
            return None
    if block.dtype != np.int64:
        if block.dtype.kind == "u" and block.size and int(block.max()) >= 1 << 63:
            return None
        block = block.astype(np.int64)
    if block.size and int(block.min()) == -(1 << 63):
        return None
    return block


def plan_dense(block: np.ndarray, n: int, bias: Optional[Sequence[int]],
               shape: Callable[[int, int, int, int], Tuple[int, int, int]], table_budget: int = TABLE_BUDGET_BYTES,
               window: int = 0) -> Optional[Plan]:
    """plan_multiexp for a dense int64 block, as array operations: every row lists the columns in the same order (a
    zero weight stays as a weight-0 term, a negative one reads the column's inverted table), plus one bias term; split-K
    cuts every row into the same pieces (the last one padded with weight-0 terms).  Only where that is what
    plan_multiexp would launch anyway up to a few padding terms: at least 7/8 of every row non-zero, tables within the
    budget.  None otherwise."""
    rows, cols = block.shape
    nnz = np.count_nonzero(block, axis=1)
    if int(nnz.min()) * 8 < cols * 7:
        return None                                               # (plan_multiexp then refuses a bias of the wrong length)
    bias_res = bias_residues(bias, rows, n, "outputs")
    pos_cols = np.flatnonzero((block > 0).any(axis=0))
    neg_cols = np.flatnonzero((block < 0).any(axis=0))
    bias_rows = sorted(bias_res)
    n_sources = len(pos_cols) + len(neg_cols) + len(bias_rows)
    terms = cols + (1 if bias_rows else 0)
    mag = np.abs(block).astype(np.uint64)
    bits = int(mag.max()).bit_length() if mag.size else 0
    win, chunk, entry_bytes = shape(n_sources, rows, terms, max(bits, 1 if bias_rows else 0))
    if window:
        win = window
    if n_sources * (entry_bytes << win) > table_budget:
        return None
    x_of = np.zeros(cols, dtype=np.int64)
    x_of[pos_cols] = np.arange(len(pos_cols))
    inv_of = np.zeros(cols, dtype=np.int64)
    inv_of[neg_cols] = len(pos_cols) + np.arange(len(neg_cols))
    index = np.where(block < 0, inv_of[None, :], x_of[None, :]).astype(np.int32)
    if bias_rows:
        bcol = np.zeros((rows, 1), dtype=np.int32)
        bw = np.zeros((rows, 1), dtype=np.uint64)
        first = len(pos_cols) + len(neg_cols)
        for k, j in enumerate(bias_rows):
            bcol[j, 0] = first + k
            bw[j, 0] = 1
        index = np.concatenate([index, bcol], axis=1)
        mag = np.concatenate([mag, bw], axis=1)
        bits = max(bits, 1)
    chunk = max(1, min(int(chunk), terms))
    pieces = -(-terms // chunk)
    if pieces * chunk != terms:                                   # pad the last piece with weight-0 terms
        pad = pieces * chunk - terms
        index = np.concatenate([index, np.zeros((rows, pad), dtype=np.int32)], axis=1)
        mag = np.concatenate([mag, np.zeros((rows, pad), dtype=np.uint64)], axis=1)
    wwords = max(1, (bits + 31) // 32)
    # pass-1 row r * pieces + p: piece p of output r
    weights = np.ascontiguousarray(mag.view(np.uint32).reshape(rows * pieces, chunk, 2)[:, :, :wwords])
    index = np.ascontiguousarray(index.reshape(rows * pieces, chunk))
    sources = [("x", int(c)) for c in pos_cols] + [("inv", int(c)) for c in neg_cols] + [("bias", j) for j in bias_rows]
    stages = [Stage(sources=sources, window=win, launches=[Launch(list(range(rows * pieces)), index, weights, bits)])]
    if pieces == 1:
        return Plan(rows, stages, rows, 1, [("p1", j) for j in range(rows)], [int(c) for c in neg_cols], bias_res)
    comb = Stage(sources=[("part", m) for m in range(rows * pieces)], window=1)
    comb.launches = [Launch(list(range(rows)), np.arange(rows * pieces, dtype=np.int32).reshape(rows, pieces),
                            np.ones((rows, pieces, 1), dtype=np.uint32), 1)]
    stages.append(comb)
    return Plan(rows, stages, rows * pieces, 1, [("p2", j) for j in range(rows)], [int(c) for c in neg_cols], bias_res)


def plan_call(weights: Sequence[Any], n_inputs: int, n: int, bias: Optional[Sequence[int]],
              shape: Callable[[int, int, int, int], Tuple[int, int, int]], table_budget: int = TABLE_BUDGET_BYTES,
              window: int = 0) -> Plan:
    """The plan of one call: plan_dense where it applies (dense rows of int64 weights), else normalize_rows +
    plan_multiexp.  Raises ValueError, before anything is launched, where either does."""
    block = _dense_block(weights, n_inputs)
    if block is not None:
        plan = plan_dense(block, n, bias, shape, table_budget, window)
        if plan is not None:
            return plan
    rows = normalize_rows(weights, n_inputs, n)
    return plan_multiexp(rows, n_inputs, n, bias, shape, table_budget, window)


def execute(plan: Plan, be: Any, inputs: Any) -> Any:
    """Runs `plan` on backend `be` over the reduced input rows `inputs`.  The backend provides
      ``take(rows, positions)``, ``invert(rows)`` (ValueError if some row is not invertible), ``bias_rows(residues)``;
      ``gather(inputs, inverted, bias, parts)``: the table inputs of a stage, parts = [("x" | "inv" | "bias", k)];
      ``run(table_rows or None, n_tables, launch, window)``: the rows of one launch (None: the stage's tables are built);
      ``rows_of([(out, r)])`` and ``assemble([(out, r) or None])``: rows picked out of launch results (None = one).
    The engine's device form is engine._MultiexpBackend; tests/test_homomorphic_host.py has one over Python ints."""
    inv_pos = {i: k for k, i in enumerate(plan.inverted)}
    inv_rows = be.invert(be.take(inputs, plan.inverted)) if plan.inverted else None
    bias_keys = sorted(plan.bias)
    bias_pos = {j: k for k, j in enumerate(bias_keys)}
    bias_rows = be.bias_rows([plan.bias[j] for j in bias_keys]) if bias_keys else None
    p1_out: List[Any] = [None] * plan.pass1_rows
    p2_out: List[Any] = []

    def run_stage(stage: Stage, table_rows: Any, sink: Callable[[int, Any, int], None]) -> None:
        first = True
        for launch in stage.launches:
            out = be.run(table_rows if first else None, len(stage.sources), launch, stage.window)
            first = False
            for r, rid in enumerate(launch.rows):
                sink(rid, out, r)

    for stage in plan.stages[: plan.combine_from]:
        parts = []
        for kind, v in stage.sources:
            if kind == "x":
                parts.append(("x", v))
            elif kind == "inv":
                parts.append(("inv", inv_pos[v]))
            else:
                parts.append(("bias", bias_pos[v]))
        table_rows = be.gather(inputs, inv_rows, bias_rows, parts)

        def sink1(rid, out, r):
            p1_out[rid] = (out, r)
        run_stage(stage, table_rows, sink1)
    if plan.combine_from < len(plan.stages):
        stage = plan.stages[plan.combine_from]
        table_rows = be.rows_of([p1_out[m] for _, m in stage.sources])
        p2_out = [None] * len(set(r for l in stage.launches for r in l.rows))

        def sink2(rid, out, r):
            p2_out[rid] = (out, r)
        run_stage(stage, table_rows, sink2)
    picks = []
    for kind, v in plan.result:
        picks.append(None if kind == "one" else (p1_out[v] if kind == "p1" else p2_out[v]))
    return be.assemble(picks)


# ---- encrypted matrix products over a batch of ciphertext vectors (csrc/mx_matmul_n2.hpp) ----------
#
#     Y[b][j] = (1 + (bias_j mod N) N) * prod_i X[b][i]^(W[j][i])   mod N^2
#
# The weight rows are shared by every sample, so everything below is planned ONCE per call, whatever the batch:
#
#   * W is normalised once (dense int64 rows as array operations on the block, anything else through normalize_rows);
#   * sign split BY COLUMN: a column used with a negative weight anywhere gets a second table column, built from the
#     inverses of that column's samples (one product tree per call over every inverted column of every sample);
#   * the bias is one SHARED table per row with a non-zero bias: index -1 - k in the launch arrays, stored once per tile
#     behind the per-sample tables (the kernel reads it without the sample's offset);
#   * tiles of `tile_batch` samples under the table budget, the last one ragged;
#   * split-K (split_k): pieces of a row's term list are extra weight rows, and the second pass (combine_launches) is
#     itself a shared-weight product (weights 1, window 1) whose table columns are the split rows' pieces of every sample;
#   * buckets of weight rows of similar length, as _bucket_launches makes them.
#
# The launch arrays have one leading entry per weight row (times pieces) and are reused by every tile.  conv_plan.py
# plans its kernels the same way; what the two plans share is TwoPassPlan.

@dataclass
class TwoPassPlan:
    """The launches of shared weight rows (the rows of a matrix, the kernels of a convolution), as split_k and
    combine_launches make them."""
    bias: Dict[int, int]                  # row -> b mod N (non-zero); shared table k belongs to sorted(bias)[k]
    window: int
    chunk: int
    launches: List[Launch]                # pass 1: Launch.rows are pass-1 rows; index < 0: shared table -1 - index
    pass1_rows: int
    part_rows: List[int]                  # pass-1 rows that are pieces of split rows = the table columns of pass 2
    combine: List[Launch]                 # pass 2 (empty if no row was split): Launch.rows are pass-2 rows
    result: List[Tuple[str, int]]         # per weight row: ("one", 0) | ("p1", pass-1 row) | ("p2", pass-2 row)

    def picks(self) -> Tuple[List[Tuple[int, int, int]], List[Optional[Tuple[int, int, int]]]]:
        """(part_picks, picks): where the tables of pass 2 and the results lie, as (pass, launch of that pass, row of
        the launch); None is a result that is one."""
        where = {("p1", rid): (1, k, r) for k, launch in enumerate(self.launches) for r, rid in enumerate(launch.rows)}
        where.update({("p2", rid): (2, k, r) for k, launch in enumerate(self.combine) for r, rid in enumerate(launch.rows)})
        return [where["p1", m] for m in self.part_rows], [None if kind == "one" else where[kind, v] for kind, v in self.result]


@dataclass
class MatmulPlan(TwoPassPlan):
    """Launch.index >= 0 in pass 1: a table column (x_cols, then inverted)."""
    n_rows: int
    n_inputs: int
    x_cols: List[int]                     # input columns with a table of their own (a positive weight somewhere), ascending
    inverted: List[int]                   # input columns whose inverses get a table column (a negative weight somewhere)
    tile_batch: int

    @property
    def n_cols(self) -> int:
        return len(self.x_cols) + len(self.inverted)


def _matmul_rows(weights: Sequence[Any], n_inputs: int, n: int) -> List[Tuple[List[int], List[int]]]:
    """Per weight row (columns, signed weights) with the zero weights dropped, columns ascending: the dense int64 block
    by array operations, anything else (sparse, mixed, weights beyond int64) through normalize_rows.  ValueError as
    normalize_rows raises it."""
    block = _dense_block(weights, n_inputs)
    if block is not None:                          # (an int64 weight is always within the bound)
        out = []
        for row in block:
            nz = np.flatnonzero(row)
            out.append((nz.tolist(), row[nz].tolist()))
        return out
    return [([i for i, _ in row], [w for _, w in row]) for row in normalize_rows(weights, n_inputs, n)]


def plan_matmul(weights: Sequence[Any], n_inputs: int, n: int, bias: Optional[Sequence[int]], batch: int,
                shape: Callable[[int, int, int, int, int, int, int], Tuple[int, int, int]],
                table_budget: int = TABLE_BUDGET_BYTES, window: int = 0) -> MatmulPlan:
    """The launches of one batched matrix product.  `weights`: one row per output, a dense sequence of `n_inputs` signed
    ints or a sparse ``{column: weight}`` (they may be mixed).  ``shape(n_cols, n_rows, terms, weight_bits, batch,
    table_budget, window) -> (window, tile_batch, chunk_terms)`` is the library's choice (mx_matmul_nsquare_shape).
    Raises ValueError — before anything is launched — for a row of the wrong length, a bad column, a weight out of
    bounds or a bias of the wrong length."""
    weights = weights if isinstance(weights, np.ndarray) else list(weights)
    n_rows = len(weights)
    bias_res = bias_residues(bias, n_rows, n, "outputs")
    rows = _matmul_rows(weights, n_inputs, n)
    shared_of = {j: k for k, j in enumerate(sorted(bias_res))}
    pos, neg = set(), set()
    for cols, ws in rows:
        for i, w in zip(cols, ws):
            (pos if w > 0 else neg).add(i)
    x_cols, inverted, slot = sign_split(pos, neg)
    term_rows: List[List[Term]] = []
    for j, (cols, ws) in enumerate(rows):
        terms = [(slot[i], w) if w > 0 else (slot[~i], -w) for i, w in zip(cols, ws)]
        if j in shared_of:
            terms.append((-1 - shared_of[j], 1))
        term_rows.append(terms)
    max_terms = max((len(r) for r in term_rows), default=0)
    max_bits = max((w.bit_length() for r in term_rows for _, w in r), default=0)
    win, tile, chunk = shape(len(x_cols) + len(inverted), n_rows, max_terms, max_bits, int(batch), int(table_budget), int(window))
    tile, chunk = max(1, int(tile)), max(1, int(chunk))
    p1, result, split = split_k(term_rows, chunk)
    return MatmulPlan(bias=bias_res, window=int(win), chunk=chunk, launches=_bucket_launches(p1, list(range(len(p1)))),
                      pass1_rows=len(p1), part_rows=[k for ks in split for k in ks], combine=combine_launches(split),
                      result=result, n_rows=n_rows, n_inputs=n_inputs, x_cols=x_cols, inverted=inverted, tile_batch=tile)


def execute_matmul(plan: MatmulPlan, be: Any, inputs: Any, batch: int) -> Any:
    """Runs `plan` on backend `be` over the sample-major input rows `inputs` (row b * n_inputs + i) and returns the
    sample-major result rows (row b * n_rows + j).  A "column block" is a set of rows [column][sample], column-major.
    The backend provides
      ``columns(inputs, n_inputs, batch, cols)``: the column block of the listed input columns over all samples;
      ``invert(block)``: its element-wise inverse (ValueError if some row is not invertible);
      ``tile(block, batch, lo, hi)``: the block restricted to samples lo .. hi - 1;
      ``bias_rows(residues)``: the rows 1 + b N;  ``concat(parts)``: row sets one behind the other;
      ``run_matmul(table_rows or None, n_cols, n_shared, tile, launch, window)``: the sample-major results
        [tile][len(launch.rows)] of one launch (None: the tables of the previous launch are still in place);
      ``select(outs, picks, tile, column_major)``: from the results of several launches, for every sample the entries
        picks = [(launch, row) or None (= one)] — sample-major [tile][len(picks)], or as a column block.
    The engine's device form is engine._MatmulBackend; tests/test_matmul_host.py has one over Python ints."""
    if batch == 0:
        return be.concat([])
    n_cols, shared = plan.n_cols, sorted(plan.bias)
    x_block = be.columns(inputs, plan.n_inputs, batch, plan.x_cols) if plan.x_cols else None
    inv_block = be.invert(be.columns(inputs, plan.n_inputs, batch, plan.inverted)) if plan.inverted else None
    bias_rows = be.bias_rows([plan.bias[j] for j in shared]) if shared else None
    # `select` takes the results of both passes as one list, pass 1 first
    part_picks, picks = ([pk and (pk[1] + (len(plan.launches) if pk[0] == 2 else 0), pk[2]) for pk in pks] for pks in plan.picks())
    results = []
    for lo in range(0, batch, plan.tile_batch):
        hi = min(batch, lo + plan.tile_batch)
        t = hi - lo
        outs = []
        if plan.launches:
            parts = [be.tile(blk, batch, lo, hi) for blk in (x_block, inv_block) if blk is not None]
            if bias_rows is not None:
                parts.append(bias_rows)
            tables = be.concat(parts)
            for launch in plan.launches:
                outs.append(be.run_matmul(tables, n_cols, len(shared), t, launch, plan.window))
                tables = None
        if plan.combine:
            tables = be.select(outs, part_picks, t, True)
            for launch in plan.combine:
                outs.append(be.run_matmul(tables, len(part_picks), 0, t, launch, 1))
                tables = None
        results.append(be.select(outs, picks, t, False))
    return be.concat(results)
