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
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

# Weights must satisfy |w| < 2^(bits(N^2) + WEIGHT_MARGIN_BITS) (include/mxpaillier.h: mx_multiexp_nsquare_run).
WEIGHT_MARGIN_BITS = 64
# Workspace of one stage's tables (bytes): larger problems run as several stages.
TABLE_BUDGET_BYTES = 256 << 20

Term = Tuple[int, int]          # (input index, weight)


def weight_bound(n: int) -> int:
    """Smallest |weight| that is refused for the modulus N."""
    return 1 << ((n * n).bit_length() + WEIGHT_MARGIN_BITS)


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
        out = []
        for i, w in items:
            if w == 0:
                continue
            if -bound >= w or w >= bound:
                raise ValueError(f"row {r}: |weight| >= 2^(bits(N^2) + {WEIGHT_MARGIN_BITS})")
            out.append((i, w))
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


def plan_multiexp(rows: List[List[Term]], n_inputs: int, n: int, bias: Optional[Sequence[int]],
                  shape: Callable[[int, int, int, int], Tuple[int, int, int]], table_budget: int = TABLE_BUDGET_BYTES,
                  window: int = 0) -> Plan:
    """The launches of one linear map.  `rows` as normalize_rows returns them; `shape(n_tables, n_rows, terms,
    weight_bits) -> (window, chunk_terms, table_bytes_per_input_per_entry)` is the library's choice
    (mx_multiexp_nsquare_shape); `window` > 0 overrides the window of the first pass."""
    n_out = len(rows)
    if bias is not None and len(bias) != n_out:
        raise ValueError(f"{len(bias)} bias values for {n_out} outputs")
    bias_res = {j: int(b) % n for j, b in enumerate(bias)} if bias is not None else {}
    bias_res = {j: b for j, b in bias_res.items() if b}
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
    # split-K
    p1: List[List[Tuple[Tuple[str, int], int]]] = []
    owner: List[int] = []
    result: List[Tuple[str, int]] = []
    pieces: Dict[int, List[int]] = {}
    for j, terms in enumerate(src_rows):
        if not terms:
            result.append(("one", 0))
            continue
        ks = []
        for lo in range(0, len(terms), chunk):
            ks.append(len(p1))
            p1.append(terms[lo : lo + chunk])
            owner.append(j)
        if len(ks) == 1:
            result.append(("p1", ks[0]))
        else:
            pieces[j] = ks
            result.append(("p2", -1))
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
    if pieces:
        outs = sorted(pieces)
        stage = Stage(sources=[("part", m) for j in outs for m in pieces[j]], window=1)
        local, pos = [], 0
        for j in outs:
            local.append([(pos + t, 1) for t in range(len(pieces[j]))])
            pos += len(pieces[j])
        stage.launches = _bucket_launches(local, list(range(len(outs))))
        stages.append(stage)
        row_of = {j: r for r, j in enumerate(outs)}
        result = [("p2", row_of[j]) if kind == "p2" else (kind, v) for j, (kind, v) in enumerate(result)]
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
    if bias is not None and len(bias) != rows:
        raise ValueError(f"{len(bias)} bias values for {rows} outputs")
    nnz = np.count_nonzero(block, axis=1)
    if int(nnz.min()) * 8 < cols * 7:
        return None
    bias_res = {j: int(b) % n for j, b in enumerate(bias)} if bias is not None else {}
    bias_res = {j: b for j, b in bias_res.items() if b}
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
