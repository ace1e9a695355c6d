"""Host-side planning of encrypted convolutions modulo N^2 (csrc/mx_matmul_n2.hpp).

    Y[b][o][y][x] = (1 + (bias_o mod N) N) * prod_(c,i,j) X[b][c][y sh - ph + i dh][x sw - pw + j dw] ^ w[o][c][i][j]   mod N^2

— cross-correlation, the convention of ``torch.nn.functional.conv2d``; a tap outside the grid contributes 1.  The kernels
are weight rows shared by every output position, as the rows of ``multiexp_plan.plan_matmul`` are shared by every sample,
and the same pieces are reused here (the refusals, bias_residues, sign_split, split_k and combine_launches, whose second
pass runs on mx_matmul_nsquare_run, and the plan's two-pass fields, TwoPassPlan).  What
differs is the table set: the tables are the PIXELS of the padded grids, one each however many windows cover it, and a
term names the table of its tap at output position 0; the kernel adds the position's origin.  Everything is planned once
per call, whatever B and H' W':

  * the kernel is normalised once and its zero taps are dropped;
  * sign split BY CHANNEL: a channel that meets a negative tap anywhere gets a second grid, of inverses (one product
    tree per call over the real pixels of those channels);
  * padded pixels are rows of the value 1 in the padded grids — the weight rows are shared by all positions, so a border
    position cannot drop its outside taps; it multiplies by a table of ones instead;
  * the bias is one SHARED table per kernel with a non-zero bias, index -1 - k;
  * tables of a tile, in table order: [image][input row][grid][column], then the shared ones.  With the input row outside
    the grid index, ``index`` does not depend on how many rows a tile holds, and the origins of a ragged last tile are a
    prefix of the full tile's: both arrays are made once;
  * tiles under the table budget: several whole images where they fit, else bands of output rows of one image with the
    input rows they need (the halo rows are tabled again by the next band).

``execute_conv`` runs a plan against a backend (the engine's device tensors, or the test double's Python ints).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np

from .multiexp_plan import (TABLE_BUDGET_BYTES, Term, TwoPassPlan, _bucket_launches, bias_residues, check_weights, combine_launches,
                            sign_split, split_k, weight_bound)


def _pair(v: Any, name: str, least: int) -> Tuple[int, int]:
    """An int or a pair of ints, each >= least."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{name} must be an int or a pair of ints")
        a, b = int(v[0]), int(v[1])
    else:
        a = b = int(v)
    if a < least or b < least:
        raise ValueError(f"{name} must be >= {least}")
    return a, b


def output_hw(h: int, w: int, kh: int, kw: int, stride: Any = 1, padding: Any = 0, dilation: Any = 1) -> Tuple[int, int]:
    """(H', W') = ((H + 2 ph - dh (kh - 1) - 1) // sh + 1, likewise for W); 0 where the kernel does not fit."""
    sh, sw = _pair(stride, "stride", 1)
    ph, pw = _pair(padding, "padding", 0)
    dh, dw = _pair(dilation, "dilation", 1)
    oh = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    ow = (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    return max(0, oh), max(0, ow)


def kernel_array(weights: Any) -> np.ndarray:
    """The public kernel as an object array [O][C][kh][kw] of Python ints.  ValueError for another rank or a ragged
    nesting.  A kernel of no channels ([O][0]) is taken as 1 x 1; no kernels at all give shape (0, 0, 1, 1)."""
    if isinstance(weights, np.ndarray):
        arr = weights
    else:
        weights = list(weights)
        if not weights:
            return np.zeros((0, 0, 1, 1), dtype=object)
        try:
            arr = np.array(weights, dtype=object)
        except ValueError as exc:
            raise ValueError("the kernel must be a rectangular nesting [O][C][kh][kw]") from exc
    if arr.ndim == 2 and arr.shape[1] == 0:
        arr = arr.reshape(arr.shape[0], 0, 1, 1)
    if arr.ndim != 4:
        raise ValueError(f"the kernel must have rank 4 ([O][C][kh][kw]), not {arr.ndim}")
    if arr.dtype != object:
        if arr.dtype.kind not in "iu":
            raise ValueError("the kernel must hold integers")
        arr = arr.astype(object)
    return arr


@dataclass
class ConvPlan(TwoPassPlan):
    """Launch.index >= 0 in pass 1: the table of the tap at position 0; pass 2 runs on mx_matmul_nsquare_run."""
    shape: Tuple[int, int, int, int]      # (B, C, H, W) of the input
    n_rows: int                           # O, the kernels
    kernel: Tuple[int, int]
    stride: Tuple[int, int]
    padding: Tuple[int, int]
    dilation: Tuple[int, int]
    out_h: int
    out_w: int
    x_ch: List[int]                       # channels with a grid of their own (a positive tap somewhere), ascending
    inverted: List[int]                   # channels whose inverses get a grid (a negative tap somewhere), ascending
    tile_images: int                      # images per tile (1 when an image is cut into bands)
    band_rows: int                        # output rows per tile (out_h when tiles hold whole images)
    origin: np.ndarray                    # [tile_images * band_rows * out_w] int64: a ragged tile takes a prefix

    @property
    def n_grids(self) -> int:
        return len(self.x_ch) + len(self.inverted)

    @property
    def padded_w(self) -> int:
        return self.shape[3] + 2 * self.padding[1]

    def rows_in(self, out_rows: int) -> int:
        """Input rows (of the padded grid) that `out_rows` consecutive output rows read."""
        return (out_rows - 1) * self.stride[0] + self.dilation[0] * (self.kernel[0] - 1) + 1

    def n_local(self, images: int, out_rows: int) -> int:
        return images * self.rows_in(out_rows) * self.n_grids * self.padded_w

    def tiles(self) -> List[Tuple[int, int, int, int]]:
        """(first image, end image, first output row, end output row) of every tile, in output order."""
        b = self.shape[0]
        if self.band_rows == self.out_h:
            return [(m, min(b, m + self.tile_images), 0, self.out_h) for m in range(0, b, self.tile_images)]
        return [(m, m + 1, y, min(self.out_h, y + self.band_rows)) for m in range(b) for y in range(0, self.out_h, self.band_rows)]


def plan_conv(weights: Any, shape: Sequence[int], n: int, bias: Optional[Sequence[int]],
              shape_fn: Callable[[int, int, int, int, int], Tuple[int, int, int]], stride: Any = 1, padding: Any = 0,
              dilation: Any = 1, table_budget: int = TABLE_BUDGET_BYTES, window: int = 0) -> ConvPlan:
    """The launches of one convolution of B grids [C][H][W] with the public kernel `weights` [O][C][kh][kw] (signed
    ints).  ``shape_fn(n_tables, n_outputs, terms, weight_bits, window) -> (window, chunk_terms, table bytes per input
    and entry)`` is the library's choice for a linear map of that size (mx_multiexp_nsquare_shape).  Raises ValueError —
    before anything is launched — for a kernel of the wrong rank or channel count, a kernel larger than the padded
    grid, stride or dilation < 1, negative padding, a weight out of bounds, a bias of the wrong length, or a budget below
    the band of a single output row."""
    if len(shape) != 4:
        raise ValueError("shape must be (B, C, H, W)")
    B, C, H, W = (int(v) for v in shape)
    if min(B, C, H, W) < 0:
        raise ValueError("shape must be (B, C, H, W) of non-negative sizes")
    sh, sw = _pair(stride, "stride", 1)
    ph, pw = _pair(padding, "padding", 0)
    dh, dw = _pair(dilation, "dilation", 1)
    arr = kernel_array(weights)
    O, kc, kh, kw = arr.shape
    if O and B and kc != C:
        raise ValueError(f"the kernel has {kc} channels, the grids have {C}")
    if kh < 1 or kw < 1:
        raise ValueError("the kernel must have at least one tap per channel")
    bias_res = bias_residues(bias, O, n, "kernels")
    Hp, Wp = H + 2 * ph, W + 2 * pw
    span_h, span_w = dh * (kh - 1) + 1, dw * (kw - 1) + 1
    if O and B and (span_h > Hp or span_w > Wp):                 # (no grid: nothing to compare the kernel with)
        raise ValueError(f"the kernel spans {span_h} x {span_w}, the padded grid is {Hp} x {Wp}")
    out_h, out_w = output_hw(H, W, kh, kw, (sh, sw), (ph, pw), (dh, dw))
    bound = weight_bound(n)
    taps: List[List[Tuple[int, int, int, int]]] = []          # per kernel (channel, i, j, weight), zero taps dropped
    pos, neg = set(), set()
    for o in range(O):
        row = []
        for c in range(C):
            for i in range(kh):
                for j in range(kw):
                    w = int(arr[o, c, i, j])
                    if w:
                        (pos if w > 0 else neg).add(c)
                        row.append((c, i, j, w))
        check_weights([w for _, _, _, w in row], bound, "kernel", o)
        taps.append(row)
    shared_of = {j: k for k, j in enumerate(sorted(bias_res))}
    x_ch, inverted, grid_of = sign_split(pos, neg)
    G = len(grid_of)
    term_rows: List[List[Term]] = []
    for o, row in enumerate(taps):
        terms = [((i * dh * G + grid_of[c if w > 0 else ~c]) * Wp + j * dw, abs(w)) for c, i, j, w in row]
        if o in shared_of:
            terms.append((-1 - shared_of[o], 1))
        term_rows.append(terms)
    max_terms = max((len(r) for r in term_rows), default=0)
    max_bits = max((w.bit_length() for r in term_rows for _, w in r), default=0)
    n_shared = len(shared_of)
    budget = int(table_budget)

    def rows_in(r: int) -> int:
        return (r - 1) * sh + span_h

    # the window of the whole call as one linear map, lowered (unless it was given) until one output row's band fits
    per_row = G * Wp                                            # tables per input row of one image
    win, _, entry_bytes = shape_fn(B * rows_in(out_h) * per_row + n_shared if out_h else n_shared, O * B * out_h * out_w,
                                   max_terms, max_bits, int(window))
    win = int(window) or int(win)
    while not window and win > 1 and rows_in(1) * per_row + n_shared > budget // (entry_bytes << win):
        win -= 1
    max_tables = budget // (entry_bytes << win)
    tile_images, band_rows = max(1, B), out_h
    if out_h and per_row:
        whole = rows_in(out_h) * per_row
        if whole + n_shared <= max_tables:
            tile_images = max(1, min(B, (max_tables - n_shared) // whole))
        else:
            tile_images = 1
            band_rows = (((max_tables - n_shared) // per_row) - span_h) // sh + 1 if max_tables > n_shared else 0
            if band_rows < 1:
                raise ValueError(f"table_budget {budget} is below the band of one output row: "
                                 f"{rows_in(1) * per_row + n_shared} tables of {entry_bytes << win} bytes")
            band_rows = min(band_rows, out_h)
    # one launch takes at most 2^30 positions
    while tile_images > 1 and tile_images * band_rows * out_w > 1 << 30:
        tile_images -= 1
    _, chunk, _ = shape_fn(tile_images * rows_in(band_rows) * per_row + n_shared if out_h else n_shared,
                           O * tile_images * band_rows * out_w, max_terms, max_bits, win)
    chunk = max(1, int(chunk))
    p1, result, split = split_k(term_rows, chunk)
    m, y, x = np.meshgrid(np.arange(tile_images, dtype=np.int64), np.arange(band_rows, dtype=np.int64),
                          np.arange(out_w, dtype=np.int64), indexing="ij")
    origin = ((m * rows_in(band_rows) + y * sh) * per_row + x * sw).reshape(-1) if out_h else np.zeros(0, dtype=np.int64)
    plan = ConvPlan(bias=bias_res, window=win, chunk=chunk, launches=_bucket_launches(p1, list(range(len(p1)))),
                    pass1_rows=len(p1), part_rows=[k for ks in split for k in ks], combine=combine_launches(split),
                    result=result, shape=(B, C, H, W), n_rows=O, kernel=(kh, kw), stride=(sh, sw), padding=(ph, pw),
                    dilation=(dh, dw), out_h=out_h, out_w=out_w, x_ch=x_ch, inverted=inverted, tile_images=tile_images,
                    band_rows=band_rows, origin=np.ascontiguousarray(origin, dtype=np.int64))
    check_addresses(plan)
    return plan


def check_addresses(plan: ConvPlan) -> None:
    """The first line of defence of the kernel's address rule: for every tile shape the plan launches, the largest
    index plus the largest origin names a table of the tile.  ValueError otherwise (a planner bug, never an input)."""
    top = max((int(l.index.max()) for l in plan.launches if l.index.size), default=-1)
    if top < 0 or not plan.origin.size:
        return
    for m0, m1, y0, y1 in {(0, m1 - m0, 0, y1 - y0) for m0, m1, y0, y1 in plan.tiles()}:
        positions = (m1 - m0) * (y1 - y0) * plan.out_w
        if positions and (int(plan.origin[:positions].min()) < 0 or
                          top + int(plan.origin[:positions].max()) >= plan.n_local(m1 - m0, y1 - y0)):
            raise ValueError("a tap of the plan lies outside its tile's tables")


def execute_conv(plan: ConvPlan, be: Any, inputs: Any) -> Any:
    """Runs `plan` on backend `be` over the input rows `inputs` ([b][c][y][x], row-major) and returns the result rows
    [b][o][y'][x'].  The backend provides
      ``grids(inputs, shape, x_ch, inverted, padding)``: the padded grids [image][padded row][grid][padded column] — the
        channels x_ch as they are, then the element-wise inverses of the channels `inverted` (ValueError if some pixel is
        not invertible), padded pixels the value 1;
      ``window(grids, m0, m1, r0, r1)``: its rows of images m0 .. m1 - 1 and padded rows r0 .. r1 - 1, in that order;
      ``bias_rows(residues)``: the rows 1 + b N;  ``concat(parts)``: row sets one behind the other;
      ``run_conv(table_rows or None, n_local, n_shared, launch, window, origin, image_positions)``: the results
        [image][len(launch.rows)][image_positions] of one launch (None: the tables of the previous launch are in place);
      ``run_matmul(...)`` as multiexp_plan.execute_matmul describes it (the second pass of split kernels);
      ``select_conv(outs, outs2, picks, images, image_positions, as_columns)``: from the results of the conv launches
        `outs` and of the second-pass launches `outs2`, the entries picks = [(pass, launch, row) or None (= one)] for
        every position — [image][len(picks)][position], or as the column block [pick][image][position] of a second pass;
      ``assemble(tiles, batch, n_rows, out_h, out_w)``: the result rows from tiles = [((m0, m1, y0, y1), rows)].
    The engine's device form is engine._ConvBackend; tests/test_conv_host.py has one over Python ints."""
    B = plan.shape[0]
    if B == 0 or plan.n_rows == 0 or plan.out_h * plan.out_w == 0:
        return be.assemble([], B, plan.n_rows, plan.out_h, plan.out_w)
    shared = sorted(plan.bias)
    grids = be.grids(inputs, plan.shape, plan.x_ch, plan.inverted, plan.padding) if plan.n_grids else None
    bias_rows = be.bias_rows([plan.bias[j] for j in shared]) if shared else None
    part_picks, picks = plan.picks()
    done = []
    for m0, m1, y0, y1 in plan.tiles():
        images, ipos = m1 - m0, (y1 - y0) * plan.out_w
        outs, outs2 = [], []
        if plan.launches:
            parts = []
            if grids is not None:
                r0 = y0 * plan.stride[0]
                parts.append(be.window(grids, m0, m1, r0, r0 + plan.rows_in(y1 - y0)))
            if bias_rows is not None:
                parts.append(bias_rows)
            tables = be.concat(parts)
            n_local = plan.n_local(images, y1 - y0)
            for launch in plan.launches:
                outs.append(be.run_conv(tables, n_local, len(shared), launch, plan.window, plan.origin[: images * ipos], ipos))
                tables = None
        if plan.combine:
            tables = be.select_conv(outs, [], part_picks, images, ipos, True)
            for launch in plan.combine:
                outs2.append(be.run_matmul(tables, len(part_picks), 0, images * ipos, launch, 1))
                tables = None
        done.append(((m0, m1, y0, y1), be.select_conv(outs, outs2, picks, images, ipos, False)))
    return be.assemble(done, B, plan.n_rows, plan.out_h, plan.out_w)
