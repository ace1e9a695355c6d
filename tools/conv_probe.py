#!/usr/bin/env python3
"""Encrypted convolution against the two ways of composing it from the existing linear operators.

B grids of C x H x W ciphertexts under O public kernels of kh x kw signed --weight-bits weights, a bias per kernel,
zero padding --padding:
  (a) Engine.conv2d_nsquare_t: one table per pixel, the kernels as shared weight rows;
  (b) im2col by index_select on the device rows (a row of the value 1 stands for the taps outside the grid), then
      Engine.matmul_nsquare_t with every output position as a sample, and the permutation to [b][o][y][x];
  (c) one sparse Engine.ciphertext_linear_map_batch per image over its explicit Toeplitz rows (ints to ints: its wall time
      includes the conversions, (a) and (b) run from device rows to device rows).
The forms alternate inside one process; medians of wall time and of the kernel time the library's own events measure
(table and main kernels; the inverse trees, gathers and copies are in the wall time only), and the launches.  The
outputs of the three forms must be bit-identical, and three outputs are held against pow.  The condition on (a): not
slower than (b) in wall and in kernel time beyond (b)'s own spread over its repetitions.
   python tools/conv_probe.py [--key-length 2048] [--batch 4] [--channels 1] [--size 28] [--kernels 8] [--ksize 3] [--padding 1]
"""
import argparse
import itertools
import json
import random
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--size", type=int, default=28)
    ap.add_argument("--kernels", type=int, default=8)
    ap.add_argument("--ksize", type=int, default=3)
    ap.add_argument("--padding", type=int, default=1)
    ap.add_argument("--weight-bits", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import numpy as np

    from protocols.distributed_keygen_amd import Engine, conv_plan as cp, limbs, synthetic

    eng = Engine()
    torch = eng.torch
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    rng = random.Random(1)
    B, C, S, O, K, P = args.batch, args.channels, args.size, args.kernels, args.ksize, args.padding
    half = 1 << (args.weight_bits - 1)
    w = [[[[rng.randrange(-half, half) for _ in range(K)] for _ in range(K)] for _ in range(C)] for _ in range(O)]
    bias = [rng.randrange(-1000, 1000) for _ in range(O)]
    oh, ow = cp.output_hw(S, S, K, K, 1, P, 1)
    l2 = limbs.limbs_for(n2)
    flat = synthetic.random_ciphertexts(key, B * C * S * S, seed=B)
    x_t = eng._upload_ints(flat, l2, n2)

    # (b): the patch entries of every position as indices into the rows of x_t; row B C S S is the value 1
    one_row = B * C * S * S
    cols = np.full((B, oh, ow, C * K * K), one_row, dtype=np.int64)
    # (c): the Toeplitz rows of one image, {input: weight}
    toeplitz = [dict() for _ in range(O * oh * ow)]
    for y, x, (c, i, j) in itertools.product(range(oh), range(ow), itertools.product(range(C), range(K), range(K))):
        yy, xc = y - P + i, x - P + j
        if 0 <= yy < S and 0 <= xc < S:
            cols[:, y, x, (c * K + i) * K + j] = (np.arange(B) * C + c) * S * S + yy * S + xc
            for o in range(O):
                if w[o][c][i][j]:
                    toeplitz[(o * oh + y) * ow + x][(c * S + yy) * S + xc] = w[o][c][i][j]
    cols_t = torch.as_tensor(cols.reshape(-1), device=eng.device)
    w_rows = [[v for ch in ker for r in ch for v in r] for ker in w]
    one_t = torch.zeros((1, l2), dtype=torch.int32, device=eng.device)
    one_t[0, 0] = 1

    def form_a():
        return eng.conv2d_nsquare_t(x_t, (B, C, S, S), w, n, bias=bias, padding=P)

    def form_b():
        patches = torch.cat([x_t, one_t], dim=0).index_select(0, cols_t)
        y = eng.matmul_nsquare_t(patches, B * oh * ow, w_rows, n, bias=bias)
        return y.view(B, oh * ow, O, l2).permute(0, 2, 1, 3).reshape(-1, l2)

    def form_c():
        per_image = C * S * S
        row_bias = [bias[k // (oh * ow)] for k in range(O * oh * ow)]
        return [eng.ciphertext_linear_map_batch(flat[m * per_image : (m + 1) * per_image], toeplitz, n, bias=row_bias) for m in range(B)]

    forms = {"a_conv": form_a, "b_im2col_matmul": form_b, "c_toeplitz_maps": form_c}

    def timed(fn):
        eng.synchronize()
        eng.profile(True)
        eng.profile_collect()
        t0 = time.perf_counter()
        out = fn()
        eng.synchronize()
        wall = time.perf_counter() - t0
        kernel_ms, launches = eng.profile_collect()
        eng.profile(False)
        return out, wall, kernel_ms, launches

    for fn in forms.values():                                 # plans, tables of constants, allocator: outside the timing
        fn()
    times = {k: [] for k in forms}
    outs = {}
    for _ in range(args.repeat):
        for name, fn in forms.items():
            out, wall, kernel_ms, launches = timed(fn)
            times[name].append((wall, kernel_ms, launches))
            outs[name] = out
    ints = {"a_conv": eng._download_ints(outs["a_conv"]), "b_im2col_matmul": eng._download_ints(outs["b_im2col_matmul"]),
            "c_toeplitz_maps": [v for img in outs["c_toeplitz_maps"] for v in img]}
    identical = all(v == ints["a_conv"] for v in ints.values())
    for m, o, y, x in ((0, 0, 0, 0), (B - 1, O - 1, oh - 1, ow - 1), (B // 2, O // 2, oh // 2, ow // 2)):
        want = (1 + (bias[o] % n) * n) % n2
        for c, i, j in itertools.product(range(C), range(K), range(K)):
            yy, xc = y - P + i, x - P + j
            if 0 <= yy < S and 0 <= xc < S:
                want = want * pow(flat[((m * C + c) * S + yy) * S + xc], w[o][c][i][j], n2) % n2
        identical = identical and ints["a_conv"][((m * O + o) * oh + y) * ow + x] == want
    plan = eng._conv_plan(n, (B, C, S, S), w, bias, 1, P, 1)
    mplan = eng._matmul_plan(n, C * K * K, B * oh * ow, w_rows, bias)
    med = lambda name, k: statistics.median(t[k] for t in times[name])
    spread = lambda name, k: max(t[k] for t in times[name]) - min(t[k] for t in times[name])
    tiles = plan.tiles()
    line = {
        "probe": "conv", "key_length": args.key_length, "batch": B, "channels": C, "size": S, "kernels": O, "ksize": K,
        "padding": P, "weight_bits": args.weight_bits, "positions": B * oh * ow, "bit_identical": identical,
        "wall_ms": {k: round(1e3 * med(k, 0), 1) for k in forms},
        "kernel_ms": {k: round(med(k, 1), 1) for k in forms},
        "launches": {k: int(med(k, 2)) for k in forms},
        "runs_wall_ms": {k: [round(1e3 * t[0], 1) for t in times[k]] for k in forms},
        "runs_kernel_ms": {k: [round(t[1], 1) for t in times[k]] for k in forms},
        "b_spread_ms": {"wall": round(1e3 * spread("b_im2col_matmul", 0), 1), "kernel": round(spread("b_im2col_matmul", 1), 1)},
        "a_not_slower_than_b": {"wall": med("a_conv", 0) <= med("b_im2col_matmul", 0) + spread("b_im2col_matmul", 0),
                                "kernel": med("a_conv", 1) <= med("b_im2col_matmul", 1) + spread("b_im2col_matmul", 1)},
        "a_plan": {"window": plan.window, "tile_images": plan.tile_images, "band_rows": plan.band_rows, "tiles": len(tiles),
                   "chunk": plan.chunk, "grids": plan.n_grids, "tables": sum(plan.n_local(m1 - m0, y1 - y0) + len(plan.bias) for m0, m1, y0, y1 in tiles),
                   "inverted_pixels": B * len(plan.inverted) * S * S, "pass1_rows": plan.pass1_rows},
        "b_plan": {"window": mplan.window, "tile_batch": mplan.tile_batch, "chunk": mplan.chunk, "n_cols": mplan.n_cols,
                   "tables": mplan.n_cols * B * oh * ow + len(mplan.bias), "inverted_entries": len(mplan.inverted) * B * oh * ow},
    }
    print(json.dumps(line), flush=True)
    assert identical, "the forms disagree"


if __name__ == "__main__":
    main()
