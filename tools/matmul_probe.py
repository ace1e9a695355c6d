#!/usr/bin/env python3
"""Batched encrypted matrix product against the two ways of composing it from single-vector maps.

One public W (R x I, signed weights of --weight-bits bits, a bias per row) over B encrypted vectors:
  (a) one Engine.ciphertext_matmul_batch;
  (b) a loop of B Engine.ciphertext_linear_map_batch calls;
  (c) one sparse Engine.ciphertext_linear_map_batch over the B * I inputs with B * R sparse rows (only for B <= --sparse-max).
The forms alternate inside one process; medians of wall time from ints to ints and of the kernel time the library's own
events measure (multi-exponentiation table and main kernels; the inverse trees and copies are in the wall time only).
The outputs of the three forms must be bit-identical, and two outputs are held against pow.  For (a) also: the chosen
window, tile and split, the time of its parts, one run with a 1 GiB table budget, and the kernel time of the same
shape with power-of-two weights (one non-zero digit each: what the skipped zero digits are worth).
   python tools/matmul_probe.py [--key-length 2048] [--rows 16] [--cols 256] [--batches 256,1024] [--repeat 3]
"""
import argparse
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
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--cols", type=int, default=256)
    ap.add_argument("--weight-bits", type=int, default=16)
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--sparse-max", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, limbs, multiexp_plan as mp, synthetic

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    rng = random.Random(1)
    R, I = args.rows, args.cols
    half = 1 << (args.weight_bits - 1)
    W = [[rng.randrange(-half, half) for _ in range(I)] for _ in range(R)]
    bias = [rng.randrange(-1000, 1000) for _ in range(R)]
    l2 = limbs.limbs_for(n2)

    def timed(fn):
        eng.synchronize()
        eng.profile(True)
        eng.profile_collect()
        t0 = time.perf_counter()
        out = fn()
        wall = time.perf_counter() - t0
        kernel_ms, launches = eng.profile_collect()
        eng.profile(False)
        return out, wall, kernel_ms, launches

    for B in [int(b) for b in args.batches.split(",")]:
        flat = synthetic.random_ciphertexts(key, B * I, seed=B)
        samples = [flat[b * I : (b + 1) * I] for b in range(B)]
        forms = {
            "a_matmul": lambda: eng.ciphertext_matmul_batch(samples, W, n, bias=bias),
            "b_loop": lambda: [eng.ciphertext_linear_map_batch(smp, W, n, bias=bias) for smp in samples],
        }
        if B <= args.sparse_max:
            sparse = [{b * I + i: w for i, w in enumerate(row) if w} for b in range(B) for row in W]
            forms["c_sparse"] = lambda: (lambda ys: [ys[b * R : (b + 1) * R] for b in range(B)])(
                eng.ciphertext_linear_map_batch(flat, sparse, n, bias=bias * B))
        for fn in forms.values():                             # plans, tables of constants, allocator: outside the timing
            fn()
        times = {k: [] for k in forms}
        outs = {}
        for _ in range(args.repeat):
            for name, fn in forms.items():
                out, wall, kernel_ms, launches = timed(fn)
                times[name].append((wall, kernel_ms, launches))
                outs[name] = out
        identical = all(o == outs["a_matmul"] for o in outs.values())
        for b, j in ((0, 0), (B - 1, R - 1)):
            want = (1 + (bias[j] % n) * n) % n2
            for c, w in zip(samples[b], W[j]):
                want = want * pow(c, w, n2) % n2
            identical = identical and outs["a_matmul"][b][j] == want
        plan = eng._matmul_plan(n, I, B, W, bias)
        # the parts of (a)
        t0 = time.perf_counter()
        plan = eng._matmul_plan(n, I, B, W, bias)
        t1 = time.perf_counter()
        x_t = eng._upload_ints(flat, l2, n2)
        eng.synchronize()
        t2 = time.perf_counter()
        ev0, ev1 = eng.torch.cuda.Event(enable_timing=True), eng.torch.cuda.Event(enable_timing=True)
        ev0.record()
        y_t = eng._matmul_run_t(x_t, B, n, plan)
        ev1.record()
        eng.synchronize()
        t3 = time.perf_counter()
        eng._download_ints(y_t)
        t4 = time.perf_counter()
        parts = {"plan_ms": 1e3 * (t1 - t0), "upload_ms": 1e3 * (t2 - t1), "device_wall_ms": 1e3 * (t3 - t2),
                 "device_span_ms": ev0.elapsed_time(ev1), "download_ms": 1e3 * (t4 - t3)}
        (big, wall_big, kernel_big, launches_big) = timed(
            lambda: eng._download_ints(eng.matmul_nsquare_t(x_t, B, W, n, bias=bias, table_budget=1 << 30)))
        big_plan = eng._matmul_plan(n, I, B, W, bias, table_budget=1 << 30)
        identical = identical and [big[b * R : (b + 1) * R] for b in range(B)] == outs["a_matmul"]
        # zero digits: the same shape with every weight a signed power of two (one non-zero digit per weight)
        # against the random weights above — same table columns, same launches
        W_pow2 = [[(1 << rng.randrange(args.weight_bits - 1)) * rng.choice((1, -1)) for _ in range(I)] for _ in range(R)]
        zero = {}
        for name, Wz in (("random", W), ("powers_of_two", W_pow2)):
            pz = eng._matmul_plan(n, I, B, Wz, bias)
            runs = []
            for _ in range(args.repeat):
                _, _, kms, _ = timed(lambda: (eng._matmul_run_t(x_t, B, n, pz), eng.synchronize()))
                runs.append(kms)
            zero[name] = {"kernel_ms": round(statistics.median(runs), 1), "window": pz.window, "n_cols": pz.n_cols}
        del x_t, y_t
        med = lambda name, k: statistics.median(t[k] for t in times[name])
        line = {
            "probe": "matmul", "key_length": args.key_length, "rows": R, "cols": I, "weight_bits": args.weight_bits, "batch": B,
            "bit_identical": identical,
            "wall_ms": {k: round(1e3 * med(k, 0), 1) for k in forms},
            "kernel_ms": {k: round(med(k, 1), 1) for k in forms},
            "launches": {k: int(med(k, 2)) for k in forms},
            "speedup_a_over_b_wall": round(med("b_loop", 0) / med("a_matmul", 0), 2),
            "a_plan": {"window": plan.window, "tile_batch": plan.tile_batch, "chunk": plan.chunk, "n_cols": plan.n_cols,
                       "pass1_rows": plan.pass1_rows, "pass2_rows": sum(len(l.rows) for l in plan.combine),
                       "table_budget": mp.TABLE_BUDGET_BYTES},
            "a_parts_ms": {k: round(v, 1) for k, v in parts.items()},
            "a_zero_digits": zero,
            "a_1GiB": {"window": big_plan.window, "tile_batch": big_plan.tile_batch, "chunk": big_plan.chunk,
                       "device_to_ints_wall_ms": round(1e3 * wall_big, 1), "kernel_ms": round(kernel_big, 1), "launches": launches_big},
        }
        print(json.dumps(line), flush=True)
        assert identical, "the forms disagree"


if __name__ == "__main__":
    main()
