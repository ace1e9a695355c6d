#!/usr/bin/env python3
"""Encrypted sparse matrix product against the same matrix through the linear map on dict rows.

n_in encrypted inputs, R rows, `per_column` stored weights per column at random rows (signed, `weight_bits` bits).
Alternating inside one process, after a warm-up of each form:
    (a) Engine.ciphertext_spmm_batch on the CSR arrays;
    (b) Engine.ciphertext_linear_map_batch on the same rows as ``{column: weight}`` dicts (made outside the timing;
        duplicate entries added up).
  ints to ints: wall time; kernel time: what the library's own events measure in the same calls; device-resident:
  Engine.spmm_nsquare_t on device rows and device index tensors against Engine.multiexp_nsquare_t on the same rows and the
  dict rows, wall time to the synchronised result.  Medians with the range; the outputs must be bit-identical, and two rows
  are held against ``pow``.
   python tools/spmm_probe.py [--key-length 2048] [--inputs 100000] [--rows 1024] [--per-column 10] [--weight-bits 16] [--repeat 5]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def spread(values, digits=1):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--inputs", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--per-column", type=int, default=10)
    ap.add_argument("--weight-bits", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, limbs, spmm_plan as sp, synthetic

    eng = Engine()
    torch = eng.torch
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    I, R, P = args.inputs, args.rows, args.per_column
    cts = synthetic.random_ciphertexts(key, I, seed=I)
    rng = np.random.default_rng(1)
    col = np.repeat(np.arange(I), P)
    row = rng.integers(0, R, size=I * P)
    half = 1 << (args.weight_bits - 1)
    val = rng.integers(-half, half, size=I * P)
    order = np.argsort(row, kind="stable")
    row, col, val = row[order], col[order], val[order]
    crow = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=R))])
    dicts = [{} for _ in range(R)]
    for r, c, v in zip(row.tolist(), col.tolist(), val.tolist()):
        dicts[r][c] = dicts[r].get(c, 0) + v
    l2 = limbs.limbs_for(n2)
    bits = int(np.abs(val).max()).bit_length()
    inverted = int(np.unique(col[val < 0]).size)
    w, positions, row_bytes = eng.spmm_nsquare_shape(n, I + inverted, R, int((val != 0).sum()), bits)
    print(json.dumps({"probe": "spmm", "setup": True, "inputs": I, "rows": R, "nnz": int(col.size), "weight_bits": bits,
                      "inverted_columns": inverted, "window": w, "positions": positions, "row_bytes": row_bytes}), flush=True)

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
        return out, 1e3 * wall, kernel_ms, launches

    def alternate(forms):
        for name, fn in forms.items():                            # plans, constants, allocator, pinned buffers: outside the timing
            fn()
            print(json.dumps({"probe": "spmm", "warmed": name}), flush=True)
        times = {k: [] for k in forms}
        outs = {}
        for _ in range(args.repeat):
            for name, fn in forms.items():
                out, wall, kernel_ms, launches = timed(fn)
                times[name].append((wall, kernel_ms, launches))
                outs[name] = out
        return times, outs

    column = lambda times, name, k: [t[k] for t in times[name]]
    # ---- ints to ints, and the kernel time of the same calls
    forms = {"a_spmm": lambda: eng.ciphertext_spmm_batch(cts, crow, col, val, n),
             "b_linear_map_dicts": lambda: eng.ciphertext_linear_map_batch(cts, dicts, n)}
    times, outs = alternate(forms)
    identical = outs["a_spmm"] == outs["b_linear_map_dicts"]
    for r in (0, R - 1):
        want = 1
        for t in range(int(crow[r]), int(crow[r + 1])):
            want = want * pow(cts[int(col[t])], int(val[t]), n2) % n2
        identical = identical and outs["a_spmm"][r] == want
    line = {"probe": "spmm", "leg": "ints_to_ints", "key_length": args.key_length, "inputs": I, "rows": R, "nnz": int(col.size),
            "weight_bits": bits, "window": w, "repeat": args.repeat, "bit_identical": identical,
            "wall_ms": {k: spread(column(times, k, 0)) for k in forms}, "kernel_ms": {k: spread(column(times, k, 1)) for k in forms},
            "launches": {k: int(statistics.median(column(times, k, 2))) for k in forms},
            "speedup_a_over_b_wall": round(statistics.median(column(times, "b_linear_map_dicts", 0)) / statistics.median(column(times, "a_spmm", 0)), 2),
            "kernel_a_over_b": round(statistics.median(column(times, "a_spmm", 1)) / statistics.median(column(times, "b_linear_map_dicts", 1)), 2)}
    print(json.dumps(line), flush=True)

    # ---- device-resident
    x_t = eng._upload_ints(cts, l2, n2)
    crow_t, col_t, val_t = (torch.as_tensor(v, device=eng.device) for v in (crow, col, val))
    forms2 = {"a_spmm_t": lambda: eng.spmm_nsquare_t(x_t, crow_t, col_t, val_t, n),
              "b_multiexp_t_dicts": lambda: eng.multiexp_nsquare_t(x_t, dicts, n)}
    times2, outs2 = alternate(forms2)
    identical2 = all(limbs.unpack(eng.to_host(o)) == outs["a_spmm"] for o in outs2.values())
    keys_t, _, _, plus_t, minus_t = sp.digit_terms(crow_t, col_t, val_t, I, w, positions)
    tables = int(plus_t.numel() + minus_t.numel())
    stages = -(-tables // sp.staging(tables, int(keys_t.numel()), w, row_bytes, sp.TABLE_BUDGET_BYTES))
    line2 = {"probe": "spmm", "leg": "device_resident", "key_length": args.key_length, "inputs": I, "rows": R, "nnz": int(col.size),
             "repeat": args.repeat, "bit_identical": identical2, "tables": tables, "digit_terms": int(keys_t.numel()), "stages": stages,
             "wall_ms": {k: spread(column(times2, k, 0)) for k in forms2}, "kernel_ms": {k: spread(column(times2, k, 1)) for k in forms2},
             "launches": {k: int(statistics.median(column(times2, k, 2))) for k in forms2},
             "speedup_a_over_b_wall": round(statistics.median(column(times2, "b_multiexp_t_dicts", 0)) / statistics.median(column(times2, "a_spmm_t", 0)), 2)}
    print(json.dumps(line2), flush=True)
    assert identical and identical2, "the forms disagree"


if __name__ == "__main__":
    main()
