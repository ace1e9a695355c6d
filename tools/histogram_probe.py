#!/usr/bin/env python3
"""Encrypted histogram against the same groups through the sum of groups.

n encrypted samples, F features of B bins each (a public bin index per feature and sample): n * F terms.
  leg 1, ints to ints, alternating inside one process:
    (a) one Engine.ciphertext_histogram_batch;
    (b) one Engine.ciphertext_sum_batch over the F * B groups of the same ciphertexts (the groups are made outside the timing).
    Medians with the range of wall time and of the kernel time the library's own events measure; the outputs must be
    bit-identical, and two bins are held against plain products.
  leg 2, Engine.histogram_nsquare_t alone on device-resident ciphertext rows and a device-resident bin tensor: wall time to the
    synchronised result, the device span between two events, and the split of that span into the conversion, the
    accumulate level, the combine levels (events around every launch) and the rest — the index arrays, built by torch on the
    same stream.
   python tools/histogram_probe.py [--key-length 2048] [--samples 100000] [--features 10] [--bins 32] [--repeat 5]
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
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--features", type=int, default=10)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-sum-batch", action="store_true", help="leg 1 without form (b)")
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, hist_plan as hp, limbs, synthetic
    from protocols.distributed_keygen_amd.engine import _HistogramBackend

    eng = Engine()
    torch = eng.torch
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    S, F, B = args.samples, args.features, args.bins
    cts = synthetic.random_ciphertexts(key, S, seed=S)
    bins = np.random.default_rng(1).integers(0, B, size=(F, S))
    groups = [[cts[i] for i in np.flatnonzero(bins[f] == b)] for f in range(F) for b in range(B)]
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
        return out, 1e3 * wall, kernel_ms, launches

    # ---- leg 1
    forms = {"a_histogram": lambda: [v for hist in eng.ciphertext_histogram_batch(cts, bins, B, n) for v in hist]}
    if not args.skip_sum_batch:
        forms["b_sum_batch"] = lambda: eng.ciphertext_sum_batch(groups, n)
    for fn in forms.values():                                 # plans, constants, allocator, pinned buffers: outside the timing
        fn()
    times = {k: [] for k in forms}
    outs = {}
    for _ in range(args.repeat):
        for name, fn in forms.items():
            out, wall, kernel_ms, launches = timed(fn)
            times[name].append((wall, kernel_ms, launches))
            outs[name] = out
    identical = all(o == outs["a_histogram"] for o in outs.values())
    for k in (0, F * B - 1):
        want = 1
        for c in groups[k]:
            want = want * c % n2
        identical = identical and outs["a_histogram"][k] == want
    col = lambda name, k: [t[k] for t in times[name]]
    line = {"probe": "histogram", "leg": 1, "key_length": args.key_length, "samples": S, "features": F, "bins": B, "terms": S * F,
            "repeat": args.repeat, "bit_identical": identical,
            "wall_ms": {k: spread(col(k, 0)) for k in forms}, "kernel_ms": {k: spread(col(k, 1)) for k in forms},
            "launches": {k: int(statistics.median(col(k, 2))) for k in forms}}
    if "b_sum_batch" in forms:
        line["speedup_a_over_b_wall"] = round(statistics.median(col("b_sum_batch", 0)) / statistics.median(col("a_histogram", 0)), 2)
        line["kernel_a_over_b"] = round(statistics.median(col("a_histogram", 1)) / statistics.median(col("b_sum_batch", 1)), 2)
    # the parts of (a): packing and upload, the device call, the download
    t0 = time.perf_counter()
    x_t = eng._upload_ints(cts, l2, n2)
    eng.synchronize()
    t1 = time.perf_counter()
    y_t = eng.histogram_nsquare_t(x_t, bins, B, n)
    eng.synchronize()
    t2 = time.perf_counter()
    eng._download_ints(y_t)
    t3 = time.perf_counter()
    line["a_parts_ms"] = {"pack_upload": round(1e3 * (t1 - t0), 1), "device_call": round(1e3 * (t2 - t1), 1), "download": round(1e3 * (t3 - t2), 1)}
    print(json.dumps(line), flush=True)

    # ---- leg 2
    class Timed(_HistogramBackend):
        def __init__(self, *a):
            super().__init__(*a)
            self.marks = []                                   # (part, start event, stop event)
            self.pieces = []

        def _span(self, part, fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            self.marks.append((part, e0, e1))
            return out

        def convert(self, cts_t, lo, hi):
            self.first = True
            return self._span("convert", lambda: super(Timed, self).convert(cts_t, lo, hi))

        def run(self, rows_t, n_rows, index_t, pair_out):
            part, self.first = ("accumulate" if self.first else "combine"), False
            self.pieces.append(tuple(index_t.shape))
            return self._span(part, lambda: super(Timed, self).run(rows_t, n_rows, index_t, pair_out))

    bins_t = torch.as_tensor(bins, device=eng.device)
    eng.histogram_nsquare_t(x_t, bins_t, B, n)
    runs = []
    for _ in range(args.repeat):
        be = Timed(eng, n, l2, n.bit_length())
        eng.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out_t = hp.histogram(be, x_t, bins_t, B)
        e1.record()
        eng.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        parts = {"convert": 0.0, "accumulate": 0.0, "combine": 0.0}
        for part, a, b in be.marks:
            parts[part] += a.elapsed_time(b)
        span = e0.elapsed_time(e1)
        parts["index_arrays_and_gaps"] = span - sum(parts.values())
        runs.append((wall, span, parts, be.pieces))
    identical2 = limbs.unpack(eng.to_host(out_t)) == outs["a_histogram"]
    _, _, kernel_ms, launches = timed(lambda: (eng.histogram_nsquare_t(x_t, bins_t, B, n), eng.synchronize()))
    line2 = {"probe": "histogram", "leg": 2, "key_length": args.key_length, "samples": S, "features": F, "bins": B, "terms": S * F,
             "repeat": args.repeat, "bit_identical": identical2,
             "wall_ms": spread([r[0] for r in runs]), "device_span_ms": spread([r[1] for r in runs]),
             "span_parts_ms": {k: spread([r[2][k] for r in runs], 2) for k in runs[0][2]},
             "levels_pieces_x_chunk": [list(p) for p in runs[-1][3]],
             "kernel_ms_library_events": round(kernel_ms, 1), "launches": launches,
             "row_bytes": be.row_bytes, "staging": list(hp.staging(S, F, be.row_bytes, hp.TABLE_BUDGET_BYTES))}
    print(json.dumps(line2), flush=True)
    assert identical and identical2, "the forms disagree"


if __name__ == "__main__":
    main()
