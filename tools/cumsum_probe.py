#!/usr/bin/env python3
"""Encrypted prefix sums against the routes they replace.

  shape A, split sums: S series of B ciphertexts (the bins of S histograms), alternating inside one process:
    (a) one Engine.ciphertext_cumsum_batch;
    (b) the best existing route, a sweep of B - 1 Engine.mulmod_batch calls over S elements (column j times the running
        column), every intermediate through Python ints.
    Wall time ints to ints and the kernel time the library's own events measure, medians with their range; then both
    device-resident (cumsum_nsquare_t against B - 1 mulmod_t calls on rows that are already there), from the call to the
    synchronised result.  The outputs must be bit-identical, and one series is held against plain products.
  shape B, one series of L ciphertexts, device-resident: wall time, the device span between two events, the span split
    by launch kind and level (events around every launch) and the launches; against the same L elements as L / 32
    series of 32, which need no carries; and, at --map-elements elements only, against ciphertext_linear_map_batch with
    a triangular W of ones.
   python tools/cumsum_probe.py [--key-length 2048] [--series 2000] [--bins 32] [--long 100000] [--map-elements 2048] [--repeat 5]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def spread(values, digits=1):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--series", type=int, default=2000)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--long", type=int, default=100000)
    ap.add_argument("--map-elements", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--parts", default="ab", help="a: split sums, b: one long series")
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, limbs, scan_plan as sp, synthetic
    from protocols.distributed_keygen_amd.engine import _ScanBackend

    eng = Engine()
    torch = eng.torch
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    l2 = limbs.limbs_for(n2)
    S, B, L = args.series, args.bins, args.long
    pool = synthetic.random_ciphertexts(key, max(S * B, L), seed=S)

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
        """Every form once outside the timing (plans, constants, allocator, pinned buffers), then `repeat` rounds of all."""
        for fn in forms.values():
            fn()
        times = {k: [] for k in forms}
        outs = {}
        for _ in range(args.repeat):
            for name, fn in forms.items():
                out, wall, kernel_ms, launches = timed(fn)
                times[name].append((wall, kernel_ms, launches))
                outs[name] = out
        col = lambda name, k: [t[k] for t in times[name]]
        return outs, {"wall_ms": {k: spread(col(k, 0)) for k in forms}, "kernel_ms": {k: spread(col(k, 1), 2) for k in forms},
                      "launches": {k: int(statistics.median(col(k, 2))) for k in forms}}

    if "a" in args.parts:
        cts = pool[: S * B]
        lengths = [B] * S
        cols = [cts[j::B] for j in range(B)]                  # column j: element j of every series (made outside the timing)

        def sweep():
            acc, out = cols[0], [cols[0]]
            for j in range(1, B):
                acc = eng.mulmod_batch(acc, cols[j], n2)
                out.append(acc)
            return [out[j][s] for s in range(S) for j in range(B)]

        outs, stats = alternate({"a_cumsum": lambda: eng.ciphertext_cumsum_batch(cts, lengths, n), "b_mulmod_sweep": sweep})
        identical = outs["a_cumsum"] == outs["b_mulmod_sweep"]
        acc = 1
        for j in range(B):
            acc = acc * cts[(S - 1) * B + j] % n2
            identical = identical and outs["a_cumsum"][(S - 1) * B + j] == acc
        line = {"probe": "cumsum", "shape": "A", "form": "ints_to_ints", "key_length": args.key_length, "series": S, "bins": B,
                "repeat": args.repeat, "bit_identical": identical, **stats}
        line["speedup_a_over_b_wall"] = round(stats["wall_ms"]["b_mulmod_sweep"]["median"] / stats["wall_ms"]["a_cumsum"]["median"], 2)
        print(json.dumps(line), flush=True)
        # device-resident: rows in, rows out
        x_t = eng._upload_ints(cts, l2, n2)
        cols_t = [x_t[j::B].contiguous() for j in range(B)]
        lengths_t = torch.full((S,), B, dtype=torch.int64, device=eng.device)

        def sweep_t():
            acc_t, out = cols_t[0], [cols_t[0]]
            for j in range(1, B):
                acc_t = eng.mulmod_t(acc_t, cols_t[j], n2)
                out.append(acc_t)
            return torch.stack(out, dim=1).reshape(S * B, l2)

        outs_t, stats_t = alternate({"a_cumsum_t": lambda: eng.cumsum_nsquare_t(x_t, lengths_t, n), "b_mulmod_t_sweep": sweep_t})
        identical_t = bool(torch.equal(outs_t["a_cumsum_t"], outs_t["b_mulmod_t_sweep"])) and limbs.unpack(eng.to_host(outs_t["a_cumsum_t"])) == outs["a_cumsum"]
        line = {"probe": "cumsum", "shape": "A", "form": "device_resident", "key_length": args.key_length, "series": S, "bins": B,
                "repeat": args.repeat, "bit_identical": identical_t, **stats_t}
        print(json.dumps(line), flush=True)
        assert identical and identical_t, "the forms disagree"

    if "b" in args.parts:
        class Timed(_ScanBackend):
            def __init__(self, *a):
                super().__init__(*a)
                self.marks = []                               # (part, shape, start event, stop event)

            def _span(self, part, shape, fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                self.marks.append((part, shape, e0, e1))
                return out

            def convert(self, cts_t, lo, hi):
                return self._span("convert", [hi - lo], lambda: super(Timed, self).convert(cts_t, lo, hi))

            def run(self, rows_t, n_rows, index_t, pair_out):
                return self._span("totals", list(index_t.shape), lambda: super(Timed, self).run(rows_t, n_rows, index_t, pair_out))

            def scan(self, rows_t, n_rows, index_t, carry, exclusive):
                return self._span("scan", list(index_t.shape), lambda: super(Timed, self).scan(rows_t, n_rows, index_t, carry, exclusive))

            def store(self, rows_t, n_rows):
                return self._span("store", [n_rows], lambda: super(Timed, self).store(rows_t, n_rows))

        cts = pool[:L]
        x_t = eng._upload_ints(cts, l2, n2)
        shapes = {"one_series": torch.tensor([L], dtype=torch.int64, device=eng.device),
                  "series_of_32": sp.as_lengths([32] * (L // 32) + ([L % 32] if L % 32 else []), L, eng.device)}
        for lengths_t in shapes.values():
            eng.cumsum_nsquare_t(x_t, lengths_t, n)
        runs = {k: [] for k in shapes}
        last = {}
        for _ in range(args.repeat):
            for name, lengths_t in shapes.items():
                be = Timed(eng, n, l2, n.bit_length())
                eng.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                last[name] = sp.cumsum(be, x_t, lengths_t)
                e1.record()
                eng.synchronize()
                wall = 1e3 * (time.perf_counter() - t0)
                runs[name].append((wall, e0.elapsed_time(e1), [(p, s, a.elapsed_time(b)) for p, s, a, b in be.marks]))
        want, acc = [], 1
        for c in cts[:2000]:
            acc = acc * c % n2
            want.append(acc)
        head = limbs.unpack(eng.to_host(last["one_series"][:2000]))
        tail_ok = limbs.unpack(eng.to_host(last["series_of_32"][:32])) == want[:32]
        for name in shapes:
            rs = runs[name]
            launches = [{"launch": p, "shape": s, "ms": spread([r[2][k][2] for r in rs], 3)} for k, (p, s, _) in enumerate(rs[0][2])]
            kinds = {}
            for k, (p, _, _) in enumerate(rs[0][2]):
                kinds.setdefault(p, []).append(k)
            by_kind = {p: spread([sum(r[2][k][2] for k in ks) for r in rs], 3) for p, ks in kinds.items()}
            by_kind["index_arrays_and_gaps"] = spread([r[1] - sum(m[2] for m in r[2]) for r in rs], 3)
            _, _, kernel_ms, n_launch = timed(lambda: eng.cumsum_nsquare_t(x_t, shapes[name], n))
            print(json.dumps({"probe": "cumsum", "shape": "B", "form": name, "key_length": args.key_length, "elements": L,
                              "repeat": args.repeat, "bit_identical_head": head == want and tail_ok,
                              "wall_ms": spread([r[0] for r in rs], 2), "device_span_ms": spread([r[1] for r in rs], 2),
                              "span_by_kind_ms": by_kind, "launches_in_order": launches,
                              "kernel_ms_library_events": round(kernel_ms, 2), "launches": n_launch}), flush=True)
        assert head == want and tail_ok, "the scan disagrees with plain products"
        # against a triangular linear map, where that route is feasible
        M = min(args.map_elements, L)
        small = cts[:M]
        tri = [{i: 1 for i in range(j + 1)} for j in range(M)]
        outs, stats = alternate({"a_cumsum": lambda: eng.ciphertext_cumsum_batch(small, None, n),
                                 "c_triangular_linear_map": lambda: eng.ciphertext_linear_map_batch(small, tri, n)})
        same = outs["a_cumsum"] == outs["c_triangular_linear_map"] == want[:M] if M <= 2000 else outs["a_cumsum"] == outs["c_triangular_linear_map"]
        print(json.dumps({"probe": "cumsum", "shape": "B", "form": "against_linear_map", "key_length": args.key_length,
                          "elements": M, "terms_of_the_map": M * (M + 1) // 2, "repeat": args.repeat, "bit_identical": same, **stats}), flush=True)
        assert same, "the forms disagree"


if __name__ == "__main__":
    main()
