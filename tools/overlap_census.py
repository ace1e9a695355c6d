#!/usr/bin/env python3
"""Which streams' modexp kernels ran side by side: a census of a rocprofv3 --kernel-trace of bench.py.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --steps 16
  python tools/overlap_census.py DIR [--kernel powmod_n2_kernel] [--last 80]

Reads DIR/**/*_kernel_trace.csv, keeps the dispatches whose kernel name contains --kernel and of those the LAST
--last by start time (the timed steps: 16 steps x 5 launches; 0 = all of them), groups them by the stream they were
enqueued on (column Stream_Id; Queue_Id where the trace has no stream column) and prints
  - per stream: launches, the hardware queue(s) its dispatches went through, summed execution time;
  - per pair of streams: for how long kernels of both were executing at the same moment — a pair that NEVER overlaps
    serialises, which is what two streams on one hardware queue do;
  - the time-averaged number of instances executing over the window from the first start to the last end
    (= summed execution time / window), the figure bench.py's kernel_ms / ms_per_step estimates.
"""
import argparse
import csv
import glob
import sys
from collections import defaultdict


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--kernel", default="powmod_n2_kernel")
    ap.add_argument("--last", type=int, default=80)
    args = ap.parse_args()
    rows = []
    for f in glob.glob(args.trace_dir + "/**/*_kernel_trace.csv", recursive=True):
        with open(f, newline="") as fh:
            rows += [r for r in csv.DictReader(fh) if args.kernel in r["Kernel_Name"]]
    if not rows:
        print(f"no dispatch of a kernel named *{args.kernel}* under {args.trace_dir}")
        return 1
    by = "Stream_Id" if "Stream_Id" in rows[0] else "Queue_Id"
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r[by], r.get("Queue_Id", "?")) for r in rows)
    total = len(ev)
    if args.last > 0:
        ev = ev[-args.last:]
    t_lo, t_hi = min(e[0] for e in ev), max(e[1] for e in ev)
    print(f"{len(ev)} of {total} dispatches of *{args.kernel}*, grouped by {by}; window {(t_hi - t_lo) / 1e6:.2f} ms")
    streams = sorted({e[2] for e in ev}, key=lambda s: (len(s), s))
    busy = defaultdict(int)
    queues = defaultdict(set)
    count = defaultdict(int)
    for s, e, st, q in ev:
        busy[st] += e - s
        queues[st].add(q)
        count[st] += 1
    for st in streams:
        print(f"  {by} {st}: {count[st]} launches on hardware queue(s) {sorted(queues[st])}, executing {busy[st] / 1e6:.2f} ms "
              f"({busy[st] / count[st] / 1e6:.2f} ms per launch)")
    # pairwise: time during which both streams had a kernel executing
    both = defaultdict(int)
    for i, (s0, e0, a, _) in enumerate(ev):
        for s1, e1, b, _ in ev[i + 1:]:
            if s1 >= e0:
                break                                    # sorted by start: nothing later begins before e0 either
            if a != b:
                both[tuple(sorted((a, b)))] += min(e0, e1) - s1
    print("  executing at the same moment, ms per pair of streams:")
    for i, a in enumerate(streams):
        for b in streams[i + 1:]:
            ms = both[tuple(sorted((a, b)))] / 1e6
            print(f"    {a} + {b}: {ms:9.2f}" + ("   NEVER: these two serialise" if ms == 0 else ""))
    for st in streams:
        never = [o for o in streams if o != st and both[tuple(sorted((st, o)))] == 0]
        print(f"  {by} {st} never overlaps: {', '.join(never) if never else 'nobody — it ran beside every other stream'}")
    # the time-averaged number of instances executing, and how long exactly k were
    edges = sorted([(s, 1) for s, _, _, _ in ev] + [(e, -1) for _, e, _, _ in ev])
    level, last, at = 0, t_lo, defaultdict(int)
    for t, d in edges:
        at[level] += t - last
        level, last = level + d, t
    avg = sum(busy.values()) / (t_hi - t_lo)
    print(f"  instances executing, time average over the window: {avg:.2f}")
    print("  share of the window with exactly k executing: " + ", ".join(f"{k}: {100 * v / (t_hi - t_lo):.1f} %" for k, v in sorted(at.items()) if v))
    return 0


if __name__ == "__main__":
    sys.exit(main())
