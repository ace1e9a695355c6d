#!/usr/bin/env python3
"""What the benchmark's process gets from the HIP runtime: the GPU_MAX_HW_QUEUES it runs under and which of its
streams run side by side.  Creates the engine and the streams in bench.py's order (importing bench calls
configure_hw_queues as a run of it does), then measures with one-wavefront spins (mx_spin), which do no work:

  python tools/hw_queue_census.py [--extra 8] [--spin-us 2000]

  - GPU_MAX_HW_QUEUES before the import and right after configure_hw_queues returned;
  - the census (Engine.stream_census = mx_stream_census) over the four streams bench.lane_stream hands out: which run
    side by side, and for the others the lane they serialise with;
  - every pair of those four alone;
  - the same census over --extra further streams created afterwards: how many streams of this process run side by
    side at all — with N hardware queues in effect no more than N can.
"""
import argparse
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--extra", type=int, default=8)
ap.add_argument("--spin-us", type=int, default=2000)
args = ap.parse_args()
sys.argv = sys.argv[:1]                                     # bench reads --hw-queues from sys.argv at import

print(f"GPU_MAX_HW_QUEUES inherited: {os.environ.get('GPU_MAX_HW_QUEUES', '(unset)')}; MX_HW_QUEUES_KEEP: {os.environ.get('MX_HW_QUEUES_KEEP', '(unset)')}")
import bench  # noqa: E402  (calls configure_hw_queues(16) at import, as a run of bench.py does)

print(f"GPU_MAX_HW_QUEUES after configure_hw_queues({bench.HW_QUEUES}): {os.environ.get('GPU_MAX_HW_QUEUES', '(unset)')}", flush=True)
import torch  # noqa: E402

from protocols.distributed_keygen_amd import Engine  # noqa: E402

torch.cuda.set_device(0)
eng = Engine(0)
eng.selftest_lanes()                                        # work on the default stream first, as the untimed set-up does
lanes = [bench.lane_stream(torch, k, 4) for k in range(4)]
torch.cuda.synchronize()


def census(streams):
    groups = eng.stream_census(streams, spin_us=args.spin_us)           # mx_stream_census: the library's own timing
    return [k for k, g in enumerate(groups) if g == k], groups


ok, groups = census(lanes)
print(f"mx_stream_census over the 4 lane streams: {len(ok)} side by side: lanes {ok}; group of every lane: {groups}", flush=True)
print("two lanes alone:")
for i in range(4):
    for j in range(i + 1, 4):
        side = len(census([lanes[i], lanes[j]])[0]) == 2
        print(f"  lane {i} + lane {j}: {'side by side' if side else 'serialise'}", flush=True)
if args.extra > 0:
    more = lanes + [torch.cuda.Stream() for _ in range(args.extra)]
    ok, groups = census(more)
    print(f"of the 4 lanes + {args.extra} further streams, {len(ok)} run side by side: {ok}; group of every stream: {groups}", flush=True)
