"""A process that inherits GPU_MAX_HW_QUEUES=4 and asks for 16 gets them: four streams created after
configure_hw_queues(16) run side by side, by the native census (mx_stream_census) and by Engine.stream_concurrency,
which is a thin caller of it.  The number of hardware queues is read once, when the runtime initialises, so each
case is a fresh child process."""

from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

CHILD = r"""
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
from protocols.distributed_keygen_amd import configure_hw_queues
in_time = configure_hw_queues(16)
import torch
from protocols.distributed_keygen_amd import Engine
eng = Engine(0)
streams = [torch.cuda.Stream() for _ in range(4)]
ptrs = (ctypes.c_void_p * 4)(*[int(s.cuda_stream) for s in streams])
groups = (ctypes.c_int * 4)()
accepted = eng.lib.mx_stream_census(ptrs, 4, 2000, groups)          # 2 ms spins
same = eng.stream_concurrency(streams, spin_us=2000)
print("REPORT " + json.dumps({"in_time": in_time, "queues": os.environ.get("GPU_MAX_HW_QUEUES"), "configured": eng.lib.mx_hw_queues_configured(),
                              "accepted": accepted, "groups": list(groups), "stream_concurrency": [streams.index(s) for s in same],
                              "late": eng.lib.mx_configure_hw_queues(16)}))
"""


def _child(keep: bool) -> dict:
    env = {k: v for k, v in os.environ.items() if k != "MX_HW_QUEUES_KEEP"}
    env["GPU_MAX_HW_QUEUES"] = "4"
    if keep:
        env["MX_HW_QUEUES_KEEP"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=120)
    line = next((l for l in r.stdout.splitlines() if l.startswith("REPORT ")), None)
    assert r.returncode == 0 and line, f"rc={r.returncode}\n{r.stdout[-500:]}\n{r.stderr[-3000:]}"
    return json.loads(line[len("REPORT "):])


def test_four_streams_get_queues_of_their_own_over_an_inherited_4():
    rep = _child(keep=False)
    print("inherited 4, asked for 16:", rep)
    assert rep["in_time"] is True and rep["queues"] == "16" and rep["configured"] == 16
    assert rep["accepted"] == 4 and rep["groups"] == [0, 1, 2, 3], "streams of a process with 16 hardware queues serialise"
    assert rep["stream_concurrency"] == [0, 1, 2, 3]
    assert rep["late"] == -6, "mx_configure_hw_queues after the library's first GPU call must report MX_ERR_STATE"
    # (only after the first child ended well) the opt-out: the user's 4 stands; how the runtime then maps four streams
    # onto its queues is its own business, so the census is printed and not judged
    kept = _child(keep=True)
    print("inherited 4 kept (MX_HW_QUEUES_KEEP=1):", kept)
    assert kept["queues"] == "4" and kept["configured"] == 4
