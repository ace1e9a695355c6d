"""The hardware-queue policy of mx_configure_hw_queues (include/mxpaillier.h, csrc/mx_queues.hpp) and of its Python
caller configure_hw_queues: what a request and an inherited GPU_MAX_HW_QUEUES add up to.  The environment is process
state and the library remembers what it configured, so every case runs in a fresh child process; all children are
started together, once, and every test looks at its own child's report.  No GPU is needed: neither function makes a
GPU call (the stand-alone program tools/hw_queue_policy_check.cpp runs the same cases on the decision function alone)."""

from __future__ import annotations

import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

# The child: imports the package (which must configure nothing), then either calls the library for every request in
# turn or the Python wrapper once, and reports what the C environment (getenv, not Python's copy) holds afterwards.
CHILD = r"""
import ctypes, json, os, sys
root, mode, requests = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
sys.path.insert(0, root)
libc = ctypes.CDLL(None)
libc.getenv.restype = ctypes.c_char_p
def c_env():
    v = libc.getenv(b"GPU_MAX_HW_QUEUES")
    return None if v is None else v.decode()
import protocols.distributed_keygen_amd as pkg
from protocols.distributed_keygen_amd import _lib
lib = _lib.lib()
out = {"after_import": c_env(), "configured_after_import": lib.mx_hw_queues_configured()}
if mode == "native":
    out["returns"] = [lib.mx_configure_hw_queues(q) for q in requests]
elif mode == "python":
    out["returns"] = [pkg.configure_hw_queues(q) for q in requests]
elif mode == "late":
    import torch
    torch.cuda.is_initialized = lambda: True          # what torch reports once anything has touched the GPU
    out["returns"] = [pkg.configure_hw_queues(q) for q in requests]
out["c_env"] = c_env()
out["os_environ"] = os.environ.get("GPU_MAX_HW_QUEUES")
out["configured"] = lib.mx_hw_queues_configured()
out["cuda_initialized"] = bool(sys.modules["torch"].cuda.is_initialized()) if mode != "late" else None
print("REPORT " + json.dumps(out))
"""

# name -> (mode, inherited GPU_MAX_HW_QUEUES or None, MX_HW_QUEUES_KEEP or None, requests)
CASES = {
    "unset": ("native", None, None, [16]),
    "inherited_4": ("native", "4", None, [16]),
    "inherited_24": ("native", "24", None, [16]),
    "request_64": ("native", None, None, [64]),
    "request_64_over_4": ("native", "4", None, [64]),
    "request_0": ("native", None, None, [0]),
    "request_negative": ("native", None, None, [-3]),
    "keep_4": ("native", "4", "1", [16]),
    "keep_unset": ("native", None, "1", [16]),
    "garbage": ("native", "lots", None, [16]),
    "second_smaller": ("native", "4", None, [16, 8]),
    "python_4": ("python", "4", None, [16]),
    "python_keep_4": ("python", "4", "1", [16]),
    "python_late": ("late", "4", None, [16]),
}


def _run(name: str) -> dict:
    mode, inherited, keep, requests = CASES[name]
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "MX_HW_QUEUES_KEEP")}
    if inherited is not None:
        env["GPU_MAX_HW_QUEUES"] = inherited
    if keep is not None:
        env["MX_HW_QUEUES_KEEP"] = keep
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), mode, json.dumps(requests)], env=env, capture_output=True,
                       text=True, timeout=300)
    line = next((l for l in r.stdout.splitlines() if l.startswith("REPORT ")), None)
    assert r.returncode == 0 and line, f"{name}: rc={r.returncode}\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(line[len("REPORT "):])


@pytest.fixture(scope="module")
def reports() -> dict:
    with ThreadPoolExecutor(max_workers=8) as pool:
        return dict(zip(CASES, pool.map(_run, CASES)))


@pytest.mark.parametrize("name,returns,c_env", [
    ("unset", [16], "16"),
    ("inherited_4", [16], "16"),                     # an inherited smaller value no longer undercuts the request
    ("inherited_24", [24], "24"),                    # a larger one stays
    ("request_64", [32], "32"),                      # never more than 32
    ("request_64_over_4", [32], "32"),
    ("request_0", [1], "1"),
    ("request_negative", [1], "1"),
    ("keep_4", [4], "4"),                            # MX_HW_QUEUES_KEEP=1: the user's value stands
    ("keep_unset", [0], None),                       # ... also when that is "nothing"
    ("garbage", [16], "16"),                         # unreadable counts as unset
    ("second_smaller", [16, 16], "16"),              # a later, smaller request does not lower it
])
def test_native_policy(reports, name, returns, c_env):
    rep = reports[name]
    assert rep["returns"] == returns and rep["c_env"] == c_env
    assert rep["configured"] == returns[-1], "mx_hw_queues_configured reports what was written or found"
    assert rep["cuda_initialized"] is False, "configuring made a GPU call"


def test_import_and_library_load_configure_nothing(reports):
    for name, (_, inherited, _, _) in CASES.items():
        assert reports[name]["after_import"] == inherited, name
        assert reports[name]["configured_after_import"] == 0, name


def test_python_wrapper_raises_an_inherited_4(reports):
    rep = reports["python_4"]
    assert rep["returns"] == [True] and rep["c_env"] == "16" and rep["os_environ"] == "16" and rep["configured"] == 16
    assert rep["cuda_initialized"] is False


def test_python_wrapper_honours_the_opt_out(reports):
    rep = reports["python_keep_4"]
    assert rep["returns"] == [True] and rep["c_env"] == "4" and rep["os_environ"] == "4" and rep["configured"] == 4


def test_python_wrapper_too_late_changes_nothing(reports):
    rep = reports["python_late"]
    assert rep["returns"] == [False] and rep["c_env"] == "4" and rep["os_environ"] == "4" and rep["configured"] == 0


# configure_hw_queues is the first thing that loads the library in tests/conftest.py and bench.py, ahead of their own build
# steps: it must bring a missing or stale library up to date BEFORE loading it, and leave a fresh one alone.
ORDER_CHILD = r"""
import json, sys
root, stale = sys.argv[1], sys.argv[2] == "stale"
sys.path.insert(0, root)
import protocols.distributed_keygen_amd as pkg
from protocols.distributed_keygen_amd import _lib, build
events = []
real_build, real_load = build.build, _lib.load
if stale:
    build.needs_build = lambda: not any(e == "build" for e in events)      # stale until somebody builds
def fake_build(force=False, verbose=False):
    events.append("build")
    return real_build(force=False) if not stale else build.LIB
def load():
    events.append("load")
    return real_load()
build.build, _lib.load = fake_build, load
ok = pkg.configure_hw_queues(16)
print("REPORT " + json.dumps({"ok": ok, "events": events}))
"""


@pytest.mark.parametrize("state,events", [("stale", ["build", "load"]), ("fresh", ["load"])])
def test_wrapper_builds_a_stale_library_before_it_loads_it(state, events):
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "MX_HW_QUEUES_KEEP")}
    r = subprocess.run([sys.executable, "-c", ORDER_CHILD, str(ROOT), state], env=env, capture_output=True, text=True, timeout=300)
    line = next((l for l in r.stdout.splitlines() if l.startswith("REPORT ")), None)
    assert r.returncode == 0 and line, f"rc={r.returncode}\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    rep = json.loads(line[len("REPORT "):])
    assert rep == {"ok": True, "events": events}
