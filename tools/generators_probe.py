"""The generator step of a key-generation round (`__biprime_test_g_generation`) on the device against
the host loop it replaces, on the device and the box in use.

    python tools/generators_probe.py [--out DIR] [--quick] [--reps 5]

At key_length 2048 with 1417 survivors x 160 generators and 3 parties (what a round of 65 536 candidates leaves), single
process, one party's work.  Both paths start from ints — the other parties' shares as the exchange delivers them — and
end with the generator rows on the device that ``Engine.biprime_v_t`` takes:

  host loop    the reference's way: ``randint(0, N)`` per own share (DK:1042), ``sum(shares) % N`` per generator
               (``AdditiveVariable.reconstruct`` without its objects), then the nested pack and upload of
               ``biprime_v_batch`` (one run: it takes most of a second)
  device path  ``generator_shares_batch`` (draw, reduce, the own shares as ints for the exchange) and
               ``generator_sum_batch`` with the own rows taken from the device and the others' lists packed and uploaded
  kernels      events around the launches alone: the rows of the generator, the share kernel on rows drawn beforehand,
               the sum kernel on share rows already on the device (each with its per-modulus set-up launch)

A sample of the device path's output is checked against tools/generators_model.py.  Writes DIR/generators_probe.json.
"""

from __future__ import annotations

import argparse
import json
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles", help="directory of the result file (default: profiles/)")
    ap.add_argument("--quick", action="store_true", help="an eighth of the survivors (a smoke run of the probe itself)")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch

    import generators_model as gm
    from protocols.distributed_keygen_amd import DeviceRng, Engine, limbs

    eng = Engine(0)
    key_length, S, G, parties = 2048, 1417 // (8 if args.quick else 1), 160, 3
    rnd = random.Random(2048)
    mods = [rnd.getrandbits(key_length + 2) | (1 << (key_length + 1)) | 1 for _ in range(S)]
    others = [[[rnd.randrange(n + 1) for _ in range(G)] for n in mods] for _ in range(parties - 1)]
    lw = limbs.limbs_for_bits(limbs.max_bits(mods))
    bits, cw = gm.draw_bits(mods), gm.draw_words(mods)
    seed = bytes(range(32))
    rng = DeviceRng(key=seed)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def event_s(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    def device_path():
        lists, rows = eng.generator_shares_batch(mods, G, rng, keep_rows=True)
        return lists, eng.generator_sum_batch([rows] + others, mods, G, keep_rows=True)

    def host_loop():
        sysrand = random.Random(7)
        own = [[sysrand.randint(0, n) for _ in range(G)] for n in mods]
        cols = [own] + others
        g = [[sum(col[c][k] for col in cols) % n for k in range(G)] for c, n in enumerate(mods)]
        return own, eng._staged_rows("generators", g, lw, mods, nested=G), g

    device_path()                                                   # first launches, workspaces, staging buffers
    mods_t = eng.to_device(limbs.pack(mods, lw))
    tm = {k: [] for k in ("rng", "share_kernels", "sum_kernels", "device")}
    for _ in range(args.reps):
        dt, draws_t = event_s(lambda: rng.rows_t(eng, S * G, bits, cw))
        tm["rng"].append(dt)
        dt, own_t = event_s(lambda: eng.generator_shares_t((mods_t, bits - 64), G, draws_t=draws_t))
        tm["share_kernels"].append(dt)
        shares_t = torch.stack([own_t] * parties)
        tm["sum_kernels"].append(event_s(lambda: eng.generator_sum_t(shares_t, (mods_t, bits - 64), G))[0])
        del draws_t, own_t, shares_t
        call = rng.next_call
        dt, (lists, g_t) = wall(device_path)
        tm["device"].append(dt)
    want = gm.shares(seed, call, mods[:2], G)                        # the first rows of a call do not depend on its count
    assert lists[:2] == want, "the device path's shares differ from the model"
    table = {0: lists[:2], **{j + 1: col[:2] for j, col in enumerate(others)}}
    assert limbs.unpack(eng.to_host(g_t[: 2 * G])) == [g for row in gm.generators(table, mods[:2], G) for g in row]
    t_host, (own, rows_t, g) = wall(host_loop)
    assert tuple(rows_t.shape) == tuple(g_t.shape)
    med = {k: statistics.median(v) for k, v in tm.items()}
    result = {
        "probe": "generators", "key_length": key_length, "survivors": S, "generators_each": G, "parties": parties,
        "rows": S * G, "modulus_bits": bits - 64, "reps": args.reps, "device": torch.cuda.get_device_name(0),
        "host_loop_ms": round(1e3 * t_host, 3),
        "device_path_ms": {"median": round(1e3 * med["device"], 3), "min": round(1e3 * min(tm["device"]), 3),
                           "max": round(1e3 * max(tm["device"]), 3)},
        "kernels_ms": {name: {"median": round(1e3 * med[name], 3), "min": round(1e3 * min(tm[name]), 3),
                              "max": round(1e3 * max(tm[name]), 3)} for name in ("rng", "share_kernels", "sum_kernels")},
        "host_loop_over_device_path": round(t_host / med["device"], 2),
        "host_loop_over_kernels": round(t_host / (med["rng"] + med["share_kernels"] + med["sum_kernels"]), 1),
        "us_per_generator": {"host_loop": round(1e6 * t_host / (S * G), 3), "device_path": round(1e6 * med["device"] / (S * G), 3)},
    }
    print(json.dumps(result, indent=1), flush=True)
    out_dir = Path(args.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / f"generators_probe{'_quick' if args.quick else ''}.json").write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
