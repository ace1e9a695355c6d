"""The sharing step of a key-generation round (`_generate_pq`) on the device against the host loop
it replaces, on the device and the box in use.

    python tools/share_probe.py [--out DIR] [--quick] [--reps 5]

For 65 536 candidates at key_length 2048 with n = 5, t = 2 and for 4096 candidates at key_length 1024 with n = 3, t = 1
(the Shamir primes are those of tests/golden/reconstruct.json), single process:

  kernels      events around the launches: the two candidate kernels, the three sharing kernels on rows drawn beforehand,
               and the five launches of the generator
  tensor call  shamir.generate_pq_t, waited for: what a caller who stays on the device gets
  int call     shamir.generate_pq_batch: ints out, as the patched `_generate_pq` uses it
  host loop    per candidate, in plain Python: two candidates from secrets.randbits (DK:874-875) and three sharings with
               secrets.randbelow(P) coefficients evaluated by Horner's rule at 1 .. n — the arithmetic of the un-vendored
               ``share_secret`` without its objects and dictionaries (one run: it takes seconds)

A sample of the int call's output is checked against tools/share_model.py.  Writes DIR/r08_share_probe.txt.
"""

from __future__ import annotations

import argparse
import json
import secrets
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def host_loop(count, prime_length, prime, n, t, first):
    """What the reference does per candidate, without its containers."""
    points = range(1, n + 1)

    def share(secret, degree):
        coeffs = [secrets.randbelow(prime) for _ in range(degree)]
        out = []
        for x in points:
            acc = 0
            for a in reversed(coeffs):
                acc = (acc + a) * x % prime
            out.append((acc + secret) % prime)
        return out

    mod4 = 3 if first else 0
    top = 1 << (prime_length - 1)
    rows = []
    for _ in range(count):
        p = top + (secrets.randbits(prime_length - 3) << 2) + mod4
        q = top + (secrets.randbits(prime_length - 3) << 2) + mod4
        rows.append((p, q, share(p, t), share(q, t), share(0, 2 * t)))
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles", help="directory of the result file (default: profiles/)")
    ap.add_argument("--quick", action="store_true", help="an eighth of the candidates (a smoke run of the probe itself)")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch

    import share_model
    from protocols.distributed_keygen_amd import DeviceRng, Engine, limbs, shamir

    eng = Engine(0)
    fixtures = json.loads((ROOT / "tests" / "golden" / "reconstruct.json").read_text())
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    def fmt(v):
        return f"{1e3 * statistics.median(v):.3f} [{1e3 * min(v):.3f}, {1e3 * max(v):.3f}]"

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

    seed = bytes(range(32))
    emit(f"sharing step of a keygen round: device against the host loop; {args.reps} runs, ms, median [min, max]; host loop: one run")
    for label, count in (("k2048_n5_t2", 65536), ("k1024_n3_t1", 4096)):
        case = fixtures[label]
        prime, n, t, length = int(case["prime"], 16), case["n_parties"], case["t"], case["key_length"] // 2
        if args.quick:
            count //= 8
        lw, bits, cw = limbs.limbs_for(prime), shamir.coefficient_bits(prime), (shamir.coefficient_bits(prime) + 31) // 32
        points = list(range(1, n + 1))
        rng = DeviceRng(key=seed)
        shamir.generate_pq_batch(1, length, prime, n, t, min(count, 256), rng, engine=eng)       # first launches, workspaces
        tm = {k: [] for k in ("rng", "candidates", "share", "tensor", "int")}
        for _ in range(args.reps):
            dt, rows = event_s(lambda: [rng.rows_t(eng, count, length - 3), rng.rows_t(eng, count, length - 3),
                                        rng.rows_t(eng, t * count, bits, cw).view(t, count, cw),
                                        rng.rows_t(eng, t * count, bits, cw).view(t, count, cw),
                                        rng.rows_t(eng, 2 * t * count, bits, cw).view(2 * t, count, cw)])
            tm["rng"].append(dt)
            dt, pq = event_s(lambda: [eng.prime_candidates_t(count, length, True, random_t=r, row_words=lw) for r in rows[:2]])
            tm["candidates"].append(dt)
            tm["share"].append(event_s(lambda: [eng.shamir_share_t(pq[0], prime, t, points, draws_t=rows[2]),
                                                eng.shamir_share_t(pq[1], prime, t, points, draws_t=rows[3]),
                                                eng.shamir_share_t(None, prime, 2 * t, points, batch=count, draws_t=rows[4])])[0])
            del rows, pq
            tm["tensor"].append(wall(lambda: shamir.generate_pq_t(1, length, prime, n, t, count, rng, engine=eng))[0])
            call = rng.next_call
            dt, got = wall(lambda: shamir.generate_pq_batch(1, length, prime, n, t, count, rng, engine=eng))
            tm["int"].append(dt)
        want = share_model.generate_pq(seed, call, 1, length, prime, n, t, 2)       # the first rows of a call do not depend on its count ...
        assert got[0][:2] == want[0] and got[1][:2] == want[1], label                # ... for the candidates: one row each
        assert all(len(got[2][name][j]) == count for name in got[2] for j in points)
        t0 = time.perf_counter()
        host = host_loop(count, length, prime, n, t, True)
        t_host = time.perf_counter() - t0
        assert len(host) == count
        med = {k: statistics.median(v) for k, v in tm.items()}
        products = count * (4 * t + 4 * t * n + 3 * n)
        emit(f"  key_length {case['key_length']} (Shamir prime of {prime.bit_length()} bits), n = {n}, t = {t}, {count} candidates:")
        emit(f"    kernels: generator (5 launches) {fmt(tm['rng'])} | candidates (2) {fmt(tm['candidates'])} | sharing (3) {fmt(tm['share'])}"
             f"   = {1e9 * med['share'] / products:.1f} ns per field product ({products} products)")
        emit(f"    tensor-level generate_pq_t      {fmt(tm['tensor'])}   = {1e6 * med['tensor'] / count:.3f} us per candidate")
        emit(f"    int-level generate_pq_batch     {fmt(tm['int'])}   = {1e6 * med['int'] / count:.3f} us per candidate")
        emit(f"    host loop (plain Python)        {1e3 * t_host:.3f}   = {1e6 * t_host / count:.3f} us per candidate")
        emit(f"    host loop / int-level = {t_host / med['int']:.2f}x | host loop / tensor-level = {t_host / med['tensor']:.1f}x"
             f" | int-level beats the host loop: {'yes' if med['int'] < t_host else 'NO'}")
    out_dir = Path(args.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / f"r08_share_probe{'_quick' if args.quick else ''}.txt").write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
