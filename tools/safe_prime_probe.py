"""Safe-prime search on the device: the joint sieve against the two-call route, the stages, whole searches and whole keys
(DESIGN.md §4.24).

    python tools/safe_prime_probe.py [--out DIR] [--quick] [--runs 5]

One process; forms alternate after a warm-up call each; min / median / max over the repeats.

  sieve A/B           on ONE drawn batch of halves h at 1024 and at 2048 bits, device events:
                        joint      Engine.safe_sieve_t(h)
                        two_call   the route without the joint kernel: sieve_t(h), the rows 2h + 1 (safe_double_t), sieve_t on
                                   those, the flags ORed — the two must agree row for row
  stages              at 1024 bits on that batch: joint sieve, base 2 on h, doubling + base 2 on p, 64 random rounds on h
                      (on the rows the base 2 on h left, so that the launch has rows to time), with the survivor counts
  search              wall clock of Engine.safe_prime_search_t(1, 1024) with the sieve list bound at 2^14 and at 2^16
  keys                wall clock of PaillierPrivateKey.generate(kl, safe=True) at key_length 2048 and 3072, ints back
  host                the pure-Python search for ONE 1024-bit safe prime on one core with the same sieve and pow
                      (tools/mr_model.py); a gmpy2 search if gmpy2 imports

Writes DIR/safe_prime_probe.json.
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


def mmm(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--quick", action="store_true", help="256 / 512 bits, key_length 512: a smoke run of the probe itself")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch

    import mr_model
    from protocols.distributed_keygen_amd import DeviceRng, Engine, PaillierPrivateKey, configure_hw_queues, primes

    configure_hw_queues(16)
    eng = Engine(0)
    runs = max(2, args.runs)
    widths = (256, 512) if args.quick else (1024, 2048)
    key_lengths = (512,) if args.quick else (2048, 3072)
    cur = lambda: torch.cuda.current_stream(eng.device)      # noqa: E731

    def device_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(cur())
        out = fn()
        b.record(cur())
        b.synchronize()
        return a.elapsed_time(b), out

    def wall_ms(fn):
        t0 = time.perf_counter()
        out = fn()
        eng.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def alternate(forms, timer, reps):
        times = {k: [] for k in forms}
        outs = {}
        for k, fn in forms.items():
            fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for k, fn in forms.items():
                ms, outs[k] = timer(fn)
                times[k].append(ms)
        return times, outs

    rng = DeviceRng()
    result = {"device": torch.cuda.get_device_name(0), "sieve_bound": primes.SIEVE_BOUND, "rounds": 64, "sieve_ab": {}}

    def halves(bits):
        rows_t = rng.rows_t(eng, primes.default_safe_batch(1, bits), bits - 1, (bits + 31) // 32)
        for b in (bits - 2, bits - 3, 0):
            rows_t[:, b >> 5] |= (1 << (b & 31)) - ((1 << 32) if (b & 31) == 31 else 0)
        return rows_t

    # ---- the joint sieve against the two-call route
    plist = primes.sieve_primes()
    for bits in widths:
        rows_t = halves(bits)
        t, outs = alternate({"joint": lambda: eng.safe_sieve_t(rows_t, plist),
                             "two_call": lambda: eng.sieve_t(rows_t, plist) | eng.sieve_t(eng.safe_double_t(rows_t, _checked=True), plist)},
                            device_ms, runs + 4)
        spread = max(max(v) - min(v) for v in t.values())
        gain = statistics.median(t["two_call"]) - statistics.median(t["joint"])
        result["sieve_ab"][str(bits)] = {"batch": int(rows_t.shape[0]), "device_ms": {k: mmm(v) for k, v in t.items()},
                                         "agree": bool(torch.equal(outs["joint"], outs["two_call"])),
                                         "survivors": int((outs["joint"] == 0).sum()),
                                         "ratio_two_call_over_joint": mmm([a / b for a, b in zip(t["two_call"], t["joint"])]),
                                         "joint_faster_by_more_than_either_spread": bool(gain > spread)}
        print(json.dumps({bits: result["sieve_ab"][str(bits)]}), flush=True)

    # ---- the stages on one batch
    bits = widths[0]
    rows_t = halves(bits)
    left_t = rows_t[eng.safe_sieve_t(rows_t, plist) == 0].contiguous()
    half_t = left_t[eng.miller_rabin_base2_t(left_t, bits - 1) != 0].contiguous()
    full_t = eng.safe_double_t(half_t)
    both_t = half_t[eng.miller_rabin_base2_t(full_t, bits) != 0].contiguous()

    def random_rounds():
        return eng.miller_rabin_t(half_t, eng.generator_shares_t((half_t, bits - 1), 64, rng=rng), 64, bits=bits - 1, _checked=True)

    stages, _ = alternate({"joint_sieve": lambda: eng.safe_sieve_t(rows_t, plist),
                           "base2_on_h": lambda: eng.miller_rabin_base2_t(left_t, bits - 1, _checked=True),
                           "double_and_base2_on_p": lambda: eng.miller_rabin_base2_t(eng.safe_double_t(half_t, _checked=True), bits, _checked=True),
                           "random_rounds_on_h": random_rounds}, device_ms, runs + 4)
    result["stages"] = {"bits": bits, "batch": int(rows_t.shape[0]), "sieve_survivors": int(left_t.shape[0]),
                        "base2_on_h_survivors": int(half_t.shape[0]), "base2_on_p_survivors": int(both_t.shape[0]),
                        "device_ms": {k: mmm(v) for k, v in stages.items()}}
    print(json.dumps(result["stages"]), flush=True)

    # ---- whole searches for one safe prime, the sieve list bound at 2^14 and at 2^16
    result["search_wall_ms"] = {}
    for bound in (1 << 14, 1 << 16):
        primes.SIEVE_BOUND = bound
        primes._ODD_PRIMES.clear()
        eng.safe_prime_search_t(1, bits, rng)
        eng.synchronize()
        t = [wall_ms(lambda: eng.to_host(eng.safe_prime_search_t(1, bits, rng)))[0] for _ in range(4 * runs)]
        result["search_wall_ms"][str(bound)] = dict(mmm(t), mean=round(statistics.mean(t), 4), list_primes=len(primes.sieve_primes()))
    primes.SIEVE_BOUND = 1 << 14
    primes._ODD_PRIMES.clear()
    print(json.dumps(result["search_wall_ms"]), flush=True)

    # ---- whole keys, ints back
    forms = {f"generate_safe_{kl}": (lambda kl=kl: PaillierPrivateKey.generate(kl, rng=rng, engine=eng, safe=True)) for kl in key_lengths}
    wall, outs = alternate(forms, wall_ms, runs)
    result["keys_wall_ms"] = {k: mmm(v) for k, v in wall.items()}
    key = outs[f"generate_safe_{key_lengths[0]}"]
    result["generated_key_round_trips"] = key.decrypt_batch(key.encrypt_batch([0, 1, key.n - 1, 12345])) == [0, 1, key.n - 1, 12345]
    result["generated_key_is_safe"] = key.check_primes(safe=True, engine=eng)
    print(json.dumps(result["keys_wall_ms"]), flush=True)

    # ---- the host: one safe prime of widths[0] bits, same sieve, pow
    host = random.Random(1)
    t0, tried = time.perf_counter(), 0
    while True:
        tried += 1
        h = mr_model.force_half_bits(host.getrandbits(bits - 1), bits)
        if not mr_model.safe_sieve_hit(h) and pow(2, h - 1, h) == 1 and pow(2, 2 * h, 2 * h + 1) == 1 \
                and all(mr_model.round_passes(h, b) for b in (3, 5, 7, 11, 13)):
            break
    result["host_python_one_safe_prime"] = {"bits": bits, "ms": round(1e3 * (time.perf_counter() - t0), 1), "candidates": tried}
    try:
        import gmpy2  # noqa: F401

        result["host_gmpy2"] = "imports; not timed by this probe"
    except ImportError:
        result["host_gmpy2"] = None
    print(json.dumps(result["host_python_one_safe_prime"]), flush=True)
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / f"safe_prime_probe{'_quick' if args.quick else ''}.json").write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
