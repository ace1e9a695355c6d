"""Private-key generation on the device against host prime searches, and the stages of the test alone.

    python tools/prime_probe.py [--out DIR] [--quick] [--runs 5] [--host-primes 1]

Wall clock around calls that end in a synchronise (ints come back), after one warm-up call each:

  generate            PaillierPrivateKey.generate(key_length) at key_length 2048 and 4096
  generate_batch      PaillierPrivateKey.generate_batch(64, 2048): one search for 128 primes
  host_synthetic      synthetic.random_prime (the tree's pure-Python Miller-Rabin loop), per prime of 1024 bits
  host_gmpy2          a gmpy2.is_prime search on one core, per prime, if gmpy2 imports

and, on ONE drawn batch of 1024-bit candidates (the default batch of a 128-prime search), alternating, device events:

  sieve               Engine.sieve_t by the odd primes below primes.SIEVE_BOUND, the whole batch
  base2               Engine.miller_rabin_base2_t on the sieve's survivors: mr_base2_kernel
  base2_via_powmod    the same survivors the way the parent commit could run them: powmod_multi_t on rows holding 2
                      with the exponents of mr_split_t, then the witness loop (Engine.miller_rabin_t)
  random_rounds       64 random bases (the draw included) on what the base 2 left

The two base-2 routes must agree row for row.  Writes DIR/prime_probe.json.
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


def mmm(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--quick", action="store_true", help="key_length 512, 4 keys per batch: a smoke run of the probe itself")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-primes", type=int, default=1, help="primes the host baselines search per run")
    args = ap.parse_args()
    import torch

    from protocols.distributed_keygen_amd import DeviceRng, Engine, PaillierPrivateKey, configure_hw_queues, primes, synthetic

    configure_hw_queues(16)
    eng = Engine(0)
    runs = max(2 if args.quick else 5, args.runs)
    key_lengths = [512] if args.quick else [2048, 4096]
    batch_keys, batch_kl = (4, 512) if args.quick else (64, 2048)
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
    result = {"device": torch.cuda.get_device_name(0), "sieve_bound": primes.SIEVE_BOUND, "rounds": 64}

    # ---- whole keys
    forms = {f"generate_{kl}": (lambda kl=kl: PaillierPrivateKey.generate(kl, rng=rng, engine=eng)) for kl in key_lengths}
    forms[f"generate_batch_{batch_keys}x{batch_kl}"] = lambda: PaillierPrivateKey.generate_batch(batch_keys, batch_kl, rng=rng, engine=eng)
    wall, outs = alternate(forms, wall_ms, runs)
    result["keys_wall_ms"] = {k: mmm(v) for k, v in wall.items()}
    key = outs[f"generate_{key_lengths[0]}"]
    result["generated_key_round_trips"] = key.decrypt_batch(key.encrypt_batch([0, 1, key.n - 1, 12345])) == [0, 1, key.n - 1, 12345]
    result["ms_per_key_in_batch"] = mmm([v / batch_keys for v in wall[f"generate_batch_{batch_keys}x{batch_kl}"]])
    print(json.dumps(result), flush=True)

    # ---- host baselines, per prime of batch_kl / 2 bits
    bits = batch_kl // 2
    host = random.Random(1)
    t = []
    for _ in range(2):
        t0 = time.perf_counter()
        for _ in range(args.host_primes):
            synthetic.random_prime(host, bits)
        t.append(1e3 * (time.perf_counter() - t0) / args.host_primes)
    result["host_synthetic_ms_per_prime"] = mmm(t)
    try:
        import gmpy2

        t = []
        for _ in range(runs):
            t0 = time.perf_counter()
            for _ in range(4 * args.host_primes):
                while True:
                    c = host.getrandbits(bits) | (3 << (bits - 2)) | 1
                    if gmpy2.is_prime(c, 64):
                        break
            t.append(1e3 * (time.perf_counter() - t0) / (4 * args.host_primes))
        result["host_gmpy2_ms_per_prime"] = mmm(t)
    except ImportError:
        result["host_gmpy2_ms_per_prime"] = None

    # ---- the stages on one batch
    batch = primes.default_batch(2 * batch_keys, bits)
    rows_t = rng.rows_t(eng, batch, bits)
    for b in (bits - 1, bits - 2, 0):
        rows_t[:, b >> 5] |= (1 << (b & 31)) - ((1 << 32) if (b & 31) == 31 else 0)
    left_t = rows_t[eng.sieve_t(rows_t, primes.sieve_primes()) == 0].contiguous()
    twos_t = torch.zeros_like(left_t)
    twos_t[:, 0] = 2
    kept_t = left_t[eng.miller_rabin_base2_t(left_t, bits) != 0].contiguous()

    def random_rounds():
        return eng.miller_rabin_t(kept_t, eng.generator_shares_t((kept_t, bits), 64, rng=rng), 64, bits=bits, _checked=True)

    stages, outs = alternate({"sieve": lambda: eng.sieve_t(rows_t, primes.sieve_primes()),
                              "base2": lambda: eng.miller_rabin_base2_t(left_t, bits, _checked=True),
                              "base2_via_powmod": lambda: eng.miller_rabin_t(left_t, twos_t, 1, bits=bits, _checked=True),
                              "random_rounds": random_rounds}, device_ms, runs + 4)
    result["stages"] = {"bits": bits, "batch": batch, "sieve_survivors": int(left_t.shape[0]), "base2_survivors": int(kept_t.shape[0]),
                        "primes": int(outs["random_rounds"].view(-1, 64).min(dim=1).values.sum()),
                        "device_ms": {k: mmm(v) for k, v in stages.items()},
                        "base2_routes_agree": bool(torch.equal(outs["base2"], outs["base2_via_powmod"])),
                        "ratio_via_powmod_over_base2": mmm([a / b for a, b in zip(stages["base2_via_powmod"], stages["base2"])])}
    print(json.dumps(result["stages"]), flush=True)
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / f"prime_probe{'_quick' if args.quick else ''}.json").write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
