"""Private-key (CRT) encryption against the existing encryption route on the same build.

    python tools/private_encrypt_probe.py [--out DIR] [--quick] [--key-lengths 2048,4096] [--batches 1,1000,10000,40000]

Per key length and batch, alternating in one process, at least 5 runs of each form after two warm-up rounds:

  crt_r         Engine.private_encrypt_t with the caller's r as shipped (prime split, modexps modulo p and q, modexps
                modulo p^2 and q^2, lift)
  crt_r_seq     ... the two chains one after the other on the caller's stream
  crt_fresh     Engine.private_encrypt_t with a DeviceRng (the draw, the split, modexps modulo p^2 and q^2, lift)
  crt_fresh_seq ... one after the other
  reference     the route of Engine.encrypt_batch: powmod_nsquare_t(r, N, N) and mulmod_t by rows of 1 + m N that are
                ALREADY on the device (in the yardstick's favour) — the yardstick
  fast          FastRandomizer's fixed-base route (slots.encrypt_t's: table of h_s, short exponents from its device
                generator) — another scheme's randomiser, beside the others for orientation only

timed on the device (events around the whole call, device rows to device rows), then the int-level forms
(Engine.private_encrypt_batch in both modes, Engine.encrypt_batch, FastRandomizer.encrypt) by the host clock, ints to
ints.  The prime split, the modexps modulo the primes, those modulo the squares and the lift are timed alone;
``share_of_crt_r`` is each part's time over the median of crt_r, in which the two chains overlap, so the shares of one row
add up to about 1.9 — over crt_r_seq they add up to 1.  The ciphertexts of crt_r, crt_r_seq and reference are compared
bit for bit; those of the fresh forms are decrypted.
Writes DIR/private_encrypt_probe.json; the condition of the issue (median of each CRT mode below the minimum of
reference at key_length 2048, batches 1 and 10 000, on the device and ints to ints) is evaluated into it.
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
    ap.add_argument("--quick", action="store_true", help="key_length 1024, batches 1 and 200: a smoke run of the probe itself")
    ap.add_argument("--key-lengths", default="2048,4096")
    ap.add_argument("--batches", default="1,1000,10000,40000")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch

    from protocols.distributed_keygen_amd import DeviceRng, Engine, configure_hw_queues, limbs, synthetic
    from protocols.distributed_keygen_amd.randomizer import FastRandomizer, generate_base

    configure_hw_queues(16)
    eng = Engine(0)
    key_lengths = [1024] if args.quick else [int(x) for x in args.key_lengths.split(",")]
    batches = [1, 200] if args.quick else [int(x) for x in args.batches.split(",")]
    runs = max(5, args.runs)
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
        for _ in range(2):
            for k, fn in forms.items():
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for k, fn in forms.items():
                ms, outs[k] = timer(fn)
                times[k].append(ms)
        return times, outs

    result = {"device": torch.cuda.get_device_name(0), "cases": []}
    for kl in key_lengths:
        key = synthetic.make_key(kl, 3, 1)
        p, q, n, n2 = key.p, key.q, key.n, key.n_square
        ln, l2 = limbs.limbs_for(n), limbs.limbs_for(n2)
        host = random.Random(kl)
        pool_m = [host.randrange(n) for _ in range(max(batches))]
        pool_r = [host.randrange(1, n) for _ in range(max(batches))]
        dev_rng = DeviceRng()
        fr = FastRandomizer(n, generate_base(n, rng=random.Random(1), engine=eng), engine=eng, device_rng=True)
        table = eng.fixed_base_table(n, fr.h_s, fr.exp_bits, fr.window)
        for batch in batches:
            msgs, rs = pool_m[:batch], pool_r[:batch]
            m_t, r_t = eng.to_device(limbs.pack(msgs, ln)), eng.to_device(limbs.pack(rs, ln))
            r2_t = eng.to_device(limbs.pack(rs, l2))
            gm_t = eng.to_device(limbs.pack([(1 + m * n) % n2 for m in msgs], l2))
            reps = runs if batch >= 10000 else runs + 4
            forms = {
                "crt_r": lambda: eng.private_encrypt_t(m_t, p, q, randomness_t=r_t)[0],
                "crt_r_seq": lambda: eng.private_encrypt_t(m_t, p, q, randomness_t=r_t, side_by_side=False)[0],
                "crt_fresh": lambda: eng.private_encrypt_t(m_t, p, q, rng=dev_rng)[0],
                "crt_fresh_seq": lambda: eng.private_encrypt_t(m_t, p, q, rng=dev_rng, side_by_side=False)[0],
                "reference": lambda: eng.mulmod_t(eng.powmod_nsquare_t(r2_t, n, n), gm_t, n2),
                "fast": lambda: eng.fixed_base_encrypt_t(table, eng.fixed_base_exponent_rows(fr._exponents(None, batch), fr.exp_bits), m_t),
            }
            dev, outs = alternate(forms, device_ms, reps)
            same = torch.equal(outs["reference"], outs["crt_r"]) and torch.equal(outs["reference"], outs["crt_r_seq"])
            for k in ("crt_fresh", "crt_fresh_seq"):
                dec_t, st_t = eng.private_decrypt_t(outs[k], p, q)
                same = same and torch.equal(dec_t, m_t) and not bool(st_t.any())
            mod_t = eng.crt_prime_split_t(r_t, p, q)
            e_p, e_q = q % (p - 1), p % (q - 1)
            sp_t, sq_t = eng.powmod_shared_t(mod_t[0], p, e_p), eng.powmod_shared_t(mod_t[1], q, e_q)
            rp_t, rq_t = eng.powmod_nsquare_t(sp_t, p, p), eng.powmod_nsquare_t(sq_t, q, q)
            parts, _ = alternate({"prime_split": lambda: eng.crt_prime_split_t(r_t, p, q),
                                  "modexp_mod_p": lambda: eng.powmod_shared_t(mod_t[0], p, e_p),
                                  "modexp_mod_q": lambda: eng.powmod_shared_t(mod_t[1], q, e_q),
                                  "modexp_mod_p2": lambda: eng.powmod_nsquare_t(sp_t, p, p),
                                  "modexp_mod_q2": lambda: eng.powmod_nsquare_t(sq_t, q, q),
                                  "lift": lambda: eng.crt_lift_t(rp_t, rq_t, p, q, messages_t=m_t)[0]}, device_ms, reps)
            wall, wouts = alternate({"crt_r": lambda: eng.private_encrypt_batch(msgs, p, q, randomness=rs)[0],
                                     "crt_fresh": lambda: eng.private_encrypt_batch(msgs, p, q, rng=dev_rng)[0],
                                     "reference": lambda: eng.encrypt_batch(msgs, rs, n),
                                     "fast": lambda: fr.encrypt(msgs)}, wall_ms, runs)
            same = same and wouts["crt_r"] == wouts["reference"]
            med = {k: statistics.median(v) for k, v in dev.items()}
            wmed = {k: statistics.median(v) for k, v in wall.items()}
            case = {
                "key_length": kl, "batch": batch, "identical_ciphertexts_and_fresh_ones_decrypt": bool(same),
                "device_ms": {k: mmm(v) for k, v in dev.items()},
                "parts_device_ms": {k: mmm(v) for k, v in parts.items()},
                "ints_to_ints_wall_ms": {k: mmm(v) for k, v in wall.items()},
                "ratio_reference_over_crt_r_device": mmm([a / b for a, b in zip(dev["reference"], dev["crt_r"])]),
                "ratio_reference_over_crt_fresh_device": mmm([a / b for a, b in zip(dev["reference"], dev["crt_fresh"])]),
                "ratio_reference_over_crt_r_wall": mmm([a / b for a, b in zip(wall["reference"], wall["crt_r"])]),
                "ratio_reference_over_crt_fresh_wall": mmm([a / b for a, b in zip(wall["reference"], wall["crt_fresh"])]),
                "ratio_seq_over_side": {"crt_r": mmm([a / b for a, b in zip(dev["crt_r_seq"], dev["crt_r"])]),
                                        "crt_fresh": mmm([a / b for a, b in zip(dev["crt_fresh_seq"], dev["crt_fresh"])])},
                "share_of_crt_r": {k: round(statistics.median(v) / med["crt_r"], 4) for k, v in parts.items()},
                "crt_median_below_reference_min": {
                    "crt_r": {"device": med["crt_r"] < min(dev["reference"]), "wall": wmed["crt_r"] < min(wall["reference"])},
                    "crt_fresh": {"device": med["crt_fresh"] < min(dev["reference"]), "wall": wmed["crt_fresh"] < min(wall["reference"])}},
            }
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
    cond = [c for c in result["cases"] if c["key_length"] == 2048 and c["batch"] in (1, 10000)]
    result["condition_key_length_2048_batches_1_and_10000"] = {
        mode: all(c["crt_median_below_reference_min"][mode][k] for c in cond for k in ("device", "wall")) if cond else None
        for mode in ("crt_r", "crt_fresh")}
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / f"private_encrypt_probe{'_quick' if args.quick else ''}.json").write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
