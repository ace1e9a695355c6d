"""Private-key (CRT) decryption against the lambda route on the same build.

    python tools/private_decrypt_probe.py [--out DIR] [--quick] [--key-lengths 2048,4096] [--batches 1,1000,10000,40000]

Per key length and batch, alternating in one process, at least 5 runs of each form after two warm-up rounds:

  crt           Engine.private_decrypt_t as shipped
  crt_seq       the two half-size modexps one after the other on the caller's stream
  crt_side      the modexp modulo q^2 on the companion stream beside the one modulo p^2
  lambda        the threshold path misused: powmod_nsquare_t(c, N, lambda) and combine_t with theta_inv = lambda^-1 mod N

timed on the device (events around the whole call, device rows to device rows), then the int-level forms
(Engine.private_decrypt_batch against powmod_nsquare_batch + combine_batch) by the host clock, ints to ints.  The split
and the recombination kernels are timed alone for their share.  A CRT decryption on ONE host core — gmpy2 if it imports,
else Python's pow — is timed on a sample as the host yardstick.  The plaintext rows of every form are compared bit for
bit.  Writes DIR/private_decrypt_probe.json; the condition of the issue (median of crt below the minimum of lambda at
key_length 2048, batches 1 and 10 000) is evaluated into it.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def mmm(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def host_crt(cts, p, q):
    """(seconds per ciphertext on one core, backend): the formulas of private_key.py with the host's modexp."""
    try:
        import gmpy2

        powmod, backend = (lambda b, e, m: int(gmpy2.powmod(b, e, m))), "gmpy2"
    except ImportError:
        powmod, backend = pow, "python pow"
    from protocols.distributed_keygen_amd.private_key import crt_constants

    h_p, h_q, p_inv = crt_constants(p, q)
    p2, q2 = p * p, q * q
    t0 = time.perf_counter()
    out = []
    for c in cts:
        m_p = (powmod(c % p2, p - 1, p2) - 1) // p * h_p % p
        m_q = (powmod(c % q2, q - 1, q2) - 1) // q * h_q % q
        out.append(m_p + p * ((m_q - m_p) * p_inv % q))
    return (time.perf_counter() - t0) / len(cts), backend, out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--quick", action="store_true", help="key_length 1024, batches 1 and 200: a smoke run of the probe itself")
    ap.add_argument("--key-lengths", default="2048,4096")
    ap.add_argument("--batches", default="1,1000,10000,40000")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch

    from protocols.distributed_keygen_amd import Engine, configure_hw_queues, limbs, synthetic

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
        lam = (p - 1) * (q - 1)
        lam_inv = pow(lam, -1, n)
        l2 = limbs.limbs_for(n2)
        pool = synthetic.random_ciphertexts(key, max(batches), seed=11)
        per_core, backend, host_out = host_crt(pool[: 16 if kl > 2048 else 48], p, q)
        for batch in batches:
            cts = pool[:batch]
            cts_t = eng.to_device(limbs.pack(cts, l2))
            reps = runs if batch >= 10000 else runs + 4
            forms = {
                "crt": lambda: eng.private_decrypt_t(cts_t, p, q)[0],
                "crt_seq": lambda: eng.private_decrypt_t(cts_t, p, q, side_by_side=False)[0],
                "crt_side": lambda: eng.private_decrypt_t(cts_t, p, q, side_by_side=True)[0],
                "lambda": lambda: eng.combine_t(eng.powmod_nsquare_t(cts_t, n, lam).unsqueeze(0), n, lam_inv)[0],
            }
            dev, outs = alternate(forms, device_ms, reps)
            same = all(torch.equal(outs["lambda"], outs[k]) for k in ("crt", "crt_seq", "crt_side"))
            if batch >= len(host_out):
                same = same and limbs.unpack(eng.to_host(outs["crt"][: len(host_out)])) == host_out
            half_t = eng.crt_split_t(cts_t, p, q)
            xp_t, xq_t = eng.powmod_nsquare_t(half_t[0], p, p - 1), eng.powmod_nsquare_t(half_t[1], q, q - 1)
            parts, _ = alternate({"split": lambda: eng.crt_split_t(cts_t, p, q),
                                  "recombine": lambda: eng.crt_recombine_t(xp_t, xq_t, p, q)[0],
                                  "modexp_p": lambda: eng.powmod_nsquare_t(half_t[0], p, p - 1),
                                  "modexp_q": lambda: eng.powmod_nsquare_t(half_t[1], q, q - 1)}, device_ms, reps)

            def lambda_ints():
                partial = eng.powmod_nsquare_batch(cts, lam, n)
                return eng.combine_batch([[x] for x in partial], n, lam_inv)[0]

            wall, wouts = alternate({"crt": lambda: eng.private_decrypt_batch(cts, p, q)[0], "lambda": lambda_ints}, wall_ms, runs)
            same = same and wouts["crt"] == wouts["lambda"]
            med = {k: statistics.median(v) for k, v in dev.items()}
            case = {
                "key_length": kl, "batch": batch, "identical_plaintexts": bool(same),
                "device_ms": {k: mmm(v) for k, v in dev.items()},
                "parts_device_ms": {k: mmm(v) for k, v in parts.items()},
                "ints_to_ints_wall_ms": {k: mmm(v) for k, v in wall.items()},
                "ratio_lambda_over_crt_device": mmm([a / b for a, b in zip(dev["lambda"], dev["crt"])]),
                "ratio_lambda_over_crt_wall": mmm([a / b for a, b in zip(wall["lambda"], wall["crt"])]),
                "ratio_seq_over_side": mmm([a / b for a, b in zip(dev["crt_seq"], dev["crt_side"])]),
                "split_share_of_crt": round(statistics.median(parts["split"]) / med["crt"], 4),
                "recombine_share_of_crt": round(statistics.median(parts["recombine"]) / med["crt"], 4),
                "crt_median_below_lambda_min": {"device": med["crt"] < min(dev["lambda"]),
                                                "wall": statistics.median(wall["crt"]) < min(wall["lambda"])},
                "host_crt_one_core": {"backend": backend, "ms_per_ciphertext": round(1e3 * per_core, 4),
                                      "batch_on_one_core_ms_extrapolated": round(1e3 * per_core * batch, 2)},
            }
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
    cond = [c for c in result["cases"] if c["key_length"] == 2048 and c["batch"] in (1, 10000)]
    result["condition_key_length_2048_batches_1_and_10000"] = bool(cond) and all(
        c["crt_median_below_lambda_min"]["device"] and c["crt_median_below_lambda_min"]["wall"] for c in cond) if cond else None
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / f"private_decrypt_probe{'_quick' if args.quick else ''}.json").write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
