"""Homomorphic linear maps at key_length 2048: the multi-exponentiation kernel against the same results
through the public API that existed before it, and against libgmp on the host cores.

    python tools/homomorphic_probe.py [--out DIR] [--quick]

Cases: 10 000 ciphertexts x signed 64-bit scalars; the same with scalars below N; a dense 1024 x 1024 map with signed
64-bit weights and a bias; one sum of 10^6 ciphertexts; 1000 sums of 1000; and the scaling case with ALL-EQUAL scalars
next to powmod_nsquare_t (the price of per-element exponents).  Every GPU result is checked against the composed path.

Baselines:
  * composed: powmod_multi_t modulo N^2 with one group per term (negative weights: modinv_t first), then a mulmod_t
    product tree per output — the public API without mx_multiexp_nsquare_run;
  * host: libgmp's mpz_powm (the routine gmpy2.powmod calls; tests/hostpow.py) on PROCS worker processes, products with
    CPython ints.
Where a baseline would take minutes it is measured on a slice of the case and scaled by the ratio of terms (stated in
the output).  Times are device-resident (rows already on the GPU, one synchronize at the end), median of 3.
"""

from __future__ import annotations

import argparse
import os
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

PROCS = 16


def timed(fn, reps=3, warmup=1):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles", help="directory of the result file (default: profiles/)")
    ap.add_argument("--quick", action="store_true", help="smaller cases (a smoke run of the probe itself)")
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, configure_hw_queues, limbs, synthetic

    configure_hw_queues(16)
    import hostpow
    import torch

    pool = __import__("multiprocessing").get_context("fork").Pool(PROCS)      # before the GPU is touched
    eng = Engine(0)
    key = synthetic.make_key(2048, 3, 1)
    n, n2 = key.n, key.n_square
    l2 = limbs.limbs_for(n2)
    rng = random.Random(2048)
    q = args.quick
    lines = [f"key_length 2048 (N {n.bit_length()} bits), host baseline: libgmp mpz_powm on {PROCS} processes "
             f"({hostpow.engine_name()}), box reports {os.cpu_count()} CPUs; sums (all weights 1) on the host are "
             "plain products on ONE core, in the composed path a mulmod_t product tree without powmod_multi_t"]

    def dev(vals):
        return eng.to_device(limbs.pack_reduced(vals, l2, n2))

    def composed(x_t, rows):
        """Public API without the multiexp kernel: one powmod_multi_t group per term, product tree per output."""
        terms = [(i, w) for row in rows for i, w in row.items()]
        if all(w == 1 for _, w in terms):
            pw = x_t[torch.tensor([i for i, _ in terms], device=eng.device)].contiguous()
            return tree(pw, rows)
        neg = sorted({i for i, w in terms if w < 0})
        inv_t = eng.modinv_t(x_t[neg].contiguous(), n2) if neg else None
        pos = {i: k for k, i in enumerate(neg)}
        idx = torch.tensor([i for i, w in terms], device=eng.device)
        bases = x_t[idx]
        if neg:
            sel = [k for k, (i, w) in enumerate(terms) if w < 0]
            bases[sel] = inv_t[torch.tensor([pos[terms[k][0]] for k in sel], device=eng.device)]
        pw = eng.powmod_multi_t(bases.contiguous(), [n2] * len(terms), [abs(w) for _, w in terms], 1)
        return tree(pw, rows)

    def tree(pw, rows):
        # product tree per output: rows of equal length here (every case), pairwise levels
        k = len(rows[0])
        cur = pw.view(len(rows), k, l2)
        while cur.shape[1] > 1:
            m = cur.shape[1]
            a = cur[:, 0 : m - (m & 1) : 2].reshape(-1, l2).contiguous()
            b = cur[:, 1:m:2].reshape(-1, l2).contiguous()
            prod = eng.mulmod_t(a, b, n2).view(len(rows), m // 2, l2)
            cur = torch.cat([prod, cur[:, m - 1 : m]], dim=1) if m & 1 else prod
        return cur.reshape(len(rows), l2)

    def host(vals, rows):
        t0 = time.perf_counter()
        if all(w == 1 for row in rows for w in row.values()):
            pw = [vals[i] for row in rows for i in row]
        else:
            jobs = [((vals[i] if w >= 0 else pow(vals[i], -1, n2)), abs(w), n2) for row in rows for i, w in row.items()]
            pw = hostpow.powmod_many(jobs, pool=pool)
        out, pos = [], 0
        for row in rows:
            acc = 1
            for v in pw[pos : pos + len(row)]:
                acc = acc * v % n2
            out.append(acc)
            pos += len(row)
        return time.perf_counter() - t0, out

    def kernel_ms(fn):
        """Sum of the multi-exponentiation kernels' durations in one call (mx_profile events around every run)."""
        eng.profile_collect()
        eng.profile(True)
        fn()
        eng.profile(False)
        ms, launches = eng.profile_collect()
        return ms, launches

    def case(name, vals, rows, bias=None, comp_rows=None, host_rows=None):
        x_t = dev(vals)
        t_gpu, y_t = timed(lambda: eng.multiexp_nsquare_t(x_t, rows, n, bias=bias))
        k_ms, k_n = kernel_ms(lambda: eng.multiexp_nsquare_t(x_t, rows, n, bias=bias))
        y = limbs.unpack(eng.to_host(y_t))
        terms = sum(len(r) for r in rows)
        rows = [r if isinstance(r, dict) else dict(enumerate(r)) for r in rows]       # (the baselines take {input: weight})
        cr = rows if comp_rows is None else rows[:comp_rows]
        t_c, c_t = timed(lambda: composed(x_t, cr), reps=1)
        c = limbs.unpack(eng.to_host(c_t))
        if bias is not None:
            c = [(1 + (b % n) * n) * v % n2 for v, b in zip(c, bias)]
        assert c == y[: len(cr)], name
        scale_c = terms / sum(len(r) for r in cr)
        hr = rows if host_rows is None else rows[:host_rows]
        t_h, h = host(vals, hr)
        if bias is not None:
            h = [(1 + (b % n) * n) * v % n2 for v, b in zip(h, bias)]
        assert h == y[: len(hr)], name
        scale_h = terms / sum(len(r) for r in hr)
        line = (f"{name}: {len(rows)} outputs, {terms} terms | multiexp {1e3 * t_gpu:.1f} ms (kernels {k_ms:.1f} ms in {k_n} runs,"
                f" the rest host planning and uploads) | composed {1e3 * t_c * scale_c:.1f} ms"
                f"{'' if scale_c == 1 else f' (x{scale_c:.0f} of {len(cr)} rows)'} = {t_c * scale_c / t_gpu:.2f}x"
                f" | libgmp {PROCS} procs {1e3 * t_h * scale_h:.1f} ms{'' if scale_h == 1 else f' (x{scale_h:.0f} of {len(hr)} rows)'}"
                f" = {t_h * scale_h / t_gpu:.2f}x")
        print(line, flush=True)
        lines.append(line)
        return t_gpu

    m = 1000 if q else 10000
    cts = synthetic.random_ciphertexts(key, m, seed=1)
    s64 = [rng.randrange(-(1 << 63), 1 << 63) for _ in range(m)]
    case("scale_s64", cts, [{k: s} for k, s in enumerate(s64)], host_rows=m // 10)
    sn = [rng.randrange(n) for _ in range(m)]
    case("scale_ltN", cts, [{k: s} for k, s in enumerate(sn)], host_rows=m // 20)
    # all-equal scalars next to the one-exponent kernel
    e = rng.getrandbits(64)
    x_t = dev(cts)
    t_eq, y_t = timed(lambda: eng.multiexp_nsquare_t(x_t, [{k: e} for k in range(m)], n))
    t_pw, p_t = timed(lambda: eng.powmod_nsquare_t(x_t, n, e))
    assert torch.equal(y_t, p_t)
    k_eq, _ = kernel_ms(lambda: eng.multiexp_nsquare_t(x_t, [{k: e} for k in range(m)], n))
    k_pw, _ = kernel_ms(lambda: eng.powmod_nsquare_t(x_t, n, e))
    line = (f"scale_equal_s64: {m} x one 64-bit scalar | multiexp {1e3 * t_eq:.1f} ms (kernels {k_eq:.1f} ms) | powmod_nsquare_t "
            f"{1e3 * t_pw:.1f} ms (kernel {k_pw:.1f} ms) = {t_eq / t_pw:.2f}x the time, {k_eq / max(k_pw, 1e-9):.2f}x the kernel time")
    print(line, flush=True)
    lines.append(line)
    d = 128 if q else 1024
    vec = synthetic.random_ciphertexts(key, d, seed=2)
    W = [[rng.randrange(-(1 << 63), 1 << 63) for i in range(d)] for _ in range(d)]        # dense rows
    bias = [rng.randrange(n) for _ in range(d)]
    case(f"dense_{d}x{d}_s64_bias", vec, W, bias=bias, comp_rows=max(1, d // 16), host_rows=max(1, d // 64))
    big = 100_000 if q else 1_000_000
    vals = synthetic.random_ciphertexts(key, big, seed=3)
    case("sum_1e6" if not q else "sum_1e5", vals, [{i: 1 for i in range(big)}], host_rows=1)
    g = 100 if q else 1000
    case(f"sums_{g}x{g}", vals[: g * g], [{j * g + i: 1 for i in range(g)} for j in range(g)], host_rows=g // 10)
    pool.close()
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / f"r07_homomorphic_probe{'_quick' if q else ''}.txt").write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
