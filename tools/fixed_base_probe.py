"""Fixed-base encryption and re-randomisation against the generic route r^N, on the device in use.

    python tools/fixed_base_probe.py [--out DIR] [--quick] [--key-lengths 2048,4096] [--skip sweep,gap,multiexp,ints,pipeline]

1. sweep: kernel time of Engine.fixed_base_encrypt_t for every window 4..8 and the model's choice, against the kernels
   Engine.encrypt_batch launches for the same count (powmod_nsquare_t(r, n, n) and mulmod_t — that function is untouched),
   alternating in one process; median and [min, max] of the repetitions; beside it the prediction from operation counts
   (the plan's real tape for the exponent N, the real number of windows); table build time and bytes per window.
2. gap: event timings that separate the measured ratio from the predicted one (gathers, the generic route's shape).
2b. multiexp: the same h_s^a through what could be composed before: multiexp_nsquare_t over the inputs h_s^(2^(w i)).
3. ints: FastRandomizer.encrypt / .randomize, ints to ints, and the share spent drawing the exponents.
4. pipeline: a dense 1024 x 1024 linear_map with fresh outputs — randomize_batch after it against randomizer=.
Outputs are checked: fixed-base results of every configuration against pow on a sample (all windows must agree bit for
bit on the whole batch), the generic route against pow on a sample.  Writes DIR/r09_fixed_base_probe.txt.
"""

from __future__ import annotations

import argparse
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles", help="directory of the result file (default: profiles/)")
    ap.add_argument("--quick", action="store_true", help="smaller cases (a smoke run of the probe itself)")
    ap.add_argument("--key-lengths", default="2048,4096")
    ap.add_argument("--skip", default="", help="comma-separated sections to skip: sweep,gap,multiexp,ints,pipeline")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch

    from protocols.distributed_keygen_amd import Engine, configure_hw_queues, homomorphic, limbs, randomizer, synthetic

    configure_hw_queues(16)
    eng = Engine(0)
    q = args.quick
    skip = set(filter(None, args.skip.split(",")))
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    def kernel_ms(fn):
        """Kernel time (events around the launches, MxKernelTimer) of one run of fn."""
        eng.profile_collect()
        eng.profile(True)
        out = fn()
        eng.profile(False)
        return eng.profile_collect()[0], out

    def alternating(fns, reps):
        """{name: (median, min, max) kernel ms} with the functions run in turn, reps times, after one warm-up each."""
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        outs = {}
        for _ in range(reps):
            for k, f in fns.items():
                ms, outs[k] = kernel_ms(f)
                ts[k].append(ms)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}, outs

    def fmt(t):
        return f"{t[0]:.3f} [{t[1]:.3f}, {t[2]:.3f}]"

    for kl in [int(x) for x in args.key_lengths.split(",")]:
        key = synthetic.make_key(kl, 3, 1)
        n, n2 = key.n, key.n_square
        ln, l2 = limbs.limbs_for(n), limbs.limbs_for(n2)
        nb = n.bit_length()
        rng = random.Random(kl)
        nprng = np.random.default_rng(kl)
        h_s = randomizer.generate_base(n, rng=rng, engine=eng)
        plan_n = eng.nsquare_plan(n, n)
        generic_products = plan_n.desc.n_sqr + plan_n.desc.n_mul
        emit(f"key_length {kl} (N {nb} bits): r^N tape {plan_n.desc.n_sqr} squarings + {plan_n.desc.n_mul} multiplications"
             f" = {generic_products} pair products, then one product modulo N^2 (mulmod_t)")
        counts = (1000, 10_000) if q else ((1000, 10_000, 100_000, 1_000_000) if kl == 2048 else (1000, 10_000, 100_000))
        top = max(counts)
        # operand pools on the device: uniform words (residues below 2^(32 limbs) are reduced by nobody here: the top word
        # of every row is cleared so that rows are below N resp. N^2 for these moduli of nb resp. 2 nb - 1 or 2 nb bits)
        def rows_below(count, words, bound):
            a = nprng.integers(0, 1 << 32, size=(count, words), dtype=np.uint64).astype(np.uint32)
            spare = 32 * words - (bound.bit_length() - 1)
            full, part = divmod(spare, 32)
            if full:
                a[:, words - full:] = 0
            if part:
                a[:, words - full - 1] &= np.uint32((1 << (32 - part)) - 1)
            return a

        r_t = eng.to_device(rows_below(top, l2, n))          # r < N (as rows of the width of N^2)
        g_t = eng.to_device(rows_below(top, l2, n2))         # stands for 1 + m N in the generic route's mulmod
        m_np = rows_below(top, ln, n)
        m_t = eng.to_device(m_np)

        if "sweep" not in skip:
            for exp_bits in (-(-nb // 2), nb + 64):
                e_np = rows_below(top, (exp_bits + 31) // 32, 1 << exp_bits)
                e_t = eng.to_device(e_np)
                tables = {}
                for w in (4, 5, 6, 7, 8):
                    torch.cuda.synchronize()
                    ms, tab = kernel_ms(lambda: eng.fixed_base_table(n, h_s, exp_bits, w))
                    tables[w] = tab
                    emit(f"  table exp_bits={exp_bits} w={w}: {tab.windows} windows, {tab.nbytes} B ({tab.nbytes / 2**20:.1f} MiB),"
                         f" built in {ms:.2f} ms of kernels ({exp_bits} chain squarings + {tab.windows * ((1 << w) - 2)} entries"
                         f" of {2 * (w - 1)} products)")
                for count in counts:
                    w_model = eng.fixed_base_shape(n, exp_bits, count)[0]
                    reps = args.reps if count <= 100_000 else 3
                    fns = {"generic": lambda: eng.mulmod_t(eng.powmod_nsquare_t(r_t[:count], n, n), g_t[:count], n2)}
                    for w in (4, 5, 6, 7, 8):
                        fns[w] = (lambda tab: lambda: eng.fixed_base_encrypt_t(tab, e_t[:count], m_t[:count]))(tables[w])
                    res, outs = alternating(fns, reps)
                    for w in (5, 6, 7, 8):
                        assert torch.equal(outs[4], outs[w]), (kl, exp_bits, count, w)
                    got = limbs.unpack(eng.to_host(outs[4][:3]))
                    es, ms_ = limbs.unpack(e_np[:3]), limbs.unpack(m_np[:3])
                    assert got == [(1 + m * n) * pow(h_s, e, n2) % n2 for e, m in zip(es, ms_)], (kl, exp_bits, count)
                    gen = limbs.unpack(eng.to_host(outs["generic"][:2]))
                    rs, gs = limbs.unpack(eng.to_host(r_t[:2])), limbs.unpack(eng.to_host(g_t[:2]))
                    assert gen == [pow(r, n, n2) * g % n2 for r, g in zip(rs, gs)]
                    emit(f"  encrypt exp_bits={exp_bits} count={count}: generic r^N + mulmod {fmt(res['generic'])} ms"
                         f" ({reps} alternating runs, median [min, max]); model's window: {w_model}")
                    best = min((4, 5, 6, 7, 8), key=lambda w: res[w][0])
                    for w in (4, 5, 6, 7, 8):
                        products = tables[w].windows - 1 + 3          # one load, windows - 1 products, 2 for 1 + m N, 1 for E
                        emit(f"    w={w}: fixed base {fmt(res[w])} ms = {res['generic'][0] / res[w][0]:.2f}x faster"
                             f" | predicted from {products} against {generic_products + 2} products: {(generic_products + 2) / products:.1f}x"
                             + ("  <- best of the sweep" if w == best else "") + ("  <- model" if w == w_model else ""))
                del tables

        if "gap" not in skip:
            # what separates the measured ratio from the predicted one, from event timings: (a) the table gathers — the
            # same launch with every exponent 0 reads ONE entry per window, from cache; (b) the generic route's shape —
            # r^N forced onto the instance type the fixed-base kernel is built on (9 limbs per lane, one wavefront);
            # (c) squarings against multiplications on that instance: the pack kernel's products are squarings, the
            # fixed-base kernel's are multiplications
            exp_bits = -(-nb // 2)
            count = 10_000 if q else 100_000
            tab = eng.fixed_base_table(n, h_s, exp_bits, 8)
            e_t = eng.to_device(rows_below(count, (exp_bits + 31) // 32, 1 << exp_bits))
            z_t = torch.zeros_like(e_t)
            res, _ = alternating({"random": lambda: eng.fixed_base_power_t(tab, e_t), "zero": lambda: eng.fixed_base_power_t(tab, z_t),
                                  "auto": lambda: eng.powmod_nsquare_t(r_t[:count], n, n),
                                  "narrow": lambda: eng.powmod_nsquare_t(r_t[:count], n, n, segments=1, shape=(9, 1))}, 3)
            shape = eng.nsquare_launch_shape(nb, count)
            emit(f"  gap exp_bits={exp_bits} w=8 count={count}: h_s^a with random exponents {fmt(res['random'])} ms, with all exponents 0"
                 f" (one cached entry per window) {fmt(res['zero'])} ms -> gathers cost {100 * (res['random'][0] / res['zero'][0] - 1):.1f} %")
            per_fixed = 1e6 * res["random"][0] / (count * tab.windows)
            emit(f"  gap r^N alone, count={count}: the library's shape {shape} {fmt(res['auto'])} ms | 9 limbs per lane, one wavefront"
                 f" {fmt(res['narrow'])} ms; ns per output and product: fixed base {per_fixed:.3f} ({tab.windows} multiplications),"
                 f" r^N auto {1e6 * res['auto'][0] / (count * generic_products):.3f}, narrow {1e6 * res['narrow'][0] / (count * generic_products):.3f}"
                 f" ({plan_n.desc.n_sqr} squarings + {plan_n.desc.n_mul} multiplications)")

        if "multiexp" not in skip:
            exp_bits = -(-nb // 2)
            for w, count in ((8, 1000),) if q else ((8, 1000), (8, 10_000), (6, 10_000)):
                tab = eng.fixed_base_table(n, h_s, exp_bits, w)
                exps = [rng.getrandbits(exp_bits) for _ in range(count)]
                e_t = eng.fixed_base_exponent_rows(exps, exp_bits)
                inputs = [h_s]
                for _ in range(tab.windows - 1):
                    inputs.append(pow(inputs[-1], 1 << w, n2))
                in_t = eng.to_device(limbs.pack(inputs, l2))
                mask = (1 << w) - 1
                weights = [{i: (e >> (w * i)) & mask for i in range(tab.windows) if (e >> (w * i)) & mask} for e in exps]
                res, outs = alternating({"fixed": lambda: eng.fixed_base_power_t(tab, e_t),
                                         "multiexp": lambda: eng.multiexp_nsquare_t(in_t, weights, n, window=w)}, 3)
                assert torch.equal(outs["fixed"], outs["multiexp"]), (kl, w, count)
                emit(f"  h_s^a exp_bits={exp_bits} w={w} count={count}: fixed_base_power_t {fmt(res['fixed'])} ms | multiexp_nsquare_t over"
                     f" {tab.windows} inputs {fmt(res['multiexp'])} ms of kernels = {res['multiexp'][0] / res['fixed'][0]:.1f}x; bit-identical")

        if "ints" not in skip:
            fr = randomizer.FastRandomizer(n, h_s, engine=eng)
            count = 10_000 if q else 100_000
            msgs = [rng.randrange(-(1 << 31), 1 << 31) for _ in range(count)]
            fr.encrypt(msgs[:100])
            for name, fn in (("encrypt", lambda: fr.encrypt(msgs)), ("randomize", None)):
                if fn is None:
                    cts = fr.encrypt(msgs)
                    fn = lambda: fr.randomize(cts)                      # noqa: E731
                ts, td = [], []
                for _ in range(3):
                    t0 = time.perf_counter()
                    out = fn()
                    ts.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    eng.fixed_base_exponent_rows(fr.draw(count), fr.exp_bits)
                    torch.cuda.synchronize()
                    td.append(time.perf_counter() - t0)
                assert len(out) == count
                emit(f"  FastRandomizer.{name} ints -> ints, count={count}: {1e3 * statistics.median(ts):.1f} ms, of which drawing"
                     f" and uploading the exponents {1e3 * statistics.median(td):.2f} ms")

        if "pipeline" not in skip and kl == 2048:
            fr = randomizer.FastRandomizer(n, h_s, engine=eng)
            dim = 256 if q else 1024
            x = [rng.randrange(-1000, 1000) for _ in range(dim)]
            W = [[rng.randrange(-128, 128) for _ in range(dim)] for _ in range(dim)]
            cts = fr.encrypt(x)
            ta, tb = [], []
            homomorphic.linear_map(cts, W, n=n, engine=eng)
            for _ in range(3):
                t0 = time.perf_counter()
                y = homomorphic.linear_map(cts, W, n=n, engine=eng)
                ya = eng.randomize_batch(y, [rng.randrange(1, n) for _ in y], n)
                ta.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                yb = homomorphic.linear_map(cts, W, n=n, engine=eng, randomizer=fr)
                tb.append(time.perf_counter() - t0)
            lam = (key.p - 1) * (key.q - 1)
            for u, v, p in list(zip(ya, yb, y))[:3]:                   # the same plaintexts: quotients are N-th residues
                assert pow(u * pow(p, -1, n2) % n2, lam, n2) == 1 and pow(v * pow(p, -1, n2) % n2, lam, n2) == 1
            ka, _ = kernel_ms(lambda: eng.randomize_batch(y, [rng.randrange(1, n) for _ in y], n))
            kb, _ = kernel_ms(lambda: homomorphic.linear_map(cts, W, n=n, engine=eng, randomizer=fr))
            kc, _ = kernel_ms(lambda: homomorphic.linear_map(cts, W, n=n, engine=eng))
            emit(f"  pipeline dense {dim} x {dim} linear_map, fresh outputs, ints -> ints: + randomize_batch {1e3 * statistics.median(ta):.1f} ms"
                 f" | randomizer= {1e3 * statistics.median(tb):.1f} ms = {statistics.median(ta) / statistics.median(tb):.2f}x"
                 f"; kernels: linear_map {kc:.2f} ms, randomize_batch {ka:.2f} ms, linear_map with randomizer= {kb:.2f} ms")

    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / f"r09_fixed_base_probe{'_quick' if q else ''}.txt").write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
