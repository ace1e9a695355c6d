"""Packed threshold decryption: the packing kernel against the same packing through the multi-
exponentiation kernel, the lone chain of one packed output, and threshold decryption of many small values packed
against unpacked — engine pipeline and the patched stand-in with three parties.

    python tools/packed_decrypt_probe.py [--out DIR] [--quick] [--key-lengths 2048,4096]

Every packed / unpacked pair runs alternately in the same process (median of the repetitions), timed with a
synchronize after each run, and the two outputs are compared bit for bit.  Writes DIR/r08_packed_decrypt_probe.txt.
"""

from __future__ import annotations

import argparse
import asyncio
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def alternate(fa, fb, reps=3, warmup=1):
    """(median seconds of fa, of fb, last outputs) with fa and fb run one after the other, reps times."""
    import torch

    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    oa = ob = None
    for _ in range(reps):
        for f, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            if f is fa:
                oa = out
            else:
                ob = out
    return statistics.median(ta), statistics.median(tb), oa, ob


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles", help="directory of the result file (default: profiles/)")
    ap.add_argument("--quick", action="store_true", help="smaller cases (a smoke run of the probe itself)")
    ap.add_argument("--key-lengths", default="2048,4096")
    ap.add_argument("--skip", default="", help="comma-separated sections to skip: kernel,lone,pipeline,standin")
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import Engine, configure_hw_queues, limbs, packing, patch, synthetic

    import standin_harness as sh
    import torch

    configure_hw_queues(16)
    eng = Engine(0)
    q = args.quick
    skip = set(filter(None, args.skip.split(",")))
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    def kernel_ms(fn):
        eng.profile_collect()
        eng.profile(True)
        fn()
        eng.profile(False)
        return eng.profile_collect()

    for kl in [int(x) for x in args.key_lengths.split(",")]:
        key = synthetic.make_key(kl, 3, 1)
        n, n2 = key.n, key.n_square
        l2 = limbs.limbs_for(n2)
        nb = n.bit_length()
        rng = random.Random(kl)
        emit(f"key_length {kl} (N {nb} bits, N^2 rows of {l2} words); slots per ciphertext: "
             f"b=32 -> {packing.slots_per_ciphertext(n, 32)}, b=64 -> {packing.slots_per_ciphertext(n, 64)}")
        pool = synthetic.random_ciphertexts(key, 100_000, seed=5)

        # ---- 1. the packing kernel against the same packing through linear_map (weights 2^(b i))
        if "kernel" not in skip:
            for b in (32, 64):
                k = packing.slots_per_ciphertext(n, b)
                for m in ((1000, 10_000) if q else (10_000, 100_000)):
                    x_t = eng.to_device(limbs.pack_reduced(pool[:m], l2, n2))
                    rows = [{j * k + i: 1 << (b * i) for i in range(min(k, m - j * k))} for j in range(-(-m // k))]
                    t_p, t_l, p_t, l_t = alternate(lambda: eng.pack_nsquare_t(x_t, n, b, k),
                                                   lambda: eng.multiexp_nsquare_t(x_t, rows, n), reps=3)
                    assert torch.equal(p_t, l_t), (kl, b, m)
                    kp, _ = kernel_ms(lambda: eng.pack_nsquare_t(x_t, n, b, k))
                    kl_ms, kl_n = kernel_ms(lambda: eng.multiexp_nsquare_t(x_t, rows, n))
                    emit(f"  pack b={b} values={m} outputs={len(rows)}: pack_nsquare_t {1e3 * t_p:.2f} ms (kernel {kp:.2f} ms)"
                         f" | linear_map route {1e3 * t_l:.2f} ms (kernels {kl_ms:.2f} ms in {kl_n} runs)"
                         f" = {t_l / t_p:.1f}x the call, {kl_ms / max(kp, 1e-9):.1f}x the kernel time; bit-identical")

        # ---- 2. the lone chain of one packed output
        if "lone" not in skip:
            for b in (32, 64):
                k = packing.slots_per_ciphertext(n, b)
                x_t = eng.to_device(limbs.pack_reduced(pool[:k], l2, n2))
                one_t = eng.to_device(limbs.pack_reduced(pool[:1], l2, n2))
                t_p, t_d, _, _ = alternate(lambda: eng.pack_nsquare_t(x_t, n, b, k),
                                           lambda: eng.powmod_nsquare_t(one_t, n, abs(key.exponent(1))), reps=5)
                kp, _ = kernel_ms(lambda: eng.pack_nsquare_t(x_t, n, b, k))
                emit(f"  lone chain b={b} ({k} slots, {(k - 1) * b} squarings): {1e3 * t_p:.2f} ms (kernel {kp:.2f} ms)"
                     f" | one partial decryption of one ciphertext {1e3 * t_d:.2f} ms")

        # ---- 3. engine pipeline, ints to ints: three parties' partial decryptions, combine, (unpack)
        def encrypt(vals):
            r = [pow(rng.randrange(1, n), n, n2) for _ in range(64)]
            base = [(1 + (v % n) * n) % n2 for v in vals]
            return eng.mulmod_batch(base, [r[i % 64] for i in range(len(vals))], n2)

        def decrypt_ints(cts):
            partials = []
            for i in (1, 2, 3):
                e = key.exponent(i)
                bases = cts if e >= 0 else eng.modinv_batch(cts, n2)
                partials.append(eng.powmod_nsquare_batch(bases, abs(e), n))
            out, ok = eng.combine_batch([list(t) for t in zip(*partials)], n, key.theta_inv)
            assert all(ok)
            return out

        def unpacked(cts):
            half = n // 2
            return [m - n if m > half else m for m in decrypt_ints(cts)]

        def packed(cts, b=32):
            p = eng.ciphertext_pack_batch(cts, n, b, packing.slots_per_ciphertext(n, b))
            return packing.unpack(decrypt_ints(p), b, len(cts), n)

        if "pipeline" not in skip:
            sizes = (1000, 10_000) if q else ((1000, 10_000, 100_000, 1_000_000) if kl == 2048 else (1000, 10_000, 100_000))
            for m in sizes:
                vals = [rng.randrange(-(1 << 31), 1 << 31) for _ in range(m)]
                cts = encrypt(vals)
                reps = 3 if m <= 100_000 else 1
                t_p, t_u, got_p, got_u = alternate(lambda: packed(cts), lambda: unpacked(cts), reps=reps, warmup=1 if m <= 100_000 else 0)
                assert got_p == got_u == vals, (kl, m)
                emit(f"  pipeline signed 32-bit values={m}: packed {1e3 * t_p:.1f} ms | unpacked {1e3 * t_u:.1f} ms"
                     f" = {t_u / t_p:.2f}x; identical values")

        # ---- 4. three stand-in parties with patch.install on the HIP engine
        if "standin" not in skip:
            for m in ((1000,) if q else (10_000, 100_000)):
                vals = [rng.randrange(-(1 << 31), 1 << 31) for _ in range(m)]
                cts = encrypt(vals)
                patch.install(engine=eng, package=sh.PACKAGE)
                try:
                    def run_packed():
                        parties = sh.parties_for_key(key)
                        cobjs = sh.ciphertexts(key, cts)

                        async def go():
                            return await asyncio.gather(*[packing.decrypt_sequence_packed(dp, cobjs, 32, engine=eng) for dp in parties])

                        return asyncio.run(go())

                    def run_raw():
                        res = sh.decrypt_sequence(sh.parties_for_key(key), sh.ciphertexts(key, cts))
                        half = n // 2
                        return [[e.value - n if e.value > half else e.value for e in r] for r in res]

                    t_p, t_u, got_p, got_u = alternate(run_packed, run_raw, reps=3 if m <= 10_000 else 2)
                finally:
                    patch.uninstall()
                assert got_p == got_u == [vals] * 3, (kl, m)
                emit(f"  stand-in, 3 parties, patched, signed 32-bit values={m}: decrypt_sequence_packed {1e3 * t_p:.1f} ms"
                     f" | _decrypt_sequence_raw {1e3 * t_u:.1f} ms = {t_u / t_p:.2f}x; identical values")

        # ---- 5. traffic: partial decryptions each party sends (one residue mod N^2 each, to each other party)
        row = (2 * nb + 7) // 8
        for b in (32, 64):
            k = packing.slots_per_ciphertext(n, b)
            for m in (1000, 100_000):
                emit(f"  traffic b={b} values={m}: {m * row} B unpacked, {-(-m // k) * row} B packed per party and receiver"
                     f" ({m / -(-m // k):.1f}x fewer)")

    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / f"r08_packed_decrypt_probe{'_quick' if q else ''}.txt").write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
