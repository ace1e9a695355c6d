"""Exponents and randomness drawn on the device against the host draw, on the device in use.

    python tools/device_rng_probe.py [--out DIR] [--quick] [--reps 7]

1. FastRandomizer.encrypt, ints to ints, with host-drawn and with device-drawn exponents, alternating in one process:
   key_length 2048 at 10^3, 10^4 and 10^5 messages, key_length 4096 at 10^5.  Medians [min, max] of the call and of its
   parts: drawing the exponents on the host (FastRandomizer.draw), uploading them (to_device, waited for), the generator's
   kernel and the encryption kernel (events around the launches).  The host-draw path is the comparison baseline.
2. Engine.encrypt_fresh_batch against Engine.encrypt_batch fed secrets.randbelow(N) values (drawing them included, and
   on its own).
Outputs are checked: a sample of every device-drawn batch against pow with the exponents / randomness the model
(tools/chacha_model.py) gives for the generator's key.  Writes DIR/r10_device_rng_probe.txt.
"""

from __future__ import annotations

import argparse
import random
import secrets
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
    ap.add_argument("--quick", action="store_true", help="smaller cases (a smoke run of the probe itself)")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch

    import chacha_model
    from protocols.distributed_keygen_amd import DeviceRng, Engine, configure_hw_queues, limbs, randomizer, synthetic

    configure_hw_queues(16)
    eng = Engine(0)
    q = args.quick
    reps = args.reps
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
        """Seconds between two events around the launches of fn on the current stream."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    seed = bytes(range(32))
    cases = [(2048, 1000), (2048, 10_000)] if q else [(2048, 1000), (2048, 10_000), (2048, 100_000), (4096, 100_000)]
    emit("FastRandomizer.encrypt, ints -> ints: exponents drawn on the host (os.urandom, uploaded) against drawn on the device"
         f" (chacha20_rows_kernel); {reps} alternating runs, ms, median [min, max]")
    for kl, count in cases:
        key = synthetic.make_key(kl, 3, 1)
        n, n2 = key.n, key.n_square
        ln = limbs.limbs_for(n)
        rnd = random.Random(kl + count)
        h_s = randomizer.generate_base(n, rng=rnd, engine=eng)
        host = randomizer.FastRandomizer(n, h_s, engine=eng)
        dev = randomizer.FastRandomizer(n, h_s, engine=eng, device_rng=DeviceRng(key=seed))
        eb = host.exp_bits
        msgs = [rnd.randrange(-(1 << 31), 1 << 31) for _ in range(count)]
        table = eng.fixed_base_table(n, h_s, eb, 0)
        m_t = eng.to_device(limbs.pack([m % n for m in msgs], ln))
        host.encrypt(msgs[:64]), dev.encrypt(msgs[:64])                  # table, pinned buffers, first launches
        host.encrypt(msgs), dev.encrypt(msgs)
        t = {k: [] for k in ("host call", "device call", "draw", "upload", "rng kernel", "encrypt kernel")}
        for _ in range(reps):
            t["host call"].append(wall(lambda: host.encrypt(msgs))[0])
            call = dev.device_rng.next_call
            dt, out = wall(lambda: dev.encrypt(msgs))
            t["device call"].append(dt)
            dt, rows = wall(lambda: host.draw(count))
            t["draw"].append(dt)
            dt, e_t = wall(lambda: eng.fixed_base_exponent_rows(rows, eb))
            t["upload"].append(dt)
            dt, d_t = event_s(lambda: dev.device_rng.rows_t(eng, count, eb))
            t["rng kernel"].append(dt)
            t["encrypt kernel"].append(event_s(lambda: eng.fixed_base_encrypt_t(table, d_t, m_t))[0])
        a = chacha_model.row_ints(seed, call, 3, eb)                      # the first rows of a call do not depend on its count
        assert out[:3] == [(1 + (m % n) * n) * pow(h_s, x, n2) % n2 for m, x in zip(msgs, a)], (kl, count)
        emit(f"  key_length {kl} exp_bits {eb} count {count}:")
        emit(f"    call with host-drawn exponents    {fmt(t['host call'])}")
        emit(f"    call with device-drawn exponents  {fmt(t['device call'])}"
             f"   = {1e3 * (statistics.median(t['host call']) - statistics.median(t['device call'])):+.3f} ms saved,"
             f" {statistics.median(t['host call']) / statistics.median(t['device call']):.2f}x")
        emit(f"    parts: host draw {fmt(t['draw'])} | upload {fmt(t['upload'])} | rng kernel {fmt(t['rng kernel'])}"
             f" | encrypt kernel {fmt(t['encrypt kernel'])}")
        emit(f"    rng kernel / encrypt kernel = {100 * statistics.median(t['rng kernel']) / statistics.median(t['encrypt kernel']):.2f} %;"
             f" rng kernel writes {count * ((eb + 31) // 32) * 4 / 1e6:.2f} MB")

    emit("Engine.encrypt_fresh_batch (r drawn on the device) against Engine.encrypt_batch fed secrets.randbelow(N): ints -> ints, ms")
    for kl, count in [(2048, 1000)] if q else [(2048, 1000), (2048, 10_000)]:
        key = synthetic.make_key(kl, 3, 1)
        n, n2 = key.n, key.n_square
        rnd = random.Random(kl)
        msgs = [rnd.randrange(-(1 << 31), 1 << 31) for _ in range(count)]
        rng = DeviceRng(key=seed)
        eng.encrypt_fresh_batch(msgs, n, rng), eng.encrypt_batch(msgs, [secrets.randbelow(n) for _ in msgs], n)
        t = {k: [] for k in ("host", "device", "randbelow", "rng kernel")}
        for _ in range(max(3, reps // 2)):
            t["host"].append(wall(lambda: eng.encrypt_batch(msgs, [secrets.randbelow(n) for _ in msgs], n))[0])
            call = rng.next_call
            dt, out = wall(lambda: eng.encrypt_fresh_batch(msgs, n, rng))
            t["device"].append(dt)
            t["randbelow"].append(wall(lambda: [secrets.randbelow(n) for _ in msgs])[0])
            t["rng kernel"].append(event_s(lambda: rng.rows_t(eng, count, n.bit_length() + 64, limbs.limbs_for(n2)))[0])
        r = chacha_model.row_ints(seed, call, 2, n.bit_length() + 64, limbs.limbs_for(n2))
        assert out[:2] == [(1 + (m % n) * n) * pow(v % n, n, n2) % n2 for m, v in zip(msgs, r)], (kl, count)
        emit(f"  key_length {kl} count {count}: encrypt_batch + randbelow {fmt(t['host'])} | encrypt_fresh_batch {fmt(t['device'])}"
             f" = {1e3 * (statistics.median(t['host']) - statistics.median(t['device'])):+.3f} ms saved"
             f" | randbelow alone {fmt(t['randbelow'])} | rng kernel {fmt(t['rng kernel'])}")

    out_dir = Path(args.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / f"r10_device_rng_probe{'_quick' if q else ''}.txt").write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
