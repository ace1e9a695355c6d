#!/usr/bin/env python3
"""Slot-packed plaintexts against the routes they replace.  One JSON line per part:
  (a) slots.encrypt of --values signed --slot-bits values, ints (a numpy array) to ints, against FastRandomizer.encrypt of the
      same values one per ciphertext; and the kernel time of the two codec kernels on their own (events around the launch);
  (b) slots.decode_t (device rows -> device tensor, events) and slots.decode (ints -> ints, wall) against packing.unpack
      (its numpy path) on the same plaintexts;
  (c) the scoring of examples/slot_packed_scoring.py, samples packed across slots, against homomorphic.matmul of the same
      samples one value per ciphertext with packing.pack before the threshold decryption, scores compared value by value.
Medians of --repeat runs after one warm-up run; tables, plans and the allocator are outside the timing.
   python tools/slots_probe.py [--key-length 2048] [--slot-bits 32] [--values 1000000] [--repeat 3] [--parts abc]
"""
import argparse
import json
import random
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "examples"))


def med_wall(fn, repeat, sync):
    fn()
    out = []
    for _ in range(repeat):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(1e3 * (time.perf_counter() - t0))
        print(f"  run {out[-1]:.1f} ms", file=sys.stderr, flush=True)
    return round(statistics.median(out), 2)


def med_events(torch, fn, repeat):
    fn()
    out = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return round(statistics.median(out), 4)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--slot-bits", type=int, default=32)
    ap.add_argument("--values", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=16)
    ap.add_argument("--scores", type=int, default=4)
    args = ap.parse_args()
    import torch

    from protocols.distributed_keygen_amd import Engine, homomorphic, limbs, packing, slots, synthetic
    from protocols.distributed_keygen_amd.randomizer import FastRandomizer, generate_base

    eng = Engine()
    key = synthetic.make_key(args.key_length, 3, 1)
    n, n2 = key.n, key.n_square
    b, count = args.slot_bits, args.values
    k = packing.slots_per_ciphertext(n, b)
    ln = limbs.limbs_for(n)
    rng = np.random.default_rng(1)
    vals = rng.integers(-(1 << (b - 1)), 1 << (b - 1), size=count, dtype=np.int64)
    fr = FastRandomizer(n, generate_base(n, rng=random.Random(1), engine=eng), engine=eng, device_rng=True)
    head = {"probe": "slots", "key_length": args.key_length, "n_bits": n.bit_length(), "slot_bits": b, "slots": k, "values": count}
    sync = eng.synchronize

    if "a" in args.parts:
        as_list = vals.tolist()
        packed = med_wall(lambda: slots.encrypt(vals, fr, b), args.repeat, sync)
        single = med_wall(lambda: fr.encrypt(as_list), args.repeat, sync)
        v_t = torch.from_numpy(vals).to(eng.device)
        rows_t = eng.slots_encode_t(v_t, n, b)
        out_t, st_t = torch.empty_like(rows_t), torch.empty(rows_t.shape[0], dtype=torch.uint8, device=eng.device)
        dec_t = torch.empty(count, dtype=torch.int64, device=eng.device)
        h_n = limbs.pack_one(n, ln)
        enc_ms = med_events(torch, lambda: eng._call("mx_slots_encode", v_t.data_ptr(), count, h_n.ctypes.data, ln, b, k, 1,
                                                     out_t.data_ptr(), ln, st_t.data_ptr()), args.repeat)
        dec_ms = med_events(torch, lambda: eng._call("mx_slots_decode", rows_t.data_ptr(), ln, count, h_n.ctypes.data, ln, b, k, 1,
                                                     dec_t.data_ptr()), args.repeat)
        ok = bool((out_t == rows_t).all()) and bool((dec_t == v_t).all()) and not bool(st_t.any())
        moved = 8 * count + 4 * ln * rows_t.shape[0]
        print(json.dumps({**head, "part": "a", "ciphertexts_packed": rows_t.shape[0], "ciphertexts_single": count,
                          "encrypt_packed_wall_ms": packed, "encrypt_single_wall_ms": single, "ratio": round(single / packed, 1),
                          "encode_kernel_ms": enc_ms, "decode_kernel_ms": dec_ms,
                          "encode_GBps": round(moved / enc_ms / 1e6, 1), "decode_GBps": round(moved / dec_ms / 1e6, 1),
                          "codec_round_trip_ok": ok}), flush=True)
        del v_t, rows_t, out_t, dec_t, as_list

    if "b" in args.parts:
        plain = slots.encode(vals, n, b, engine=eng)
        rows_t = eng.to_device(limbs.pack(plain, ln))
        want = packing.unpack(plain, b, count, n)
        same = slots.decode(plain, n, b, count, engine=eng) == want and slots.decode_t(rows_t, n, b, count, engine=eng).tolist() == want
        dev = med_events(torch, lambda: slots.decode_t(rows_t, n, b, count, engine=eng), args.repeat)
        ints = med_wall(lambda: slots.decode(plain, n, b, count, engine=eng), args.repeat, sync)
        tens = med_wall(lambda: slots.decode_t(rows_t, n, b, count, engine=eng).cpu(), args.repeat, sync)
        host = med_wall(lambda: packing.unpack(plain, b, count, n), args.repeat, sync)
        print(json.dumps({**head, "part": "b", "plaintexts": len(plain), "decode_t_device_ms": dev,
                          "decode_t_rows_to_host_tensor_wall_ms": tens, "decode_ints_to_ints_wall_ms": ints,
                          "packing_unpack_wall_ms": host, "equal": same}), flush=True)

    if "c" in args.parts:
        import slot_packed_scoring as ex

        B, I, R = args.batch, args.features, args.scores
        x = rng.integers(-128, 128, size=(B, I))
        W = rng.integers(-255, 256, size=(R, I))
        bias = rng.integers(-1023, 1024, size=R)
        l2 = limbs.limbs_for(n2)

        def decrypt_rows(flat):
            partials = []
            for i in (1, 2, 3):
                e = key.exponent(i)
                bases = flat if e >= 0 else eng.modinv_batch(flat, n2)
                partials.append(eng.powmod_nsquare_t(eng.to_device(limbs.pack_reduced(bases, l2, n2)), n, abs(e)))
            return eng.combine_t(torch.stack(partials), n, key.theta_inv, packed=True)

        def packed():
            return ex.packed_scores(eng, key, fr, x, W, bias)[0].cpu().numpy()

        def unpacked():
            flat = fr.encrypt([int(v) for v in x.reshape(-1)])
            scores = homomorphic.matmul([flat[s * I : (s + 1) * I] for s in range(B)], W.tolist(), n=n, bias=[int(v) for v in bias],
                                        engine=eng, randomizer=fr)
            pk = packing.pack([c for row in scores for c in row], 32, n=n, engine=eng)
            rows_t = decrypt_rows(pk)
            return slots.decode_t(rows_t, n, 32, B * R, engine=eng).cpu().numpy().reshape(B, R)

        want = x @ W.T + bias
        equal = bool((packed() == want).all()) and bool((unpacked() == want).all())
        _, sb, n_enc, n_dec = ex.packed_scores(eng, key, fr, x, W, bias)
        t_p = med_wall(packed, args.repeat, sync)
        t_u = med_wall(unpacked, args.repeat, sync)
        k32 = packing.slots_per_ciphertext(n, 32)
        print(json.dumps({**head, "part": "c", "batch": B, "features": I, "scores": R, "score_slot_bits": sb,
                          "score_slots": packing.slots_per_ciphertext(n, sb), "packed_wall_ms": t_p, "unpacked_wall_ms": t_u,
                          "ratio": round(t_u / t_p, 1), "encryptions": [n_enc, B * I], "matmul_samples": [-(-B // packing.slots_per_ciphertext(n, sb)), B],
                          "threshold_decryptions": [n_dec, -(-B * R // k32)], "scores_equal": equal}), flush=True)
        assert equal, "the routes disagree"


if __name__ == "__main__":
    main()
