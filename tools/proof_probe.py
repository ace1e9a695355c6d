#!/usr/bin/env python3
"""Cost of the decryption proofs of a dealt threshold key on one GPU — developer tool, not a test.

(a) Proving and verifying `--count` ciphertexts by stage (device events between the stages of Engine.dleq_prove_t /
    dleq_verify_t: base squarings, multi-exponentiation, fixed-base, hash, response, compare), beside the partial
    decryption alone (Engine.powmod_nsquare_t with the exponent 2 x_i).
(b) The two new kernels — the challenge (mx_sha256_rows over four row sets) and the response (mx_dleq_response) —
    against the route without them: rows to the host, hashlib, Python ints, rows back; the call and its parts.
Forms alternate after a warm-up; every figure is reported as min – median – max over the repeats.  Key lengths in --keys-file
(default: tests/golden/threshold_keys.json) use its safe primes; any other length searches two on the device first.

    python tools/proof_probe.py --key-lengths 2048 4096 --count 10000 --repeats 5 --out profiles/proof_probe.json
"""
from __future__ import annotations

import argparse
import hashlib
import json
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def spread(values):
    return {"min": round(min(values), 3), "median": round(statistics.median(values), 3), "max": round(max(values), 3)}


def stage_ms(stages):
    return {name: prev.elapsed_time(ev) for (_, prev), (name, ev) in zip(stages, stages[1:])}


def probe(eng, key_length, count, repeats, seed, keys_file):
    import numpy as np
    import torch

    from protocols.distributed_keygen_amd import DeviceRng, PaillierPrivateKey, limbs, threshold

    golden = json.loads(Path(keys_file).read_text())["keys"]
    if str(key_length) in golden:
        key = PaillierPrivateKey(int(golden[str(key_length)]["p"], 16), int(golden[str(key_length)]["q"], 16), engine=eng)
    else:
        key = PaillierPrivateKey.generate(key_length, safe=True, engine=eng)
    pub, shares = threshold.deal(key, 5, 2, rng=random.Random(seed), check=False, engine=eng)
    share = shares[1]
    rnd = random.Random(seed + 1)
    cts_t = eng.to_device(limbs.pack([rnd.randrange(1, pub.n_square) for _ in range(count)], pub.limbs2))
    rng = DeviceRng()
    sync = eng.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return out, (time.perf_counter() - t0) * 1e3

    # warm-up: plans, tables, workspaces
    partials_t, proofs = share.partial_decrypt_t(cts_t, prove=True, rng=rng)
    assert bool(pub.verify_t(share.index, cts_t, partials_t, proofs).all())
    x_t = share._x_t
    ctx = pub.ctx(share.index)
    rows = {k: [] for k in ("partial_ms", "prove_ms", "verify_ms", "challenge_device_ms", "challenge_host_ms", "response_device_ms",
                            "response_host_ms")}
    prove_stages, verify_stages, host_parts = [], [], []
    for _ in range(repeats):
        partials_t, ms = timed(lambda: eng.powmod_nsquare_t(cts_t, pub.n, 2 * share.x))
        rows["partial_ms"].append(ms)
        st = []
        (a_t, b_t, z_t), ms = timed(lambda: eng.dleq_prove_t(cts_t, partials_t, pub.n, pub.v_bases, ctx, x_t, pub.rho_bits, pub.kw,
                                                            rng=rng, _stages=st))
        rows["prove_ms"].append(ms)
        prove_stages.append(stage_ms(st))
        st = []
        verdict, ms = timed(lambda: eng.dleq_verify_t(cts_t, partials_t, a_t, b_t, z_t, pub.n, pub.v_bases, pub.verification_key(share.index),
                                                      ctx, pub.z_bits, pub.kw, _stages=st))
        assert bool(verdict.all())
        rows["verify_ms"].append(ms)
        verify_stages.append(stage_ms(st))
        # (b) the challenge and the response: the kernels against the host route, on the same rows
        chat_t = eng.powmod_nsquare_t(cts_t, pub.n, 4)
        ci2_t = eng.mulmod_t(partials_t, partials_t, pub.n_square)
        rho_t = rng.rows_t(eng, count, pub.rho_bits, pub.z_words)
        e_t, ms = timed(lambda: eng._dleq_challenge_t(ctx, chat_t, ci2_t, a_t, b_t))
        rows["challenge_device_ms"].append(ms)
        (zd_t, _), ms = timed(lambda: eng.dleq_response_t(rho_t, e_t, x_t))
        rows["response_device_ms"].append(ms)
        parts = {}

        def host_challenge():
            t0 = time.perf_counter()
            sets = [eng.to_host(t) for t in (chat_t, ci2_t, a_t, b_t)]
            t1 = time.perf_counter()
            be = [np.ascontiguousarray(s[:, ::-1]).astype(">u4") for s in sets]
            digests = [hashlib.sha256(ctx + be[0][r].tobytes() + be[1][r].tobytes() + be[2][r].tobytes() + be[3][r].tobytes()).digest()[:16]
                       for r in range(count)]
            t2 = time.perf_counter()
            out = eng.to_device(np.frombuffer(b"".join(d[::-1] for d in digests), dtype="<u4").reshape(count, 4))
            sync()
            parts.update(challenge_fetch_ms=(t1 - t0) * 1e3, challenge_hashlib_ms=(t2 - t1) * 1e3, challenge_upload_ms=(time.perf_counter() - t2) * 1e3)
            return out

        eh_t, ms = timed(host_challenge)
        rows["challenge_host_ms"].append(ms)
        assert torch.equal(eh_t, e_t)

        def host_response():
            t0 = time.perf_counter()
            rho, e = limbs.unpack(eng.to_host(rho_t)), limbs.unpack(eng.to_host(e_t))
            t1 = time.perf_counter()
            z = [r + k * share.x for r, k in zip(rho, e)]
            t2 = time.perf_counter()
            out = eng.to_device(limbs.pack(z, pub.z_words))
            sync()
            parts.update(response_fetch_ms=(t1 - t0) * 1e3, response_ints_ms=(t2 - t1) * 1e3, response_upload_ms=(time.perf_counter() - t2) * 1e3)
            return out

        zh_t, ms = timed(host_response)
        rows["response_host_ms"].append(ms)
        assert torch.equal(zh_t, zd_t)
        host_parts.append(parts)
    out = {"key_length": key_length, "count": count, "repeats": repeats, "parties": 5, "threshold": 2, "pieces": pub.pieces, "kw": pub.kw,
           "z_words": pub.z_words, "x_words": int(x_t.numel())}
    out.update({k: spread(v) for k, v in rows.items()})
    out["prove_over_partial"] = spread([p / d for p, d in zip(rows["prove_ms"], rows["partial_ms"])])
    out["verify_over_partial"] = spread([p / d for p, d in zip(rows["verify_ms"], rows["partial_ms"])])
    out["prove_stages_ms"] = {k: spread([s[k] for s in prove_stages]) for k in prove_stages[0]}
    out["verify_stages_ms"] = {k: spread([s[k] for s in verify_stages]) for k in verify_stages[0]}
    out["host_route_parts_ms"] = {k: spread([p[k] for p in host_parts]) for k in host_parts[0]}
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--key-lengths", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--count", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--keys-file", default=str(ROOT / "tests" / "golden" / "threshold_keys.json"),
                    help='JSON {"keys": {key length: {"p": hex, "q": hex}}} of safe primes; lengths it lacks are searched on the device')
    ap.add_argument("--out", default=str(ROOT / "profiles" / "proof_probe.json"))
    args = ap.parse_args()
    import torch

    from protocols.distributed_keygen_amd import Engine

    eng = Engine(0)
    result = {"device": torch.cuda.get_device_name(0), "runs": []}
    for kl in args.key_lengths:
        result["runs"].append(probe(eng, kl, args.count, args.repeats, args.seed, args.keys_file))
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
        print(json.dumps(result["runs"][-1]), flush=True)


if __name__ == "__main__":
    main()
