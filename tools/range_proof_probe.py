#!/usr/bin/env python3
"""Cost of the range proofs on one GPU — developer tool, not a test.

(a) Proving and verifying `--count` ciphertexts by stage (device events between the stages of Engine.range_prove_t /
    range_verify_t: the launches modulo Nh, r^N, the multi-exponentiations modulo N^2, hash, responses, the launch modulo
    N, compares), beside a plain encryption of the same rows on the device (r^N and the product with 1 + m N).
(b) The two new kernels against the route without them.  S = s^m t^mu mod Nh (shared bases) and z2 = rho r^e mod N
    (per-row bases) through Engine.multiexp_mod_t, against powmod_multi_t with one group per row — modulus and exponent
    copied per row — for each term and mulmod_t to join them: the two routes of Engine._shared_pair_t / _own_pair_t,
    between which the proofs choose by these figures (Engine.RANGE_MULTIEXP_MIN_BITS).  z1 = alpha + e m through Engine.response_rows_t against
    rows to the host, Python ints, rows back.
Forms alternate after a warm-up; every figure is min – median – max over the repeats.  Key lengths in --keys-file (default:
tests/golden/threshold_keys.json) use its safe primes for N and Nh; any other length uses random odd moduli of that length
— the arithmetic and its cost are the same, and the equations of the proof hold for any odd moduli.

    python tools/range_proof_probe.py --key-lengths 2048 4096 --count 10000 --repeats 5 --out profiles/range_proof_probe.json
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


def spread(values):
    return {"min": round(min(values), 3), "median": round(statistics.median(values), 3), "max": round(max(values), 3)}


def stage_ms(stages):
    return {name: prev.elapsed_time(ev) for (_, prev), (name, ev) in zip(stages, stages[1:])}


def moduli(key_length, keys_file, seed):
    golden = json.loads(Path(keys_file).read_text())["keys"]
    rnd = random.Random(seed)
    if str(key_length) in golden:
        p, q = (int(golden[str(key_length)][k], 16) for k in "pq")
        other = rnd.getrandbits(key_length) | (1 << (key_length - 1)) | 1
        return p * q, other, False
    return tuple(rnd.getrandbits(key_length) | (1 << (key_length - 1)) | 1 for _ in range(2)) + (True,)


def probe(eng, key_length, count, bits, repeats, seed, keys_file):
    import torch

    from protocols.distributed_keygen_amd import DeviceRng, limbs, range_proof

    n, nh, synthetic = moduli(key_length, keys_file, seed)
    rnd = random.Random(seed + 1)
    t = pow(rnd.randrange(2, nh), 2, nh)
    params = range_proof.RangeParameters(nh, pow(t, rnd.getrandbits(key_length - 2), nh), t)
    sh = range_proof.shape(n, nh, bits)
    ctx = range_proof.context(n, params, bits, b"probe")
    rng = DeviceRng()
    sync = eng.synchronize
    n2 = n * n
    msgs = [rnd.getrandbits(bits) for _ in range(count)]
    m_t = eng.to_device(limbs.pack(msgs, sh["z1_words"]))
    onemn_t = eng.to_device(limbs.pack([1 + m * n for m in msgs], sh["limbs2"]))
    r_wide_t = rng.rows_t(eng, count, sh["rho_bits"], sh["limbs2"])
    r_t = eng._reduce_wide_t(r_wide_t, n)
    cts_t = eng.mulmod_t(eng.powmod_nsquare_t(r_wide_t, n, n), onemn_t, n2)

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return out, (time.perf_counter() - t0) * 1e3

    def prove(st=None):
        return eng.range_prove_t(cts_t, m_t, r_t, n, nh, params.s, params.t, bits, ctx, rng=rng, message_bits=bits, _stages=st)

    proof = prove()                                                      # warm-up: plans, workspaces
    assert bool(eng.range_verify_t(cts_t, *proof, n, nh, params.s, params.t, bits, ctx).all())
    rows = {k: [] for k in ("encrypt_ms", "prove_ms", "verify_ms", "shared_multiexp_ms", "shared_parent_ms", "own_multiexp_ms",
                            "own_parent_ms", "response_device_ms", "response_host_ms")}
    prove_stages, verify_stages = [], []
    lh, ln = sh["limbs_h"], sh["limbs_n"]
    mu_t = rng.rows_t(eng, count, sh["mu_bits"])
    alpha_t = rng.rows_t(eng, count, sh["alpha_bits"], sh["z1_words"])
    e_t = rng.rows_t(eng, count, 128)
    rho_t = eng._reduce_wide_t(rng.rows_t(eng, count, sh["rho_bits"], sh["limbs2"]), n)
    for _ in range(repeats):
        _, ms = timed(lambda: eng.mulmod_t(eng.powmod_nsquare_t(rng.rows_t(eng, count, sh["rho_bits"], sh["limbs2"]), n, n), onemn_t, n2))
        rows["encrypt_ms"].append(ms)
        st = []
        proof, ms = timed(lambda: prove(st))
        rows["prove_ms"].append(ms)
        prove_stages.append(stage_ms(st))
        st = []
        verdict, ms = timed(lambda: eng.range_verify_t(cts_t, *proof, n, nh, params.s, params.t, bits, ctx, _stages=st))
        assert bool(verdict.all())
        rows["verify_ms"].append(ms)
        verify_stages.append(stage_ms(st))
        # (b) shared bases: s^m t^mu mod Nh
        new_t, ms = timed(lambda: eng._shared_pair_t(params.s, params.t, m_t, mu_t, nh, bits, sh["mu_bits"], route="multiexp"))
        rows["shared_multiexp_ms"].append(ms)
        old_t, ms = timed(lambda: eng._shared_pair_t(params.s, params.t, m_t, mu_t, nh, bits, sh["mu_bits"], route="modexps"))
        rows["shared_parent_ms"].append(ms)
        assert torch.equal(new_t, old_t)
        # per-row bases: rho r^e mod N
        new_t, ms = timed(lambda: eng._own_pair_t(rho_t, r_t, e_t, n, route="multiexp"))
        rows["own_multiexp_ms"].append(ms)
        old_t, ms = timed(lambda: eng._own_pair_t(rho_t, r_t, e_t, n, route="modexps"))
        rows["own_parent_ms"].append(ms)
        assert torch.equal(new_t, old_t)
        # the response rows
        (zd_t, _), ms = timed(lambda: eng.response_rows_t(alpha_t, e_t, m_t))
        rows["response_device_ms"].append(ms)

        def host_response():
            a, e, m = (limbs.unpack(eng.to_host(x)) for x in (alpha_t, e_t, m_t))
            return eng.to_device(limbs.pack([x + y * z for x, y, z in zip(a, e, m)], sh["z1_words"]))

        zh_t, ms = timed(host_response)
        rows["response_host_ms"].append(ms)
        assert torch.equal(zh_t, zd_t)
    k, l, w_shared = eng.multiexp_mod_shape(nh, 2, count, 2, 32 * max(sh["z1_words"], (sh["mu_bits"] + 31) // 32))
    out = {"key_length": key_length, "aux_length": nh.bit_length(), "count": count, "bits": bits, "repeats": repeats, "synthetic_moduli": synthetic,
           "lanes": k, "limbs_per_lane": l, "proof_takes_multiexp": bool(eng.range_uses_multiexp(nh)), "window_shared": w_shared, "window_own": eng.multiexp_mod_shape(n, 2 * count, count, 2, 128)[2]}
    out.update({k_: spread(v) for k_, v in rows.items()})
    out["prove_over_encrypt"] = spread([p / d for p, d in zip(rows["prove_ms"], rows["encrypt_ms"])])
    out["verify_over_encrypt"] = spread([p / d for p, d in zip(rows["verify_ms"], rows["encrypt_ms"])])
    out["prove_stages_ms"] = {k_: spread([s[k_] for s in prove_stages]) for k_ in prove_stages[0]}
    out["verify_stages_ms"] = {k_: spread([s[k_] for s in verify_stages]) for k_ in verify_stages[0]}
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--key-lengths", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--count", type=int, default=10000)
    ap.add_argument("--bits", type=int, default=64, help="the claimed bit length l")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--keys-file", default=str(ROOT / "tests" / "golden" / "threshold_keys.json"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "range_proof_probe.json"))
    args = ap.parse_args()
    import torch

    from protocols.distributed_keygen_amd import Engine

    eng = Engine(0)
    result = {"device": torch.cuda.get_device_name(0), "runs": []}
    for kl in args.key_lengths:
        result["runs"].append(probe(eng, kl, args.count, args.bits, args.repeats, args.seed, args.keys_file))
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
        print(json.dumps(result["runs"][-1]), flush=True)


if __name__ == "__main__":
    main()
