#!/usr/bin/env python3
"""Cost of the one-of-k membership proofs on one GPU — developer tool, not a test.

(a) Proving and verifying `--count` ciphertexts over lists of k values by stage (device events between the stages of
    Engine.member_prove_t / member_verify_t: the challenge kernel, the inverse and the branch rows, r^N, the
    multi-exponentiation modulo N^2, hash, response, compares), beside a plain encryption of the same rows on the device
    (r^N and the product with 1 + m N).
(b) The challenge kernel (csrc/mx_member.hpp: mask, split and sum, one launch each) against the route without it: rows to
    the host, Python ints, rows back — which would also carry the secret index through Python ints.
Forms alternate after a warm-up; every figure is min – median – max over the repeats.  Key lengths in --keys-file (default:
tests/golden/threshold_keys.json) use its safe primes for N; any other length uses a key generated on the device for the run
(PaillierPrivateKey.generate) — the prover inverts its ciphertexts, so N has to be a proper key.

    python tools/member_probe.py --key-lengths 2048 4096 --ks 2 4 16 --count 10000 --repeats 5 --out profiles/member_probe.json
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
M128 = (1 << 128) - 1


def spread(values):
    return {"min": round(min(values), 3), "median": round(statistics.median(values), 3), "max": round(max(values), 3)}


def stage_ms(stages):
    return {name: prev.elapsed_time(ev) for (_, prev), (name, ev) in zip(stages, stages[1:])}


_generated = {}


def modulus(eng, key_length, keys_file):
    """(N, generated): the golden key of that length, else a key generated on the device once per run (the prover inverts
    its ciphertexts, so N must be a proper key: a random odd number has small factors that the randomness meets)."""
    golden = json.loads(Path(keys_file).read_text())["keys"]
    if str(key_length) in golden:
        p, q = (int(golden[str(key_length)][k], 16) for k in "pq")
        return p * q, False
    if key_length not in _generated:
        from protocols.distributed_keygen_amd import PaillierPrivateKey

        _generated[key_length] = int(PaillierPrivateKey.generate(key_length, engine=eng).n)
    return _generated[key_length], True


def probe(eng, key_length, k, count, repeats, seed, keys_file):
    import torch

    from protocols.distributed_keygen_amd import DeviceRng, limbs, membership

    n, generated = modulus(eng, key_length, keys_file)
    rnd = random.Random(seed + k)
    values = list(range(k))
    sh = membership.shape(n, k)
    ctx = membership.context(n, values, b"probe")
    rng = DeviceRng()
    sync = eng.synchronize
    n2 = n * n
    index = [rnd.randrange(k) for _ in range(count)]
    index_t = torch.tensor(index, dtype=torch.int32, device=eng.device)
    onemn_t = eng.to_device(limbs.pack([1 + values[i] * n for i in index], sh["limbs2"]))
    r_wide_t = rng.rows_t(eng, count, sh["draw_bits"], sh["limbs2"])
    r_t = eng._reduce_wide_t(r_wide_t, n)
    cts_t = eng.mulmod_t(eng.powmod_nsquare_t(r_wide_t, n, n), onemn_t, n2)

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return out, (time.perf_counter() - t0) * 1e3

    def prove(st=None):
        return eng.member_prove_t(cts_t, index_t, r_t, n, values, ctx, rng=rng, _stages=st)

    proof = prove()                                                      # warm-up: plans, workspaces
    assert bool(eng.member_verify_t(cts_t, *proof, n, values, ctx).all())
    rows = {name: [] for name in ("encrypt_ms", "prove_ms", "verify_ms", "challenges_device_ms", "challenges_host_ms")}
    prove_stages, verify_stages = [], []
    sim_t = rng.rows_t(eng, count * k, 128).view(count, 4 * k)
    e_t = rng.rows_t(eng, count, 128)

    def device_challenges():
        masked_t = eng.member_challenges_t(None, sim_t, index_t, 0)
        split_t = eng.member_challenges_t(e_t, masked_t, index_t, 1)
        return split_t, eng.member_challenges_t(e_t, split_t, None, 2)

    def host_challenges():
        sims, es, idx = limbs.unpack(eng.to_host(sim_t.view(count * k, 4))), limbs.unpack(eng.to_host(e_t)), index_t.cpu().tolist()
        out, status = [], []
        for r in range(count):
            row = [0 if j == idx[r] else sims[r * k + j] for j in range(k)]
            row[idx[r]] = (es[r] - sum(row)) & M128
            out.extend(row)
            status.append(int(sum(row) & M128 != es[r]))
        return eng.to_device(limbs.pack(out, 4)).view(count, 4 * k), torch.tensor(status, dtype=torch.uint8, device=eng.device)

    device_challenges()
    for _ in range(repeats):
        _, ms = timed(lambda: eng.mulmod_t(eng.powmod_nsquare_t(rng.rows_t(eng, count, sh["draw_bits"], sh["limbs2"]), n, n), onemn_t, n2))
        rows["encrypt_ms"].append(ms)
        st = []
        proof, ms = timed(lambda: prove(st))
        rows["prove_ms"].append(ms)
        prove_stages.append(stage_ms(st))
        st = []
        verdict, ms = timed(lambda: eng.member_verify_t(cts_t, *proof, n, values, ctx, _stages=st))
        assert bool(verdict.all())
        rows["verify_ms"].append(ms)
        verify_stages.append(stage_ms(st))
        (new_t, new_status), ms = timed(device_challenges)
        rows["challenges_device_ms"].append(ms)
        (old_t, old_status), ms = timed(host_challenges)
        rows["challenges_host_ms"].append(ms)
        assert torch.equal(new_t, old_t) and torch.equal(new_status, old_status) and not bool(new_status.any())
    out = {"key_length": key_length, "k": k, "count": count, "repeats": repeats, "generated_key": generated}
    out.update({name: spread(v) for name, v in rows.items()})
    out["prove_over_encrypt"] = spread([p / d for p, d in zip(rows["prove_ms"], rows["encrypt_ms"])])
    out["verify_over_encrypt"] = spread([p / d for p, d in zip(rows["verify_ms"], rows["encrypt_ms"])])
    out["prove_stages_ms"] = {name: spread([s[name] for s in prove_stages]) for name in prove_stages[0]}
    out["verify_stages_ms"] = {name: spread([s[name] for s in verify_stages]) for name in verify_stages[0]}
    dev, host = out["challenges_device_ms"], out["challenges_host_ms"]
    out["kernel_stays"] = bool(host["median"] - dev["median"] > max(dev["max"] - dev["min"], host["max"] - host["min"]))
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--key-lengths", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 4, 16])
    ap.add_argument("--count", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--keys-file", default=str(ROOT / "tests" / "golden" / "threshold_keys.json"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "member_probe.json"))
    args = ap.parse_args()
    import torch

    from protocols.distributed_keygen_amd import Engine

    eng = Engine(0)
    result = {"device": torch.cuda.get_device_name(0), "runs": []}
    for kl in args.key_lengths:
        for k in args.ks:
            result["runs"].append(probe(eng, kl, k, args.count, args.repeats, args.seed, args.keys_file))
            Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
            print(json.dumps(result["runs"][-1]), flush=True)


if __name__ == "__main__":
    main()
