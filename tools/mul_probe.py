#!/usr/bin/env python3
"""Cost of the multiplication proofs on one GPU — developer tool, not a test.

(a) Proving and verifying `--count` statements by stage (device events between the stages of Engine.mul_prove_t /
    mul_verify_t: the reductions, r^N, the multi-exponentiation modulo N^2, hash, the response modulo N, the products
    modulo N, compares), beside a plain encryption of the same rows on the device (r^N and the product with 1 + m N).
(b) The response kernel (csrc/mx_response_mod.hpp: (w, t) = divmod(x + e a, N), one launch) against the route without
    it: rows to the host, Python divmod, rows back — which would also carry a and x through Python ints.
Forms alternate after a warm-up; every figure is min – median – max over the repeats.  Key lengths in --keys-file (default:
tests/golden/threshold_keys.json) use its safe primes for N; any other length uses a key generated on the device for the run.

    python tools/mul_probe.py --key-lengths 2048 4096 --count 10000 --repeats 5 --out profiles/mul_probe.json
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


def spread(values):
    return {"min": round(min(values), 3), "median": round(statistics.median(values), 3), "max": round(max(values), 3)}


def stage_ms(stages):
    return {name: prev.elapsed_time(ev) for (_, prev), (name, ev) in zip(stages, stages[1:])}


_generated = {}


def modulus(eng, key_length, keys_file):
    """(N, generated): the golden key of that length, else a key generated on the device once per run."""
    golden = json.loads(Path(keys_file).read_text())["keys"]
    if str(key_length) in golden:
        p, q = (int(golden[str(key_length)][k], 16) for k in "pq")
        return p * q, False
    if key_length not in _generated:
        from protocols.distributed_keygen_amd import PaillierPrivateKey

        _generated[key_length] = int(PaillierPrivateKey.generate(key_length, engine=eng).n)
    return _generated[key_length], True


def probe(eng, key_length, count, repeats, keys_file):
    import torch

    from protocols.distributed_keygen_amd import DeviceRng, limbs, multiplication

    n, generated = modulus(eng, key_length, keys_file)
    sh = multiplication.shape(n)
    ln, limbs2 = sh["limbs_n"], sh["limbs2"]
    ctx = multiplication.context(n, b"probe")
    rng = DeviceRng()
    sync = eng.synchronize
    n2 = n * n

    def wide():
        return rng.rows_t(eng, count, sh["draw_bits"], limbs2)

    def encrypt(m_t, r_wide_t):
        return eng.mulmod_t(eng.powmod_nsquare_t(r_wide_t, n, n), eng._one_plus_mn_t(m_t, n), n2)

    a_t, b_t = eng._reduce_wide_t(wide(), n), eng._reduce_wide_t(wide(), n)
    ra_wide_t = wide()
    ra_t, gamma_t = eng._reduce_wide_t(ra_wide_t, n), eng._reduce_wide_t(wide(), n)
    ca_t, cb_t = encrypt(a_t, ra_wide_t), encrypt(b_t, wide())

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return out, (time.perf_counter() - t0) * 1e3

    def prove(st=None):
        return eng.mul_prove_t(ca_t, cb_t, a_t, ra_t, gamma_t, n, ctx, rng=rng, _stages=st)

    proof = prove()                                                      # warm-up: plans, workspaces
    assert bool(eng.mul_verify_t(ca_t, cb_t, *proof, n, ctx).all())
    rows = {name: [] for name in ("encrypt_ms", "prove_ms", "verify_ms", "response_device_ms", "response_host_ms")}
    prove_stages, verify_stages = [], []
    x_t, e_t = eng._reduce_wide_t(wide(), n), rng.rows_t(eng, count, 128)

    def device_response():
        return eng.response_mod_rows_t(x_t, e_t, a_t, n)[:2]

    def host_response():
        xs, es, as_ = (limbs.unpack(eng.to_host(t)) for t in (x_t, e_t, a_t))
        pairs = [divmod(x + e * a, n) for x, e, a in zip(xs, es, as_)]
        return eng.to_device(limbs.pack([w for _, w in pairs], ln)), eng.to_device(limbs.pack([t for t, _ in pairs], 4))

    device_response()
    for _ in range(repeats):
        _, ms = timed(lambda: encrypt(a_t, wide()))
        rows["encrypt_ms"].append(ms)
        st = []
        proof, ms = timed(lambda: prove(st))
        rows["prove_ms"].append(ms)
        prove_stages.append(stage_ms(st))
        st = []
        verdict, ms = timed(lambda: eng.mul_verify_t(ca_t, cb_t, *proof, n, ctx, _stages=st))
        assert bool(verdict.all())
        rows["verify_ms"].append(ms)
        verify_stages.append(stage_ms(st))
        new, ms = timed(device_response)
        rows["response_device_ms"].append(ms)
        old, ms = timed(host_response)
        rows["response_host_ms"].append(ms)
        assert all(torch.equal(x.view(count, -1), y.view(count, -1)) for x, y in zip(new, old))
    out = {"key_length": key_length, "count": count, "repeats": repeats, "generated_key": generated}
    out.update({name: spread(v) for name, v in rows.items()})
    out["prove_over_encrypt"] = spread([p / d for p, d in zip(rows["prove_ms"], rows["encrypt_ms"])])
    out["verify_over_encrypt"] = spread([p / d for p, d in zip(rows["verify_ms"], rows["encrypt_ms"])])
    out["prove_stages_ms"] = {name: spread([s[name] for s in prove_stages]) for name in prove_stages[0]}
    out["verify_stages_ms"] = {name: spread([s[name] for s in verify_stages]) for name in verify_stages[0]}
    dev, host = out["response_device_ms"], out["response_host_ms"]
    out["kernel_pays_in_time"] = bool(host["median"] - dev["median"] > max(dev["max"] - dev["min"], host["max"] - host["min"]))
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--key-lengths", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--count", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--keys-file", default=str(ROOT / "tests" / "golden" / "threshold_keys.json"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mul_probe.json"))
    args = ap.parse_args()
    import torch

    from protocols.distributed_keygen_amd import Engine

    eng = Engine(0)
    result = {"device": torch.cuda.get_device_name(0), "runs": []}
    for kl in args.key_lengths:
        result["runs"].append(probe(eng, kl, args.count, args.repeats, args.keys_file))
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
        print(json.dumps(result["runs"][-1]), flush=True)


if __name__ == "__main__":
    main()
