#!/usr/bin/env python3
"""Inputs that prove their size: senders encrypt with range proofs, the receiver verifies, drops the bad row, sums the rest.

The receiver holds a Paillier key and makes the auxiliary parameters (Nh, s, t) of the proofs — two more safe primes it
keeps to itself — with a proof that s lies in the group of t, which every sender checks first.  Each sender encrypts its
values under the receiver's key with a proof that every one of them has at most `--bits` bits (range_proof.py:
csrc/mx_multiexp.hpp for the products modulo Nh and N, csrc/mx_response.hpp for the responses, the engine's r^N route and
its multi-exponentiation modulo N^2 for the rest).  One sender smuggles in a value 2^400 too large: its row fails, the
receiver names it, and the homomorphic sum runs over the rows that passed — without the proofs that value would have
corrupted the total without an error.
   python examples/range_proved_inputs.py [--key-length 2048] [--aux-length 1024] [--senders 4] [--values 25] [--bits 40]
"""
import argparse
import random
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-length", type=int, default=2048)
    ap.add_argument("--aux-length", type=int, default=1024)
    ap.add_argument("--senders", type=int, default=4)
    ap.add_argument("--values", type=int, default=25)
    ap.add_argument("--bits", type=int, default=40)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import DeviceRng, Engine, PaillierPrivateKey, RangeParameters, homomorphic, range_proof

    eng = Engine()
    rng = DeviceRng()
    key = PaillierPrivateKey.generate(args.key_length, rng=rng, engine=eng)
    n = key.n
    params, secret = RangeParameters.generate(args.aux_length, engine=eng, rng=rng)   # the receiver's; `secret` never leaves it
    sent_params = (params.to_ints(), params.prove_parameters(secret))

    host = random.Random(1)
    received = {}
    t0 = time.perf_counter()
    for sender in range(args.senders):
        theirs = RangeParameters.from_ints(*sent_params[0])
        assert theirs.verify_parameters(sent_params[1])                               # or the proofs might leak the values
        label = b"sender %d / round 1" % sender
        values = [host.randrange(1 << args.bits) for _ in range(args.values)]
        cts, proofs = range_proof.encrypt_with_proof(n, theirs, args.bits, values, label, engine=eng)
        received[sender] = (label, values, cts, proofs.to_ints())
    t1 = time.perf_counter()
    # sender 1 replaces its third ciphertext by one of a value far out of range; it cannot make a proof for it
    label, values, cts, ints = received[1]
    huge = values[2] + (1 << 400)
    cts[2] = eng.encrypt_fresh_batch([huge], n, rng)[0]

    kept, total, dropped = [], 0, []
    t2 = time.perf_counter()
    for sender, (label, values, cts, ints) in received.items():
        proofs = range_proof.RangeProofs.from_ints(*ints, n, params, args.bits)
        for k, ok in enumerate(range_proof.verify_batch(n, params, args.bits, cts, proofs, label, engine=eng)):
            if ok:
                kept.append(cts[k])
                total += values[k]
            else:
                dropped.append((sender, k))
    t3 = time.perf_counter()
    assert dropped == [(1, 2)]
    (summed,) = homomorphic.sum_groups([kept], n=n, engine=eng)
    assert key.decrypt_batch([summed]) == [total]
    print(f"key_length {args.key_length}, Nh of {args.aux_length} bits, {args.senders} senders x {args.values} values of {args.bits} bits: "
          f"encrypting with proofs {1e3 * (t1 - t0):.0f} ms, verifying {1e3 * (t3 - t2):.0f} ms; row {dropped[0]} refused, "
          f"the sum of the other {len(kept)} decrypts to {total}")


if __name__ == "__main__":
    main()
