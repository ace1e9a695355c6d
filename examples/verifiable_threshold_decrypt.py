#!/usr/bin/env python3
"""Threshold decryption where a cheater is caught: deal -> encrypt -> partial decryptions with proofs -> verify -> combine.

A dealer makes a key of two safe primes on the GPU and shares it among five parties so that any three decrypt
(threshold.deal: Damgård–Jurik / Shoup).  Every party sends c_i = c^(2 x_i) with a proof that it used its dealt share
(csrc/mx_sha256.hpp: the challenges, csrc/mx_response.hpp: the responses; everything else is the engine's modexps, its
multi-exponentiation and its fixed-base tables).  Party 3 spoils one of its partial decryptions: its proof for that row
fails, decrypt_verified names it and decrypts from the others; without the proofs the combination would only have
reported that SOMETHING is wrong.
   python examples/verifiable_threshold_decrypt.py [--key-length 2048] [--messages 100]
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
    ap.add_argument("--messages", type=int, default=100)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import DeviceRng, Engine, PaillierPrivateKey, threshold

    eng = Engine()
    rng = DeviceRng()
    key = PaillierPrivateKey.generate(args.key_length, rng=rng, engine=eng, safe=True)
    public, shares = threshold.deal(key, parties=5, threshold=2, engine=eng)          # vets the primes, then shares the key
    host = random.Random(1)
    msgs = [host.randrange(1 << 40) for _ in range(args.messages)]
    cts = key.encrypt_batch(msgs, rng=rng)
    del key                                                                           # from here on nobody holds p and q

    t0 = time.perf_counter()
    sent = {s.index: s.partial_decrypt_batch(cts, prove=True) for s in shares}        # (partials, DecryptionProofs) per party
    t1 = time.perf_counter()
    partials, proofs = sent[3]
    partials[7 % len(partials)] = partials[7 % len(partials)] * cts[0] % public.n_square      # party 3 cheats in one row
    verdicts = public.verify_batch(3, cts, partials, proofs)
    assert verdicts.count(False) == 1 and not verdicts[7 % len(partials)]
    try:
        public.combine_batch({i: sent[i][0] for i in (1, 2, 3)})                      # without proofs: an error, no culprit
        raise AssertionError("a spoilt partial decryption combined")
    except ValueError as err:
        print(f"combining parties 1, 2, 3 unverified: {str(err)[:58]} ...")
    t2 = time.perf_counter()
    out, cheaters = public.decrypt_verified(cts, sent)
    t3 = time.perf_counter()
    assert out == msgs and cheaters == [3]
    assert public.combine_batch({i: sent[i][0] for i in (2, 4, 5)}) == msgs           # any other three decrypt as well
    print(f"key_length {args.key_length}, {args.messages} ciphertexts: five parties prove in {1e3 * (t1 - t0):.0f} ms, "
          f"verifying all five and combining takes {1e3 * (t3 - t2):.0f} ms; party {cheaters} named, plaintexts from the rest")


if __name__ == "__main__":
    main()
