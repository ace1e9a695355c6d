#!/usr/bin/env python3
"""The variance of encrypted values: nobody sees a value, the parties of a dealt threshold key learn only sum x and
sum x^2.

A dealer shares a Paillier key among three parties so that any two decrypt (threshold.deal).  Every value arrives as a
ciphertext.  Paillier adds under encryption but does not multiply two ciphertexts, so the squares come from the protocol
of Cramer-Damgard-Nielsen (secure_product.square): every party blinds the ciphertext with a mask of its own and publishes
Enc(d_i) and Enc(d_i x) with a proof of correct multiplication (multiplication.py: csrc/mx_response_mod.hpp for the
response modulo N and its quotient, the engine's r^N route, its multi-exponentiation modulo N^2 and its hash for the
rest); the blinded value x + sum d_i is opened with verified partial decryptions, and Enc(x^2) = Enc(x)^(x + sum d_i) /
prod Enc(d_i x).  Then sum x and sum x^2 are two homomorphic sums and one verified threshold decryption, and
the variance is sum x^2 / n - (sum x / n)^2 on the two opened numbers.
   python examples/encrypted_variance.py [--key-length 2048] [--values 32] [--bits 16]
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
    ap.add_argument("--values", type=int, default=32)
    ap.add_argument("--bits", type=int, default=16)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import DeviceRng, Engine, PaillierPrivateKey, homomorphic, secure_product, threshold

    if args.values < 2 or not 1 <= args.bits <= 64:
        raise SystemExit("at least two values of 1 .. 64 bits expected")
    eng = Engine()
    rng = DeviceRng()
    key = PaillierPrivateKey.generate(args.key_length, rng=rng, engine=eng, safe=True)
    public, shares = threshold.deal(key, parties=3, threshold=1, engine=eng)
    n = public.n
    del key                                                                           # from here on nobody holds p and q

    host = random.Random(1)
    xs = [host.getrandbits(args.bits) for _ in range(args.values)]
    cts = eng.encrypt_fresh_batch(xs, n, rng)                                         # what the owners of the values send
    t0 = time.perf_counter()
    squares, cheaters = secure_product.square(public, shares, cts, b"variance / batch 1", rng=rng, engine=eng)
    t1 = time.perf_counter()
    assert cheaters == []
    sums = homomorphic.sum_groups([cts, squares], n=n, engine=eng)                     # Enc(sum x), Enc(sum x^2)
    sent = {s.index: s.partial_decrypt_batch(sums, prove=True) for s in shares}
    (s1, s2), cheaters = public.decrypt_verified(sums, sent)
    t2 = time.perf_counter()
    assert cheaters == [] and (s1, s2) == (sum(xs), sum(x * x for x in xs))
    count = len(xs)
    variance = s2 / count - (s1 / count) ** 2
    plain = sum((x - sum(xs) / count) ** 2 for x in xs) / count
    assert abs(variance - plain) <= 1e-9 * max(1.0, plain)
    print(f"key_length {args.key_length}, {count} encrypted values of {args.bits} bits, 3 parties: squaring under encryption "
          f"{1e3 * (t1 - t0):.0f} ms, sums and verified decryption {1e3 * (t2 - t1):.0f} ms; sum x = {s1}, sum x^2 = {s2}, "
          f"variance {variance:.3f} (plaintext {plain:.3f})")


if __name__ == "__main__":
    main()
