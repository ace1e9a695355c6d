#!/usr/bin/env python3
"""A key of two safe primes made on the GPU: generate(safe=True) -> check_primes(safe=True) -> encrypt -> decrypt -> compare.

Threshold Paillier with a dealer and the auxiliary moduli of range proofs want p = 2 p' + 1 and q = 2 q' + 1 with p', q'
prime.  Such primes are rare — one odd candidate in about 190 000 at 1024 bits — so the search draws halves p' in large
batches, drops those where a small prime divides p' or 2 p' + 1 in ONE pass (csrc/mx_sieve.hpp: sieve_kernel<true>), runs the
base 2 on p' and on p, and 64 random bases on p' alone (Pocklington: with p' prime, the base 2 proves p).
   python examples/safe_prime_key.py [--key-length 2048] [--messages 1000]
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
    ap.add_argument("--messages", type=int, default=1000)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import DeviceRng, Engine, PaillierPrivateKey

    eng = Engine()
    rng = DeviceRng()
    t0 = time.perf_counter()
    key = PaillierPrivateKey.generate(args.key_length, rng=rng, engine=eng, safe=True)
    t1 = time.perf_counter()
    assert key.n.bit_length() == args.key_length and key.p % 4 == key.q % 4 == 3
    assert key.check_primes(rng=rng, safe=True)
    ordinary = PaillierPrivateKey.generate(args.key_length, rng=rng, engine=eng)
    assert ordinary.check_primes(rng=rng) and not ordinary.check_primes(rng=rng, safe=True)      # all but certainly
    host = random.Random(1)
    msgs = [host.randrange(-(1 << 40), 1 << 40) for _ in range(args.messages)]
    assert key.decrypt_batch(key.encrypt_batch(msgs, rng=rng), signed=True) == msgs
    print(f"key_length {args.key_length}: a key of two safe primes in {1e3 * (t1 - t0):.0f} ms; "
          f"{args.messages} messages round-trip under it")


if __name__ == "__main__":
    main()
