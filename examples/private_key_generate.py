#!/usr/bin/env python3
"""A private key made on the GPU: generate -> check_primes -> encrypt -> decrypt -> compare.

PaillierPrivateKey.generate draws candidates of key_length / 2 bits on the device, sieves them, runs the strong-pseudoprime
test to the base 2 on the survivors (csrc/mx_mr.hpp: mr_base2_kernel) and 64 random bases on what is left, and builds the
key from the first two primes; generate_batch makes one key per client from ONE search.  No other library is involved:
the primes are found, vetted (check_primes, as for a key received from elsewhere) and used by the engine alone.
   python examples/private_key_generate.py [--key-length 2048] [--clients 8] [--messages 1000]
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
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--messages", type=int, default=1000)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import DeviceRng, Engine, PaillierPrivateKey

    eng = Engine()
    rng = DeviceRng()
    t0 = time.perf_counter()
    key = PaillierPrivateKey.generate(args.key_length, rng=rng, engine=eng)
    t1 = time.perf_counter()
    assert key.n.bit_length() == args.key_length and key.p.bit_length() == key.q.bit_length() == args.key_length // 2
    assert key.check_primes(rng=rng)
    host = random.Random(1)
    msgs = [host.randrange(-(1 << 40), 1 << 40) for _ in range(args.messages)]
    assert key.decrypt_batch(key.encrypt_batch(msgs, rng=rng), signed=True) == msgs
    t2 = time.perf_counter()
    keys = PaillierPrivateKey.generate_batch(args.clients, args.key_length, rng=rng, engine=eng)
    t3 = time.perf_counter()
    assert len({k.n for k in keys}) == args.clients
    for k in keys:
        assert k.decrypt(k.encrypt(42, rng=rng)) == 42
    print(f"key_length {args.key_length}: one key in {1e3 * (t1 - t0):.0f} ms, {args.clients} keys from one search in "
          f"{1e3 * (t3 - t2):.0f} ms; {args.messages} messages round-trip under the generated key")


if __name__ == "__main__":
    main()
