#!/usr/bin/env python3
"""Ballots that prove their validity: one-hot slot-packed votes with membership proofs, a double vote refused and named,
the rest summed, threshold-decrypted by a dealt key and decoded into the tally.

A dealer shares a Paillier key among three parties so that any two decrypt (threshold.deal).  A vote for choice j of k is
the plaintext 2^(b j) — 1 in slot j of the slot layout, 0 elsewhere (slots.one_hot_values) —, so the sum of the
ciphertexts decrypts to a plaintext whose slots are the tally.  Every polling station sends its ballots with a proof per
ballot that it holds ONE of those k values (membership.py: csrc/mx_member.hpp for the challenge arithmetic, the engine's
r^N route, its multi-exponentiation modulo N^2, its hash and its inverse for the rest) — without saying which.  One
station slips in a ballot holding two votes: it cannot make a proof for it, its row fails, the receiver names it, and
the homomorphic sum runs over the ballots that passed.  Without the proofs the double vote would have entered the tally
without an error anywhere.
   python examples/verified_ballots.py [--key-length 2048] [--stations 4] [--ballots 25] [--choices 5] [--slot-bits 16]
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
    ap.add_argument("--stations", type=int, default=4)
    ap.add_argument("--ballots", type=int, default=25)
    ap.add_argument("--choices", type=int, default=5)
    ap.add_argument("--slot-bits", type=int, default=16)
    args = ap.parse_args()
    from protocols.distributed_keygen_amd import DeviceRng, Engine, PaillierPrivateKey, homomorphic, limbs, membership, slots, threshold

    if args.stations < 2 or args.ballots < 3 or args.stations * args.ballots >> args.slot_bits:
        raise SystemExit("at least two stations of three ballots, and fewer ballots than a slot counts, expected")
    eng = Engine()
    rng = DeviceRng()
    key = PaillierPrivateKey.generate(args.key_length, rng=rng, engine=eng, safe=True)
    public, shares = threshold.deal(key, parties=3, threshold=1, engine=eng)
    n = public.n
    del key                                                                           # from here on nobody holds p and q
    values = slots.one_hot_values(n, args.slot_bits, args.choices)                    # the public list: 2^(b j) for every choice j

    host = random.Random(1)
    received = {}
    t0 = time.perf_counter()
    for station in range(args.stations):
        label = b"station %d / election 1" % station
        votes = [host.randrange(args.choices) for _ in range(args.ballots)]
        cts, proofs = membership.encrypt_with_proof(n, values, [values[v] for v in votes], label, engine=eng)
        received[station] = (label, votes, cts, proofs.to_ints())
    t1 = time.perf_counter()
    # station 1 replaces its third ballot by one that holds two votes; it has no proof for it and sends the old one
    label, votes, cts, ints = received[1]
    cts[2] = eng.encrypt_fresh_batch([values[0] + values[args.choices - 1]], n, rng)[0]

    kept, tally, refused = [], [0] * args.choices, []
    t2 = time.perf_counter()
    for station, (label, votes, cts, ints) in received.items():
        proofs = membership.MembershipProofs.from_ints(*ints, n, args.choices)
        for r, ok in enumerate(membership.verify_batch(n, values, cts, proofs, label, engine=eng)):
            if ok:
                kept.append(cts[r])
                tally[votes[r]] += 1
            else:
                refused.append((station, r))
    t3 = time.perf_counter()
    assert refused == [(1, 2)]
    (summed,) = homomorphic.sum_groups([kept], n=n, engine=eng)
    sent = {s.index: s.partial_decrypt_batch([summed], prove=True) for s in shares}   # (partials, DecryptionProofs) per party
    plain, cheaters = public.decrypt_verified([summed], sent)
    assert cheaters == []
    rows_t = eng.to_device(limbs.pack_reduced(plain, limbs.limbs_for(n), n))
    counted = slots.decode_t(rows_t, n, args.slot_bits, args.choices, signed=False, engine=eng).tolist()
    assert counted == tally and sum(counted) == len(kept) == args.stations * args.ballots - 1
    print(f"key_length {args.key_length}, {args.stations} stations x {args.ballots} ballots over {args.choices} choices: "
          f"encrypting with proofs {1e3 * (t1 - t0):.0f} ms, verifying {1e3 * (t3 - t2):.0f} ms; ballot {refused[0]} refused (two votes), "
          f"the other {len(kept)} tally to {counted}")


if __name__ == "__main__":
    main()
