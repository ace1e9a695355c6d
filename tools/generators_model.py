#!/usr/bin/env python3
"""Model of the generator kernels (csrc/mx_generators.hpp) and of the layers above them — developer tool and test
vehicle.  Pure Python: random rows come from tools/chacha_model.py, reductions are ``%`` on Python ints.

The definitions (what the kernels, ``Engine.generator_shares_t`` / ``generator_sum_t`` and ``biprime.BiprimeRound`` must
reproduce bit for bit), for the survivors c = 0 .. S-1 with moduli N_c and G generators each:

    B, cw                   B = max_c bits(N_c); a draw has B + 64 bits in cw = ceil((B + 64) / 32) words
    own share               s[c G + k] = D[c G + k] mod N_c        D: the rows of ONE ``rng.rows_t(S G, B + 64, cw)``
    generator               g[c G + k] = (sum_j share_j[c G + k]) mod N_c        canonical residue, any integer share

Row c G + k belongs to generator k of survivor c.  A draw-then-reduce share is uniform on [0, N_c) up to a bias below
2^-64; the reference draws ``randint(0, N_c)`` on [0, N_c] inclusive (DK:1042) — only the sum modulo N_c is ever used, so
parties on either path interoperate.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import chacha_model


def draw_bits(moduli: Sequence[int]) -> int:
    """B + 64 for the widest of `moduli`."""
    return max(int(n).bit_length() for n in moduli) + 64


def draw_words(moduli: Sequence[int]) -> int:
    return -(-draw_bits(moduli) // 32)


def shares_of_draws(draws: Sequence[int], moduli: Sequence[int], G: int) -> List[List[int]]:
    """One list of G shares per modulus from the S * G draws, row c * G + k first by c."""
    if len(draws) != len(moduli) * G:
        raise ValueError("one draw per generator of every modulus expected")
    return [[draws[c * G + k] % n for k in range(G)] for c, n in enumerate(moduli)]


def device_draws(key: bytes, call: int, moduli: Sequence[int], G: int) -> List[int]:
    """The S * G draws of the one rows call a device-drawn step makes (call number `call` of `key`)."""
    count = len(moduli) * G
    return chacha_model.row_ints(key, call, count, draw_bits(moduli), draw_words(moduli)) if count else []


def shares(key: bytes, call: int, moduli: Sequence[int], G: int) -> List[List[int]]:
    """``BiprimeRound.draw_generator_shares`` for ``DeviceRng(key, call)``: nested per candidate."""
    return shares_of_draws(device_draws(key, call, moduli, G), moduli, G)


def generators(shares_by_party: Dict[int, Sequence[Sequence[int]]], moduli: Sequence[int], G: int) -> List[List[int]]:
    """The reference's ``sum(shares) % N`` (utils.py: AdditiveVariable.reconstruct) for every generator."""
    for lists in shares_by_party.values():
        if len(lists) != len(moduli) or any(len(row) != G for row in lists):
            raise ValueError("every party needs G shares per modulus")
    return [[sum(int(lists[c][k]) for lists in shares_by_party.values()) % n for k in range(G)] for c, n in enumerate(moduli)]


if __name__ == "__main__":
    mods = [(1 << 61) - 1, 1000003]
    mine = shares(bytes(range(32)), 0, mods, 2)
    print(mine, generators({1: mine, 2: [[5, mods[0]], [mods[1] + 7, 0]]}, mods, 2))
