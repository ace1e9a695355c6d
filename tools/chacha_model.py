#!/usr/bin/env python3
"""Bit-exact model of the device random-row generator (csrc/mx_chacha.hpp) — developer tool and test vehicle.

ChaCha20 as RFC 8439 specifies it: a state of sixteen 32-bit words — four constants, eight key words, a 32-bit block
counter in word 12 and a 96-bit nonce in words 13-15 —, twenty rounds (ten column / diagonal double rounds), then the
feed-forward addition of the input state; the sixteen output words are keystream words 0 .. 15 of the block, in state
order (serialised little-endian they are the 64 keystream bytes of the RFC).

The mapping of keystream words to rows is part of the kernel's contract and the same for every launch shape:

    w = ceil(bits / 32)
    keystream word i = r * w + j  ->  out[r][j]  for j < w;  it is word i mod 16 of block counter0 + i div 16
    the top word of a row is masked to bits mod 32 bits when that is not 0
    words w .. row_words - 1 of a row are 0
    the unused tail of the last block is discarded

``rows(key, call, ...)`` is what ``DeviceRng.rows_t`` returns for call number ``call``: the call number is the nonce
(96 bits, little-endian in words 13-15) and the block counter starts at 0.  tests/test_device_rng_host.py checks the block
function against the RFC's vector, tests/test_gpu_device_rng.py the kernel against this file.
"""
from __future__ import annotations

import struct
from typing import List, Sequence

CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)      # "expand 32-byte k"
M32 = 0xFFFFFFFF


def _rotl(x: int, n: int) -> int:
    return ((x << n) & M32) | (x >> (32 - n))


def _quarter(x: List[int], a: int, b: int, c: int, d: int) -> None:
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)


def key_words(key: bytes) -> List[int]:
    """The eight little-endian key words of a 32-byte key."""
    if len(key) != 32:
        raise ValueError("a ChaCha20 key has 32 bytes")
    return list(struct.unpack("<8I", key))


def nonce_words(call: int) -> List[int]:
    """A 96-bit call number as the nonce: little-endian in words 13-15."""
    if not 0 <= call < 1 << 96:
        raise ValueError("the call number must lie in [0, 2^96)")
    return [(call >> (32 * k)) & M32 for k in range(3)]


def block(key: Sequence[int], counter: int, nonce: Sequence[int]) -> List[int]:
    """The sixteen output words of one block (key: 8 words, nonce: 3 words)."""
    state = [*CONSTANTS, *key, counter & M32, *nonce]
    x = list(state)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(x, state)]


def block_bytes(key: bytes, counter: int, nonce: bytes) -> bytes:
    """The 64 keystream bytes of one block from the RFC's byte strings (key 32 bytes, nonce 12 bytes)."""
    return struct.pack("<16I", *block(key_words(key), counter, struct.unpack("<3I", nonce)))


def rows_words(key: Sequence[int], nonce: Sequence[int], counter0: int, count: int, bits: int, row_words: int) -> List[List[int]]:
    """out[count][row_words] of the kernel for these key / nonce words and first block counter."""
    w = -(-bits // 32)
    if count < 0 or bits < 1 or w > row_words:
        raise ValueError("count >= 0 and 1 <= bits <= 32 * row_words expected")
    total = count * w
    if counter0 + -(-total // 16) > 1 << 32:
        raise ValueError("the request does not fit the 32-bit block counter")
    stream: List[int] = []
    for b in range(-(-total // 16)):
        stream.extend(block(key, counter0 + b, nonce))
    top = (1 << (bits % 32)) - 1 if bits % 32 else M32
    out = []
    for r in range(count):
        row = stream[r * w : (r + 1) * w]
        row[w - 1] &= top
        out.append(row + [0] * (row_words - w))
    return out


def rows(key: bytes, call: int, count: int, bits: int, row_words: int = 0) -> List[List[int]]:
    """The rows of ``DeviceRng(key, first_call=call).rows_t(engine, count, bits, row_words)``; row_words 0 = ceil(bits / 32)."""
    return rows_words(key_words(key), nonce_words(call), 0, count, bits, row_words or -(-bits // 32))


def row_ints(key: bytes, call: int, count: int, bits: int, row_words: int = 0) -> List[int]:
    """The same rows as integers (little-endian words)."""
    return [sum(v << (32 * j) for j, v in enumerate(row)) for row in rows(key, call, count, bits, row_words)]


if __name__ == "__main__":
    rfc = block_bytes(bytes(range(32)), 1, bytes.fromhex("000000090000004a00000000"))
    print(rfc.hex())
