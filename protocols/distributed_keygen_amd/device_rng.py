"""Random rows drawn on the device: exponents of the fixed-base randomiser and the randomness r of r^N without a host
draw and an upload.

What this is — read before use:

  * ChaCha20 (RFC 8439) as a DETERMINISTIC EXPANSION of a 256-bit seed from the operating system (``os.urandom``).  The
    kernel (csrc/mx_chacha.hpp) writes the keystream as limb rows on the device; tools/chacha_model.py is its bit-exact
    model.  Nothing else is random here: who knows the key knows every row this object ever produced or will produce.
  * The key is visible to whoever can read this process's memory or its kernel arguments — the same exposure as the
    exponents themselves, which are uploaded from this process's memory today.
  * Every call takes the next value of a 96-bit call counter as the nonce and starts the 32-bit block counter at 0, so a
    (key, nonce, block) triple is never used twice: not across calls, not across threads (the counter is taken under a
    lock), not across objects (different keys).  A forked child gets a new key and a new lock for every live object
    at the fork itself (``os.register_at_fork``), whatever a thread of the parent held at that moment; the process id
    is checked again in every call for a child made in a way that skips those hooks.
  * There is no reseeding and no backtracking resistance beyond the per-call nonce: the key lives as long as the
    object, and reading it later reveals earlier rows.
  * Opt-in.  Nothing in the package uses it unless a caller passes a ``DeviceRng`` (or ``device_rng=True`` to
    ``randomizer.FastRandomizer``); the host draw with ``os.urandom`` stays the default.
"""

from __future__ import annotations

import os
import struct
import threading
import weakref
from typing import Any, Optional, Tuple

MAX_BLOCKS = 1 << 32          # blocks one call can address: the block counter has 32 bits and starts at 0
MAX_CALLS = 1 << 96           # the nonce

_live: "weakref.WeakSet[DeviceRng]" = weakref.WeakSet()


def _rekey_in_child() -> None:
    """In a forked child: every generator gets a key of its own and a fresh lock — the inherited one may have been held
    by a thread of the parent that does not exist here.  The call counter is kept; the key is what separates the
    streams."""
    for rng in list(_live):
        rng._lock = threading.Lock()
        rng._key_words = struct.unpack("<8I", os.urandom(32))
        rng._pid = os.getpid()


if hasattr(os, "register_at_fork"):
    os.register_at_fork(after_in_child=_rekey_in_child)


class DeviceRng:
    """A keyed ChaCha20 stream whose rows are produced on the device (module docstring: what that means).

    ``key``: 32 bytes, ``os.urandom(32)`` by default; ``first_call``: the first value of the call counter.  Injecting
    either is for tests and makes the output deterministic: call number c of key K gives
    ``tools/chacha_model.rows(K, c, count, bits, row_words)``."""

    def __init__(self, key: Optional[bytes] = None, first_call: int = 0) -> None:
        if key is None:
            key = os.urandom(32)
        key = bytes(key)
        if len(key) != 32:
            raise ValueError("the key must have 32 bytes")
        first_call = int(first_call)
        if not 0 <= first_call < MAX_CALLS:
            raise ValueError("first_call must lie in [0, 2^96)")
        self._key_words: Tuple[int, ...] = struct.unpack("<8I", key)
        self._pid = os.getpid()
        self._next_call = first_call
        self._lock = threading.Lock()
        _live.add(self)

    def __repr__(self) -> str:
        return f"DeviceRng(next_call={self._next_call})"

    @property
    def next_call(self) -> int:
        """The call number the next ``rows_t`` will use."""
        return self._next_call

    def _take(self) -> Tuple[Tuple[int, ...], Tuple[int, int, int]]:
        """(key words, nonce words) of the next call.  In a process other than the one the key was drawn in — a child
        whose fork did not run _rekey_in_child — a new key is drawn first: the child must not repeat its parent's
        stream."""
        with self._lock:
            pid = os.getpid()
            if pid != self._pid:
                self._key_words = struct.unpack("<8I", os.urandom(32))
                self._pid = pid
            call = self._next_call
            if call >= MAX_CALLS:
                raise ValueError("the 96-bit call counter is exhausted")
            self._next_call = call + 1
            return self._key_words, (call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF, call >> 64)

    def rows_t(self, engine: Any, count: int, bits: int, row_words: Optional[int] = None):
        """``count`` rows of ``bits`` random bits each as the int32 device tensor ``[count, row_words]`` the engine's
        ``*_t`` functions take (little-endian words, zero above ``bits``; ``row_words`` defaults to ceil(bits / 32)),
        enqueued on `engine`'s current stream — whatever reads the rows runs on that stream or waits for it.  ValueError — before anything is launched and before a call number is
        taken — for a request of more than 2^32 blocks of 64 bytes."""
        count, bits = int(count), int(bits)
        words = (bits + 31) // 32
        row_words = words if row_words is None else int(row_words)
        if count < 0 or bits < 1 or row_words < words:
            raise ValueError("count >= 0 and 1 <= bits <= 32 * row_words expected")
        if (count * words + 15) // 16 > MAX_BLOCKS:
            raise ValueError("one call draws at most 2^32 blocks of 64 bytes")
        key, nonce = self._take()
        return engine.chacha20_rows_t(key, nonce, 0, count, bits, row_words)
