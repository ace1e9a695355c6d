"""What the tests of patch.install(generator_rng=...) share: an in-memory pool that records every broadcast, three
in-process parties running compute_modulus (the reference's distributed=False shape), and the checks themselves — run on
the stand-in package by tests/test_generators_host.py and on the real reference by
tests/test_patch_reference_generators.py.  Lives in tests/ only."""

from __future__ import annotations

import asyncio
import random
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import generators_model as gm  # noqa: E402

from fake_engine import FakeEngine  # noqa: E402
from generators_engine import GeneratorsEngine  # noqa: E402
from protocols.distributed_keygen_amd import biprime  # noqa: E402
from protocols.distributed_keygen_amd.device_rng import DeviceRng  # noqa: E402

KEY = bytes((5 * k + 9) & 0xFF for k in range(32))
REF = ROOT / "oracle" / "_ref" / "distributed_keygen"
NAMES = ["p1", "p2", "p3"]


class RecordingHub:
    def __init__(self) -> None:
        self.box = {n: {} for n in NAMES}
        self.sent = []                  # (sender, msg_id, message) of every broadcast


class RecordingPool:
    def __init__(self, hub, me) -> None:
        self.hub, self.me = hub, me
        self.pool_handlers = {n: None for n in NAMES if n != me}

    def async_broadcast(self, message, msg_id=None, handler_names=None):
        self.hub.sent.append((self.me, msg_id, message))
        for n in (handler_names if handler_names is not None else self.pool_handlers):
            self.hub.box[n].setdefault(msg_id, []).append((self.me, message))

    def asend(self, party, message, msg_id=None):
        self.hub.box[party].setdefault(msg_id, []).append((self.me, message))

    async def recv_all(self, msg_id=None):
        while len(self.hub.box[self.me].get(msg_id, [])) < len(self.pool_handlers):
            await asyncio.sleep(0)
        return tuple(self.hub.box[self.me].pop(msg_id))


def standin_package():
    """(package name, distributed_keygen module, is it the real reference) of the stand-in"""
    import standin_harness as sh

    return sh.PACKAGE, sh.modules()[1], False


def reference_package():
    """... and of the real reference where build() left it (None otherwise).  Loaded once per process: a second
    load_reference() would put new stand-in classes under the names the loaded reference has bound already."""
    if not REF.exists():
        return None
    import make_golden

    dk = sys.modules.get("tno.mpc.protocols.distributed_keygen.distributed_keygen")
    if dk is None:
        _, dk = make_golden.load_reference()
    return "tno.mpc.protocols.distributed_keygen", dk, True


def _keygen(dk, real, seed, key_length, batch_size, correct_param):
    """Three in-process parties (the reference's distributed=False shape) run compute_modulus; returns (moduli, the
    parties' Shares, the hub with every broadcast)."""
    import secrets as _secrets

    DP = dk.DistributedPaillier
    rnd = random.Random(seed)
    hub = RecordingHub()
    held = {}
    if real:
        saved = (_secrets.randbits, _secrets.randbelow, dk.randint)
        _secrets.randbits = dk.secrets.randbits = rnd.getrandbits
        _secrets.randbelow = lambda n: rnd.randrange(n)
        dk.randint = rnd.randint
    else:
        dk.rng.seed(seed)
    try:
        async def party(i, me):
            pool = RecordingPool(hub, me)
            party_indices = {("self" if n == me else n): k for k, n in enumerate(NAMES, start=1)}
            if real:
                _, prime_length, prime_list, sh_t, sh_2t, shares = DP.setup_input(pool, key_length, 200, 1)
            else:
                prime_length, prime_list, sh_t, sh_2t, _ = DP.setup_input(len(NAMES), key_length, 200, 1)
                shares = dk.Shares()
            held[i] = shares
            return await DP.compute_modulus(shares, i, pool, prime_list, party_indices, prime_length, sh_t, sh_2t, correct_param, 7,
                                            batch_size)

        async def run():
            return await asyncio.gather(*[party(i, me) for i, me in enumerate(NAMES, start=1)])

        return asyncio.run(run()), held, hub
    finally:
        if real:
            _secrets.randbits, _secrets.randbelow, dk.randint = saved
            dk.secrets.randbits = saved[0]


def check_patched_generator_step_is_a_drop_in(package, dk, real):
    """A distributed=False key generation at key_length 128 with ``generator_rng=``: it completes with a biprime every
    party agrees on; the generator messages carry the reference's ids and labels (DK:1035-1049: ``f"{msg_id}_g"``, one
    ``{"label": "biprime", "value": [...]}`` per candidate on the real reference's exchange); one call number per party
    and round; the generators reach the v-calculation as device rows, merged over the co-located parties; and
    ``uninstall()`` restores the original method."""
    import sympy

    from protocols.distributed_keygen_amd import patch

    DP = dk.DistributedPaillier
    name = "_DistributedPaillier__biprime_test_g_generation"
    original = DP.__dict__[name]
    keep, batch = 10, 60
    G = keep * biprime.JACOBI_CORRECTION_FACTOR
    eng, rng = GeneratorsEngine(), DeviceRng(key=KEY, first_call=500)
    patch.install(engine=eng, package=package, generator_rng=rng)
    try:
        assert DP.__dict__[name] is not original and isinstance(DP.__dict__[name], classmethod)
        moduli, held, hub = _keygen(dk, real, 13, 128, batch, keep)
        stats = dict(patch.round_coalescer(package).stats)
    finally:
        patch.uninstall()
    assert DP.__dict__[name] is original

    assert len(set(moduli)) == 1 and 125 <= moduli[0].bit_length() <= 134
    p, q = (sum(getattr(held[i], which).additive for i in held) for which in ("p", "q"))
    assert p * q == moduli[0] and sympy.isprime(p) and sympy.isprime(q)
    g_msgs = [(who, mid, msg) for who, mid, msg in hub.sent if mid.endswith("_g")]
    rounds = sorted({mid for _, mid, _ in g_msgs})
    assert rounds and all(re.fullmatch(r"distributed_keygen_session#7_biprime_test_g_[1-9][0-9]*_g", mid) for mid in rounds)
    assert len(g_msgs) == 3 * len(rounds)                                 # one exchange_reconstruct per party and round
    assert rng.next_call == 500 + len(g_msgs)                            # ... and one call number
    shares_calls = [c for c in eng.gen_calls if c[0] == "shares"]
    assert len(shares_calls) == len(g_msgs) and all(c[2] == G for c in shares_calls)
    for who, mid, msg in g_msgs:
        if real:                                                          # utils.exchange_reconstruct's own message
            assert all(set(m) == {"label", "value"} and m["label"] == "biprime" and len(m["value"]) == G for m in msg)
            lists = [m["value"] for m in msg]
        else:
            lists = msg["value"]
            assert msg["content"] == "shares" and all(len(row) == G for row in lists)
        assert all(type(s) is int and s >= 0 for row in lists for s in row)
    # the three parties' own rows were taken from the device, the sums left rows there, and their v-calculations merged
    assert sum(1 for c in eng.gen_calls if c[0] == "own_share_rows_from_device") == len(g_msgs)
    assert sum(1 for c in eng.gen_calls if c[0] == "sum") == len(g_msgs)
    assert stats["v_requests"] == 3 * stats["v_launches"] == sum(3 for c in eng.gen_calls if c[0] == "v_from_generator_rows")


def check_the_rebound_method_keeps_the_references_signature_and_return_type(package, dk, real):
    import inspect

    from protocols.distributed_keygen_amd import patch

    DP = dk.DistributedPaillier
    name = "_DistributedPaillier__biprime_test_g_generation"
    original = DP.__dict__[name]
    eng, rng = GeneratorsEngine(), DeviceRng(key=KEY, first_call=0)
    mods = [1000003, (1 << 61) - 1]
    patch.install(engine=eng, package=package, generator_rng=rng)
    try:
        rebound = DP.__dict__[name]
        assert list(inspect.signature(rebound.__func__).parameters) == list(inspect.signature(original.__func__).parameters)
        assert inspect.iscoroutinefunction(rebound.__func__)
        hub = RecordingHub()

        async def party(i, me):
            pool = RecordingPool(hub, me)
            party_indices = {("self" if n == me else n): k for k, n in enumerate(NAMES, start=1)}
            return await getattr(DP, name)(3, i, mods, party_indices, pool, "sid_biprime_test_g_1")

        async def run():
            return await asyncio.gather(*[party(i, me) for i, me in enumerate(NAMES, start=1)])

        got = asyncio.run(run())
    finally:
        patch.uninstall()
    assert DP.__dict__[name] is original
    G = 3 * biprime.JACOBI_CORRECTION_FACTOR
    table = {i: gm.shares(KEY, i - 1, mods, G) for i in (1, 2, 3)}
    assert got[0] == got[1] == got[2] == gm.generators(table, mods, G)
    assert all(type(g) is int for row in got[0] for g in row) and {mid for _, mid, _ in hub.sent} == {"sid_biprime_test_g_1_g"}


def check_install_without_generator_rng_leaves_the_method_alone(package, dk, real):
    from protocols.distributed_keygen_amd import patch

    name = "_DistributedPaillier__biprime_test_g_generation"
    original = dk.DistributedPaillier.__dict__[name]
    patch.install(engine=FakeEngine(), package=package)
    try:
        assert dk.DistributedPaillier.__dict__[name] is original
    finally:
        patch.uninstall()
