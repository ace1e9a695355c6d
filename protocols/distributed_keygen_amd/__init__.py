"""MI355X-native engine for the compute hot path of TNO-MPC/protocols.distributed_keygen.

Batched modular exponentiation (biprimality-test v-values, partial decryptions), small-prime
sieve, share recombination and biprimality verdict as hand-written HIP kernels for gfx950 behind
a C ABI (include/mxpaillier.h), with a Python layer that mirrors the reference's operator
surface.  See DESIGN.md and INTEGRATION.md.
"""

import os as _os


def configure_hw_queues(queues: int = 16) -> bool:
    """Opt-in process set-up for callers that keep several launches of this engine in flight (bench.py
    calls it; importing the package does NOT).  The HIP runtime multiplexes streams onto 4 hardware queues
    by default and two streams that share a queue serialise their kernels; a launch of this engine occupies
    the GPU for tens of milliseconds, so a collision between two of the streams that are meant to fill the
    machine together costs 25-40 % (profiles/r02_hw_queue_collisions.txt).  ``GPU_MAX_HW_QUEUES`` is read
    once, when the runtime initialises.  The decision is the native library's (``mx_configure_hw_queues``,
    include/mxpaillier.h): the request, clamped to 1..32, is written when the variable is unset, unreadable or
    SMALLER than the request — an inherited 4 no longer undercuts a caller that asked for 16 —, a larger
    inherited value stays, and ``MX_HW_QUEUES_KEEP=1`` in the environment is the opt-out of a user who really
    wants fewer queues (nothing is changed).  Returns True if the process has not touched the GPU yet, False —
    without changing anything — if it is too late.  Either way ``Engine`` measures what it actually got
    (``Engine.stream_concurrency``) and cuts long batches into no more chunks than run concurrently.
    Unlike the dictionary write it used to be, the call loads the native library and with it torch (some hundred
    milliseconds, no GPU call) — after making sure that the library is built from the sources as they are
    (``build.ensure_built``: a missing or stale library is compiled first, by one process if several ask at once), so
    that it is never the call that pins an outdated library in the process."""
    import sys

    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        return False
    from . import _lib, build

    build.ensure_built()                                      # before the first load (callers' own build steps come later)
    now = _lib.lib().mx_configure_hw_queues(int(queues))      # loading the library makes no GPU call
    if now < 0:                                               # MX_ERR_STATE: the library itself has used the GPU already
        return False
    # the library wrote the C environment; os.environ is Python's copy of it (what later readers here and
    # subprocess calls with an explicit env= see)
    mine = _os.environ.get("GPU_MAX_HW_QUEUES", "").strip()
    if now > 0 and not (mine.isdigit() and int(mine) == now):
        _os.environ["GPU_MAX_HW_QUEUES"] = str(now)
    return True


from . import device_rng, homomorphic, limbs, membership, multiplication, packing, primes, randomizer, range_proof, secure_product, slots, threshold  # noqa: F401
from .device_rng import DeviceRng  # noqa: F401
from .engine import Engine, default_engine  # noqa: F401
from .membership import MembershipProofs  # noqa: F401
from .multiplication import MultiplicationProofs  # noqa: F401
from .primes import is_probable_prime_batch, random_primes  # noqa: F401
from .private_key import PaillierPrivateKey  # noqa: F401
from .randomizer import FastRandomizer, generate_base  # noqa: F401
from .range_proof import RangeParameters, RangeProofs  # noqa: F401
from .threshold import DecryptionProofs, ThresholdKeyShare, ThresholdPublicKey  # noqa: F401
from .operators import mod_inv, mod_inv_batch, pow_mod, pow_mod_batch, pow_mod_batch_multi  # noqa: F401

__version__ = "0.1.0"
