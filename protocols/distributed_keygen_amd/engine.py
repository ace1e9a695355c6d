"""Batched GPU operators over the C ABI (include/mxpaillier.h).

Two levels:
  * tensor level (``*_t``): operands are device-resident ``torch.int32`` tensors of limb rows
    ``[batch, limbs]`` — what bench.py and the multi-GPU path use;
  * int level: Python ints in / out, mirroring the reference's scalar operators
    (``pow_mod(value, exponent, modulus)`` of tno.mpc.encryption_schemes.utils, bound at
    distributed_keygen.py:35 and paillier_shared_key.py:20) as the batched forms
    ``powmod_batch`` / ``powmod_batch_multi`` / ``sieve_batch`` / ``combine_batch`` /
    ``biprime_verdict_batch``.

PyTorch is used only for device memory and streams.  There is no CPU fallback: constructing an
Engine without a GPU or without the built library raises.
"""

from __future__ import annotations

import ctypes as _ctypes
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, limbs as _limbs
from ._checks import _check_modulus, _check_rows_n2, _int_args, _is_device_rows, _nsquare  # noqa: F401  (tests import them from here)
from .key_flows import PrivateKeyFlows
from .proof_flows import ProofFlows

_INTS = (_ctypes.c_int,) * 5       # out-parameter types of the shape queries (Engine._query), sliced to the count


class _Plan:
    """A per-key plan: the ctypes descriptor, the device block it points to (kept alive here) and the
    event that marks the end of prepare's uploads on the stream they were enqueued on."""

    __slots__ = ("desc", "block", "stream_ptr", "ready")

    def __init__(self, desc, block, stream_ptr, ready) -> None:
        self.desc, self.block, self.stream_ptr, self.ready = desc, block, stream_ptr, ready


class FixedBaseTable(_Plan):
    """Handle of a fixed-base table (Engine.fixed_base_table): the device block of mx_fixedbase_nsquare_prepare with
    what a launch needs to read it.  ``desc`` is the N^2 plan whose constants the table was built with (kept alive here)."""

    __slots__ = ("n", "base", "exp_bits", "window", "windows", "nbytes", "plan")

    def __init__(self, plan, block, stream_ptr, ready, n, base, exp_bits, window, windows, nbytes) -> None:
        super().__init__(plan.desc, block, stream_ptr, ready)
        self.plan, self.n, self.base, self.exp_bits, self.window, self.windows, self.nbytes = plan, n, base, exp_bits, window, windows, nbytes


class _ModulusRows:
    """Moduli of a key-generation round kept on the device between its steps (survivors of the sieve, in order):
    device rows of the width they were produced in, and the largest bit length."""

    __slots__ = ("rows", "bits")

    def __init__(self, rows, bits: int) -> None:
        self.rows, self.bits = rows, int(bits)

    def operand(self, eng, groups: int, limbs: int):
        """The (rows, bits) operand the tensor-level entry points take, `limbs` words wide."""
        if self.rows.shape[0] != groups:
            raise ValueError("the kept moduli rows do not belong to these candidates")
        if self.bits > 32 * limbs:
            raise ValueError("modulus wider than the limb rows")
        rows = self.rows
        if rows.shape[1] > limbs:
            rows = rows[:, :limbs].contiguous()         # produced in the Shamir field's width: the upper words are zero
        elif rows.shape[1] < limbs:
            rows = eng.torch.nn.functional.pad(rows, (0, limbs - rows.shape[1]))
        return rows, self.bits


    def repeated(self, times: int) -> "_ModulusRows":
        """The same moduli `times` times over (the candidate groups of co-located parties in one launch)."""
        return self if times == 1 else _ModulusRows(self.rows.repeat(times, 1), self.bits)


class _VRows:
    """A party's v values of a round kept on the device: rows [groups * keep, limbs] as biprime_v_t produced them
    (rows beyond a candidate's count hold the modexp of a zero row: 0 or 1) and the counts."""

    __slots__ = ("rows", "counts", "keep")

    def __init__(self, rows, counts, keep: int) -> None:
        self.rows, self.counts, self.keep = rows, counts, int(keep)

    def slots(self, eng, groups: int, n_slots: int, limbs: int):
        if self.rows.shape[0] != groups * self.keep or n_slots > self.keep or self.rows.shape[1] != limbs:
            raise ValueError("the kept v rows do not belong to these candidates")
        return self.rows.view(groups, self.keep, limbs)[:, :n_slots, :]

    def part(self, k: int, parts: int) -> "_VRows":
        """The k-th of `parts` equal slices of the candidate groups (one party's share of a merged launch)."""
        groups = len(self.counts) // parts
        return _VRows(self.rows[k * groups * self.keep : (k + 1) * groups * self.keep], self.counts[k * groups : (k + 1) * groups], self.keep)


class NestedColumn:
    """A party's v values for ``Engine.biprime_verdict_columns`` as ONE LIST PER CANDIDATE (what the reference exchanges,
    distributed_keygen.py:1331-1337) instead of one flat list: each candidate contributes its first n_slots values, zero
    padded — packed by one codec call without a flattened copy."""

    __slots__ = ("lists",)

    def __init__(self, lists) -> None:
        self.lists = lists if isinstance(lists, (list, tuple)) else list(lists)


class Engine(ProofFlows, PrivateKeyFlows):
    """One engine per process/GPU.  Calls enqueue on ``torch.cuda.current_stream()``; every stream gets
    its own workspace, so one Engine may be driven from several streams (one launch in flight per
    stream).  Not thread-safe (matches the reference's single asyncio thread)."""

    MAX_PLANS = 16     # per-key plans kept (a party normally has one key)
    NestedColumn = NestedColumn      # biprime.py asks the engine it was given for it (the CPU test double has none)

    def __init__(self, device: Optional[int] = None) -> None:
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("protocols.distributed_keygen_amd needs an AMD GPU (torch.cuda unavailable); no CPU fallback")
        self.torch = torch
        self.lib = _lib.lib()
        idx = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", idx)
        self._ws: Dict[int, Any] = {}          # stream -> workspace tensor
        self._lpl = 0                          # lane geometry of this engine's modexp launches (0 = automatic)
        self._wpg = 0                          # wavefronts per group of the N^2 pair kernel (0 = automatic, 1, 2)
        self._segments = 0                     # launches per N^2 exponentiation (0 = automatic; include/mxpaillier.h)
        self._fixed_window = False             # tapes of new N^2 plans: fixed windows (secret-independent schedule) instead of sliding ones
        self._n2_plans: "OrderedDict[Tuple[int, int, bool], _Plan]" = OrderedDict()
        self._combine_plans: "OrderedDict[Tuple[int, int, int], _Plan]" = OrderedDict()
        self._crt_plans: "OrderedDict[Tuple[int, int, int], _Plan]" = OrderedDict()
        self._crt_enc_plans: "OrderedDict[Tuple[int, int, int], _Plan]" = OrderedDict()
        self._fixed_base_tables: "OrderedDict[Tuple[int, int, int, int], FixedBaseTable]" = OrderedDict()
        self._side_streams: List[Any] = []     # chunked int-level batches (_pipelined): streams verified concurrent
        self._side_streams_capped = False      # the process has fewer concurrent queues than chunks were wanted
        self._pin: Dict[str, Any] = {}         # pinned staging buffers of _pipelined
        self.last_timing: Optional[Dict[str, Any]] = None   # host/GPU time split of the last int-level modexp batch
        self._priority_aux = False             # small kernels on a high-priority companion stream (set_priority_aux)
        self._aux: Dict[int, Any] = {}         # stream -> its companion
        self._split_streams: Dict[int, Any] = {}   # stream -> the companion that runs the second part of a split launch
        self._crt_streams: Dict[int, Any] = {}     # stream -> the companion that runs the chain modulo q^2 of a private decryption or encryption
        self._cu_streams: Dict[int, List[Any]] = {}    # cu_slice_streams: n -> its streams
        self._side_stream_pool: List[Any] = []     # every chunk stream ever created (_chunk_streams probes them again)
        self._capped_calls = 0                     # requests since _side_streams_capped was set (RECHECK_CAPPED_EVERY)
        self._capped_warned = False
        self._probe_stream: Any = None             # clock_probe_start

    # ------------------------------------------------------------------ plumbing
    def _stream_ptr(self) -> int:
        return int(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, nbytes: int):
        """Scratch of the CURRENT stream (launches on different streams must not share scratch: the
        window tables of one launch would be overwritten by the next)."""
        if nbytes < 0:
            _lib.check(int(nbytes), "workspace query")
        key = self._stream_ptr()
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            self._ws[key] = None
            with self.torch.cuda.device(self.device):
                ws = self.torch.empty(int(nbytes), dtype=self.torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    def _call(self, symbol: str, *args, workspace: Optional[Tuple[Any, ...]] = None, plans: Sequence[_Plan] = ()) -> int:
        """The one way to a C entry point that enqueues work.  Inside the device context: orders the current stream behind
        `plans`, sizes the current stream's workspace by the query `workspace` = (symbol, arguments ...) if the entry point
        takes one, calls `symbol` with `args` followed by (workspace pointer, workspace bytes, stream) or by (stream) —
        every such entry point of include/mxpaillier.h ends in one of the two — and checks the status under its name."""
        with self.torch.cuda.device(self.device):
            for plan in plans:
                self._use_plan(plan)
            if workspace is not None:
                ws = self._workspace(getattr(self.lib, workspace[0])(*workspace[1:]))
                args += (ws.data_ptr(), ws.numel())
            rc = getattr(self.lib, symbol)(*args, self._stream_ptr())
        return _lib.check(rc, symbol)

    def _query(self, symbol: str, *args, outs: Sequence[Any], allow: Any = ()) -> Optional[Tuple[Any, ...]]:
        """The values a C query writes through its trailing out-parameters (`outs`: their ctypes types).  A status in
        `allow` gives None instead of raising."""
        cells = tuple(t() for t in outs)
        rc = getattr(self.lib, symbol)(*args, *cells)
        if rc in allow:
            return None
        _lib.check(rc, symbol)
        return tuple(c.value for c in cells)

    def _use_plan(self, plan: _Plan) -> None:
        """Order the current stream after the plan's uploads if they were enqueued on another stream."""
        cur = self.torch.cuda.current_stream(self.device)
        if plan.stream_ptr != int(cur.cuda_stream):
            # the block was allocated on the stream that prepared it: tell the caching allocator that this
            # stream reads it too, so that an evicted plan's memory is not handed out while launches of
            # this stream that use it are still in flight
            plan.block.record_stream(cur)
        if plan.ready is not None:
            if plan.stream_ptr != int(cur.cuda_stream):
                cur.wait_event(plan.ready)
            if plan.ready.query():
                plan.ready = None

    def _cache_plan(self, cache: "OrderedDict[Any, _Plan]", key: Any, plan: _Plan) -> _Plan:
        """Keeps `plan`, dropping the least recently used ones beyond MAX_PLANS.  Dropping a plan only drops this
        engine's reference to its device block; the memory goes back to torch's caching allocator, which hands a block
        out again only behind the work of (a) the stream it was allocated on — the stream that prepared the plan — and
        (b) every stream named to it with record_stream.  _use_plan names every OTHER stream before that stream's launch
        reads the plan, so a launch still in flight on any stream when a 17th key evicts its plan keeps reading intact
        memory (tests/test_host_logic.py: the eviction test on a stand-in allocator)."""
        cache[key] = plan
        while len(cache) > self.MAX_PLANS:
            cache.popitem(last=False)
        return plan

    def _cached(self, cache: "OrderedDict[Any, _Plan]", key: Any) -> Optional[_Plan]:
        """The plan kept under `key`, now the most recently used one, or None."""
        plan = cache.get(key)
        if plan is not None:
            cache.move_to_end(key)
        return plan

    def _prepare(self, cache: "OrderedDict[Any, _Plan]", key: Any, nbytes: int, symbol: str, args: Tuple[Any, ...], wrap) -> _Plan:
        """A new per-key device block: `nbytes` allocated on the current stream, filled by the prepare entry point `symbol`
        (`args`, then the block and the stream), with the event that marks the end of its uploads;
        ``wrap(block, stream pointer, event)`` makes the plan, which is kept under `key` (_cache_plan)."""
        torch = self.torch
        with torch.cuda.device(self.device):
            block = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            self._call(symbol, *args, block.data_ptr(), block.numel())
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(self.device))
        return self._cache_plan(cache, key, wrap(block, self._stream_ptr(), ready))

    def to_device(self, rows: np.ndarray):
        """uint32 rows -> int32 device tensor (bit pattern preserved)."""
        t = self.torch.from_numpy(np.ascontiguousarray(rows, dtype="<u4").view(np.int32))
        return t.to(self.device, non_blocking=False)

    @staticmethod
    def to_host(t) -> np.ndarray:
        return t.detach().cpu().numpy().view(np.uint32)

    def _upload_ints(self, values, limbs: int, moduli):
        """ints -> device rows of their residues (limbs.pack_reduced), through a pageable copy."""
        return self.to_device(_limbs.pack_reduced(values, limbs, moduli))

    def _empty_rows(self, limbs: int, rows: int = 0):
        return self.torch.empty((rows, limbs), dtype=self.torch.int32, device=self.device)

    def _flags_out(self, out_t, n: int):
        """The caller's uint8 ``[n]`` output once checked, a fresh one when there is none."""
        if out_t is None:
            return self.torch.empty(n, dtype=self.torch.uint8, device=self.device)
        if tuple(out_t.shape) != (n,) or out_t.dtype != self.torch.uint8 or not out_t.is_contiguous():
            raise ValueError(f"out_t must be contiguous uint8 of the shape ({n},)")
        return out_t

    def _download_ints(self, rows_t) -> List[int]:
        """Device rows -> ints, through a pageable copy."""
        return _limbs.unpack(self.to_host(rows_t))

    def synchronize(self) -> None:
        self.torch.cuda.current_stream(self.device).synchronize()

    def set_limbs_per_lane(self, limbs_per_lane: int) -> None:
        """Lane geometry of this engine's modexp launches: 0 = automatic (from the batch size), 9 =
        narrow, 18 = wide, 3 = the latency geometry (the N^2 pair kernel: two wavefronts per group, any key
        length; the generic-modulus kernels: moduli up to 5533 bits, wider ones fall back to the automatic
        choice), 6 = the generic kernels' bipartite latency form (3 limbs per lane, every product on two wavefronts:
        moduli up to 5359 bits; the N^2 pair kernel reads it as 3).  Passed with every call (no process-wide state)."""
        if limbs_per_lane not in (0, 3, 6, 9, 18):
            raise ValueError("limbs_per_lane must be 0, 3, 6, 9 or 18")
        self._lpl = int(limbs_per_lane)

    def set_wavefronts_per_group(self, wavefronts: int) -> None:
        """N^2 pair kernel (powmod_nsquare_t): 1 = one wavefront runs both Montgomery passes of a pair product,
        2 = two wavefronts, one pass each (for launches that leave SIMDs idle), 4 = the five-wavefront latency form
        (both passes bipartite, csrc/mx_bipair.hpp: 3 limbs per lane only, moduli whose groups have 16 or 32 lanes),
        0 = the library's choice (include/mxpaillier.h: mx_powmod_nsquare_run)."""
        if wavefronts not in (0, 1, 2, 4):
            raise ValueError("wavefronts per group must be 0, 1, 2 or 4")
        self._wpg = int(wavefronts)

    GENERIC_LATENCY_MAX_BITS = 29 * 3 * 64 - 4 - 31      # 5533: widest modulus with a 3-limb generic instance (mx_host.hpp: choose_geometry)
    GENERIC_BIPARTITE_MAX_BITS = 29 * 3 * 62 - 35        # 5359: wavefront H needs Pd / 3 + 2 <= 64 lanes (mx_host.hpp)

    def _lpl_generic(self, mod_bits: int = 0) -> int:
        """The engine's lane geometry as the generic-modulus kernels take it.  The latency geometry (3) exists for the
        N^2 pair kernel at every key length but for a GENERIC modulus only up to 5533 bits: an engine tuned with
        set_limbs_per_lane(3) for low-latency decryptions leaves wider generic launches (N^2 of key_length 4096 through
        powmod_batch, say) to the library's automatic choice instead of failing with MX_ERR_SIZE."""
        if self._lpl == 3 and mod_bits > self.GENERIC_LATENCY_MAX_BITS:
            return 0
        if self._lpl == 6 and mod_bits > self.GENERIC_BIPARTITE_MAX_BITS:
            return 0
        return self._lpl if self._lpl in (3, 6, 9, 18) else 0

    def _lpl_n2(self) -> int:
        """... as the N^2 pair kernel takes it: 6 (the generic kernel's bipartite latency form) is its latency geometry 3."""
        return 3 if self._lpl == 6 else self._lpl

    def generic_launch_form(self, mod_bits: int, batch: int = 1, groups: int = 1) -> Tuple[int, int]:
        """(wavefronts per group of elements, pivot) of a generic-modulus modexp launch with this engine's settings:
        (2, hL) for the bipartite latency form (include/mxpaillier.h: mx_powmod_launch_form), else (1, 0)."""
        return self._query("mx_powmod_launch_form", mod_bits, batch, groups, self._lpl_generic(mod_bits), outs=_INTS[:2])

    def set_segments(self, segments: int) -> None:
        """Launches one mx_powmod_nsquare_run exponentiation is cut into (0 = automatic, 1..64)."""
        if not 0 <= segments <= 64:
            raise ValueError("segments must be 0..64")
        self._segments = int(segments)

    def set_fixed_window(self, enable: bool) -> None:
        """Partial decryptions (powmod_nsquare_*) with a FIXED-window tape (MX_PLAN_FIXED_WINDOW, include/mxpaillier.h): the
        number and order of the squarings and multiplications of a launch then depend on the exponent's bit length
        only — the exponent is the party's secret share folded with its Lagrange coefficient (PSK:79-85), and the default
        sliding-window tape is a function of its bits, like gmpy2's mpz_powm.  +3.6 % instructions at key_length 2048 (and twice
        the window table);
        the table row a window reads is still chosen by the secret digit.  Same results bit for bit."""
        self._fixed_window = bool(enable)

    def set_priority_aux(self, enable: bool) -> None:
        """With several launches in flight on several streams, the small kernels of a step (recombination,
        verdict, Jacobi filter, selection: 0.5-5 ms of work) queue for wavefront slots behind the other streams'
        full-machine modexp launches — 4-34 ms of waiting measured (profiles/r02_bench_*_rocprof_summary.txt).
        When enabled they run on a HIGH-PRIORITY companion of the calling stream, ordered by events on both sides
        (the caller still sees them in stream order): the dispatcher hands them the first slots that free up."""
        self._priority_aux = bool(enable)

    def _small(self, fn):
        """fn() on the current stream, or — set_priority_aux — on its high-priority companion between two waits."""
        if not self._priority_aux:
            return fn()
        torch = self.torch
        cur = torch.cuda.current_stream(self.device)
        key = int(cur.cuda_stream)
        aux = self._aux.get(key)
        if aux is None:
            with torch.cuda.device(self.device):
                aux = self._aux[key] = torch.cuda.Stream(device=self.device, priority=-1)
        aux.wait_stream(cur)
        with torch.cuda.stream(aux):
            out = fn()
        cur.wait_stream(aux)
        for t in (out if isinstance(out, tuple) else (out,)):
            if hasattr(t, "record_stream"):
                t.record_stream(cur)         # allocated on the companion, used by the caller's stream from here on
        return out

    def selftest_lanes(self) -> int:
        return self._call("mx_selftest_lanes")

    def geometry(self, mod_bits: int, batch: int = 1, groups: int = 1) -> Tuple[int, int, int, int]:
        """(lanes per element, limbs per lane, limb bits, blocks) of a generic-modulus modexp launch."""
        return self._query("mx_powmod_geometry_for", mod_bits, batch, groups, self._lpl_generic(mod_bits), outs=_INTS[:4])

    def debug_knob(self, knob: str, value: int) -> None:
        """Developer overrides of the library (include/mxpaillier.h: mx_debug_knob; process-wide, 0 restores
        the default): "n2_segments", "jacobi_max_batches", "n2_timeslice" (1 never, 2 always), "n2_friendly_1w" (1 never),
        "n2_lift" (the lifted tape of one-wavefront N^2 launches: 0 never, 1 wherever a plan holds one, 2 = the default, the planner's choice)."""
        ids = {"n2_segments": 1, "jacobi_max_batches": 2, "n2_timeslice": 3, "n2_friendly_1w": 4, "generic_latency": 5, "n2_split": 6, "bi_pivot": 7, "lat_lanes": 8, "n2_bipair": 9, "n2_lift": 10}
        _lib.check(self.lib.mx_debug_knob(ids[knob], int(value)), "mx_debug_knob")

    def cu_slice_streams(self, n: int) -> List[Any]:
        """`n` streams (2..8) whose kernels are confined to disjoint slices of the compute units — the same CU range
        in every XCD (mx_stream_create_cu_slice) — as torch streams.  For callers that keep several SMALL launches in
        flight (each fitting its slice at about one wavefront per SIMD): on ordinary streams the dispatcher stacks
        them on the same CUs.  Created once per engine and n; they live as long as the engine."""
        if n not in self._cu_streams:
            with self.torch.cuda.device(self.device):
                ptrs = [self._query("mx_stream_create_cu_slice", k, n, 0, outs=(_ctypes.c_void_p,))[0] for k in range(n)]
                self._cu_streams[n] = [self.torch.cuda.ExternalStream(ptr, device=self.device) for ptr in ptrs]
        return self._cu_streams[n]

    def clock_probe_start(self, microseconds: int = 300):
        """Enqueue a shader-clock probe (mx_clock_probe) on a high-priority stream of its own, so that it runs
        beside whatever the other streams have in flight; returns a handle for clock_probe_mhz."""
        torch = self.torch
        if self._probe_stream is None:
            with torch.cuda.device(self.device):
                self._probe_stream = torch.cuda.Stream(device=self.device, priority=-1)
        with torch.cuda.device(self.device), torch.cuda.stream(self._probe_stream):
            # allocated and cleared ON the probe stream: a fill enqueued on the caller's (busy) stream would run
            # after the probe and wipe its result
            out = torch.zeros(2, dtype=torch.int64, device=self.device)
            _lib.check(self.lib.mx_clock_probe(int(microseconds), out.data_ptr(), int(self._probe_stream.cuda_stream)), "mx_clock_probe")
        return out

    def clock_probe_mhz(self, handle) -> float:
        """Shader clock in MHz measured by a finished probe (waits for it)."""
        self._probe_stream.synchronize()
        ticks = handle.cpu().tolist()
        return ticks[0] / ticks[1] * 100.0 if ticks[1] else 0.0

    def profile(self, enable: bool) -> None:
        """Start/stop recording events around every modexp kernel launch (process-wide)."""
        _lib.check(self.lib.mx_profile(1 if enable else 0), "mx_profile")

    def profile_collect(self) -> Tuple[float, int]:
        """(sum of kernel durations in ms, launches) since the last collect; waits for the launches."""
        return self._query("mx_profile_collect", outs=(_ctypes.c_double, _ctypes.c_int))

    def nsquare_geometry(self, n_bits: int, batch: int) -> Tuple[int, int, int, int]:
        """(lanes per element, limbs per lane, limb bits, blocks) of a powmod_nsquare launch."""
        return self.nsquare_launch_shape(n_bits, batch)[:4]

    def nsquare_launch_shape(self, n_bits: int, batch: int) -> Tuple[int, int, int, int, int]:
        """(lanes per element, limbs per lane, limb bits, blocks, wavefronts per group) of a
        powmod_nsquare launch of `batch` elements with this engine's settings."""
        return self._query("mx_nsquare_launch_shape", n_bits, batch, self._lpl_n2(), self._wpg, outs=_INTS[:5])

    def nsquare_latency_form(self, n_bits: int) -> Optional[Tuple[int, int, int, int]]:
        """(lanes per element, data positions, pivot, largest batch the library takes the form for by itself) of the
        five-wavefront latency form of powmod_nsquare for moduli of n_bits bits, or None where it has no instance."""
        return self._query("mx_nsquare_latency_form", n_bits, outs=_INTS[:3] + (_ctypes.c_int64,), allow=(-2,))     # MX_ERR_SIZE

    def saturating_shape(self, n_bits: int, total: int) -> Tuple[int, int]:
        """(limbs per lane, wavefronts per group) for powmod_nsquare launches that run SIDE BY SIDE on several
        streams, `total` elements between them.  When they bring about two wavefronts per SIMD or more at one
        wavefront per group of elements and 18 limbs per lane, that shape: fewest instructions per ciphertext
        (include/mxpaillier.h: "callers that keep several launches in flight ... should pass 18 / 1").  Otherwise
        the library's choice for ONE launch of the total, which is what the launches then resemble.  The engine's
        explicit settings win."""
        if not (self._lpl and self._wpg):
            # (a size the library has no such shape for is no error here: it falls through to the pieces' shape)
            wide = self._query("mx_nsquare_launch_shape", n_bits, total, self._lpl_n2() or 18, self._wpg or 1, outs=_INTS[:5], allow=_lib.ERRORS)
            if wide is not None:
                k, l, _, _, wv = wide
                simds = 4 * self.torch.cuda.get_device_properties(self.device).multi_processor_count
                if wv == 1 and l == 18 and total * k // 64 >= 15 * simds // 8:
                    return (18, 1)
        # otherwise what one PLAIN launch of the total would run (a time-sliced form is a lone launch's: 4 x 2500 ciphertexts
        # at key_length 2048 reach 214 k/s at 9 limbs per lane, 179 k/s in the shape of the time-sliced choice for 10 000)
        l_, w_ = self._query("mx_nsquare_pieces_shape", n_bits, total, self._lpl_n2(), self._wpg, outs=_INTS[:2])
        if w_ == 1 and not self._wpg:
            # One launch of the total would run one wavefront per group (a few per cent ahead of two once it has a
            # wavefront for every SIMD), but the launches are `total` in PIECES: a piece with fewer wavefronts than SIMDs
            # is stacked on the CUs of its neighbours, and the two-wavefront form has twice the wavefronts to spread
            # (key_length 4096, 8 x 1024 in flight: 28.7 ms per step on two wavefronts per group, 42.2 on one)
            two = self._query("mx_nsquare_pieces_shape", n_bits, total, self._lpl_n2(), 2, outs=_INTS[:2], allow=_lib.ERRORS)
            if two is not None:
                return (self._lpl_n2() or two[0], 2)
        return (self._lpl_n2() or l_, self._wpg or w_)

    def nsquare_launch_split(self, n_bits: int, batch: int) -> Optional[Tuple[int, Tuple[int, int], Tuple[int, int]]]:
        """(rows of the first launch, its shape, the shape of the rest) when ONE powmod_nsquare batch of this size is
        better run as two launches side by side (mx_nsquare_launch_split) and this engine's settings leave the choice to
        the library; None otherwise.  powmod_nsquare_t follows the hint unless the caller fixed the shape or asked for
        more than one segment (both parts run as single launches); with profile() on, the two launches count as two."""
        if self._lpl or self._wpg:
            return None
        first, a, b, c, d = self._query("mx_nsquare_launch_split", n_bits, batch, outs=(_ctypes.c_int64,) + _INTS[:4])
        return (int(first), (a, b), (c, d)) if first else None

    def nsquare_launch_timesliced(self, n_bits: int, batch: int) -> Tuple[int, int]:
        """(resident workgroups per CU, units per group) when a powmod_nsquare launch of `batch` elements with this
        engine's settings runs in the time-sliced form (mx_nsquare_launch_timesliced), (0, 0) for a plain launch."""
        return self._query("mx_nsquare_launch_timesliced", n_bits, batch, self._lpl_n2(), self._wpg, outs=_INTS[:2])

    def _mods_operand(self, mods, limbs: int, odd_only: bool = True):
        """Moduli of a per-group launch as (device rows [groups, limbs], max bits).  `mods` is a sequence
        of Python ints (validated and uploaded here) or an already device-resident pair (rows, bits)."""
        if _is_device_pair(mods):
            rows_t, bits = mods
            if rows_t.shape[1] != limbs:
                raise ValueError("device moduli must have the row width of the operands")
            return rows_t, int(bits)
        for m in mods:
            if odd_only:
                _check_modulus(m)
        bits = _limbs.max_bits(mods)
        if bits > 32 * limbs:
            raise ValueError("modulus wider than the limb rows")
        return self.to_device(_limbs.pack(mods, limbs)), bits

    # ------------------------------------------------------------------ modexp, tensor level
    @_int_args
    def powmod_shared_t(self, bases_t, mod: int, exp: int, out_t=None):
        """out[e] = bases[e]^exp mod `mod`; bases_t: int32 [batch, limbs] on this device."""
        if exp < 0:
            raise ValueError("negative exponent: invert the base first (paillier_shared_key.py:89-91)")
        batch, limbs = bases_t.shape
        if _limbs.limbs_for(mod) > limbs:
            raise ValueError("modulus wider than the limb rows")
        elimbs = _limbs.limbs_for(exp)
        h_mod = _limbs.pack_one(mod, limbs)
        h_exp = _limbs.pack_one(exp, elimbs)
        if out_t is None:
            out_t = self.torch.empty_like(bases_t)
        self._call("mx_powmod_shared_lpl", bases_t.data_ptr(), out_t.data_ptr(), h_mod.ctypes.data, h_exp.ctypes.data,
                   limbs, elimbs, batch, self._lpl_generic(mod.bit_length()),
                   workspace=("mx_powmod_workspace_bytes", limbs, elimbs, batch, 1))
        return out_t

    def powmod_multi_t(self, bases_t, mods, exps, group_size: int, out_t=None):
        """out[g*group_size+k] = bases[g*group_size+k]^exps[g] mod mods[g].  `mods` / `exps`: sequences of
        ints, or device-resident (rows, max bits) pairs — the operands reach the kernel as device rows
        either way (mx_powmod_multi_dev), so thousands of candidates cost no host-side staging."""
        batch, limbs = bases_t.shape
        mods_t, mod_bits = self._mods_operand(mods, limbs)
        groups = mods_t.shape[0]
        if _is_device_pair(exps):
            exps_t, exp_bits = exps[0], int(exps[1])
        else:
            if len(exps) != groups:
                raise ValueError("one exponent per modulus expected")
            if any(e < 0 for e in exps):
                raise ValueError("negative exponent")
            exp_bits = _limbs.max_bits(exps)
            exps_t = self.to_device(_limbs.pack(exps, _limbs.limbs_for_bits(exp_bits)))
        if exps_t.shape[0] != groups:
            raise ValueError("one exponent per modulus expected")
        elimbs = exps_t.shape[1]
        if batch != groups * group_size:
            raise ValueError("bases must hold groups*group_size rows")
        if out_t is None:
            out_t = self.torch.empty_like(bases_t)
        self._call("mx_powmod_multi_dev", bases_t.data_ptr(), out_t.data_ptr(), mods_t.data_ptr(), exps_t.data_ptr(),
                   limbs, elimbs, mod_bits, exp_bits, groups, group_size, self._lpl_generic(mod_bits),
                   workspace=("mx_powmod_workspace_bytes", limbs, elimbs, batch, groups))
        return out_t

    # ------------------------------------------------------------------ per-key plans
    @_int_args
    def nsquare_plan(self, n: int, exp: int) -> _Plan:
        """The plan of `x -> x^exp mod n^2` (constants and tape of mx_powmod_nsquare_prepare), cached:
        (n, exp) is a key's public modulus and the party's Lagrange-folded share (PSK:46, PSK:79-85)."""
        key = (n, exp, self._fixed_window)
        plan = self._cached(self._n2_plans, key)
        if plan is not None:
            return plan
        if exp < 0:
            raise ValueError("negative exponent: invert the base first (paillier_shared_key.py:89-91)")
        _check_modulus(n)
        limbs_n = _limbs.limbs_for(n)
        elimbs = _limbs.limbs_for(exp)
        h_n = _limbs.pack_one(n, limbs_n)
        h_exp = _limbs.pack_one(exp, elimbs)
        desc = _lib.NsquarePlan()
        nbytes = _lib.check(self.lib.mx_nsquare_plan_bytes(limbs_n, elimbs), "mx_nsquare_plan_bytes")
        flags = _lib.MX_PLAN_FIXED_WINDOW if self._fixed_window else 0
        return self._prepare(self._n2_plans, key, nbytes, "mx_powmod_nsquare_prepare_ex",
                             (desc, h_n.ctypes.data, h_exp.ctypes.data, limbs_n, elimbs, flags), lambda *made: _Plan(desc, *made))

    @_int_args
    def combine_plan(self, n: int, theta_inv: int, limbs2: int) -> _Plan:
        """The plan of the share recombination for a key (mx_combine_prepare), cached."""
        key = (n, theta_inv, limbs2)
        plan = self._cached(self._combine_plans, key)
        if plan is not None:
            return plan
        _check_modulus(n)
        limbs = _limbs.limbs_for(n)
        if _limbs.limbs_for(n * n) > limbs2:
            raise ValueError("partial rows narrower than N^2")
        if not 0 <= theta_inv < n:
            raise ValueError("theta_inv must be a residue modulo N")
        h_n = _limbs.pack_one(n, limbs)
        h_t = _limbs.pack_one(theta_inv, limbs)
        desc = _lib.CombinePlan()
        nbytes = _lib.check(self.lib.mx_combine_plan_bytes(limbs, limbs2), "mx_combine_plan_bytes")
        return self._prepare(self._combine_plans, key, nbytes, "mx_combine_prepare",
                             (desc, h_n.ctypes.data, h_t.ctypes.data, limbs, limbs2), lambda *made: _Plan(desc, *made))

    @_int_args
    def powmod_nsquare_t(self, bases_t, n: int, exp: int, out_t=None, segments: Optional[int] = None,
                         shape: Optional[Tuple[int, int]] = None):
        """out[e] = bases[e]^exp mod n^2 (rows of the width of n^2), computed through pairs modulo n
        (include/mxpaillier.h: mx_powmod_nsquare_prepare / _run) — the fast path of the partial
        decryption PSK:92.  The per-key plan is prepared on first use; afterwards a call is launches only
        (`segments` of them, default: the engine's setting, 0 = the library's choice).  `shape` =
        (limbs per lane, wavefronts per group) overrides the engine's settings for this call."""
        if exp < 0:
            raise ValueError("negative exponent: invert the base first (paillier_shared_key.py:89-91)")
        batch, limbs2 = bases_t.shape
        _check_modulus(n)
        _check_rows_n2(n, limbs2)
        plan = self.nsquare_plan(n, exp)
        if out_t is None:
            out_t = self.torch.empty_like(bases_t)
        # (the split form runs both parts as single launches: an explicit number of segments — the `segments` argument
        # or Engine.set_segments() above 1 — only has a meaning in the one-launch form and disables the split)
        split = None
        if shape is None and segments in (None, 0, 1) and self._segments in (0, 1) and bases_t.is_contiguous() and out_t.is_contiguous():
            split = self.nsquare_launch_split(n.bit_length(), batch)
        if split is not None:
            # one batch just above a capacity step of the wide two-wavefront shape: the part that fills the CUs once in
            # that shape on this stream, the rest at 9 limbs per lane on a companion stream at the same time
            first, shape_a, shape_b = split
            torch = self.torch
            cur = torch.cuda.current_stream(self.device)
            side = self._split_streams.get(int(cur.cuda_stream))
            if side is None:
                with torch.cuda.device(self.device):
                    side = self._split_streams[int(cur.cuda_stream)] = torch.cuda.Stream(device=self.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self.powmod_nsquare_t(bases_t[first:], n, exp, out_t=out_t[first:], segments=1, shape=shape_b)
            self.powmod_nsquare_t(bases_t[:first], n, exp, out_t=out_t[:first], segments=1, shape=shape_a)
            cur.wait_stream(side)
            return out_t
        self._call("mx_powmod_nsquare_run", plan.desc, bases_t.data_ptr(), out_t.data_ptr(), limbs2, batch,
                   self._lpl_n2() if shape is None else int(shape[0]), self._wpg if shape is None else int(shape[1]),
                   self._segments if segments is None else int(segments),
                   workspace=("mx_powmod_nsquare_run_workspace_bytes", plan.desc, batch), plans=(plan,))
        return out_t

    @_int_args
    def powmod_nsquare_batch(self, bases: Sequence[int], exp: int, n: int, keep_rows: bool = False):
        """[pow_mod(b, exp, n*n) for b in bases] through the N-adic pair kernel.  Sequences of
        PIPELINE_MIN elements or more are cut into chunks that run on several streams: the chunks
        together fill the machine (one 10 000-element launch occupies 61 % of the SIMDs), and the
        packing of chunk k+1 and the PCIe copies overlap the modexps of chunk k.
        With ``keep_rows`` the result is ``(ints, rows)`` where ``rows`` is the device-resident copy of
        the results (an opaque column for ``combine_columns``: the party's own partial decryptions go
        into the recombination without being packed a second time)."""
        if len(bases) == 0:
            return ([], None) if keep_rows else []
        n2, limbs2 = _nsquare(n)
        vals = bases if isinstance(bases, list) else list(bases)
        if len(vals) < self.PIPELINE_MIN:
            import time as _t

            # rows are packed straight into a page-locked buffer and come back through one (a pageable copy of the 5.7 MB
            # of 10 000 ciphertexts costs ~1 ms each way: 2 of the 46 ms of such a call)
            count = len(vals)
            t0 = _t.perf_counter()
            in_pin = self._packed_rows("in", vals, limbs2, n2)
            self._pinned("out", count, limbs2)          # (a first call's page-locked allocations both count as packing)
            t1 = _t.perf_counter()
            # a lone launch that is waited for right away: nothing else is in flight whose drain segments
            # could shorten, and the three extra segment boundaries would cost ~1 % (a time-sliced launch keeps the
            # library's number of units per group)
            lone_segments = None
            if self._segments == 0:
                lone_segments = 0 if self.nsquare_launch_timesliced(n.bit_length(), count)[0] else 1
            out_t = self.powmod_nsquare_t(in_pin.to(self.device, non_blocking=True), n, exp, segments=lone_segments)
            out_np = self._fetched_rows("out", out_t)
            t2 = _t.perf_counter()
            res = _limbs.unpack(out_np)
            self.last_timing = {"chunks": 1, "pack_s": t1 - t0, "copies_and_gpu_s": t2 - t1, "unpack_s": _t.perf_counter() - t2}
            return (res, out_t) if keep_rows else res
        self.nsquare_plan(n, exp)          # prepared once, before the chunks fan out over streams
        kept: List[Any] = []
        # the chunks run side by side and fill the machine between them: the shape for that is not the one a lone
        # chunk would get
        chunk_shape = self.saturating_shape(n.bit_length(), len(vals))

        def launch(t):
            out_t = self.powmod_nsquare_t(t, n, exp, shape=chunk_shape)
            if keep_rows:
                kept.append(out_t)
            return out_t

        res = self._pipelined(vals, limbs2, limbs2, launch, modulus=n2)
        if not keep_rows:
            return res
        # the chunk results were allocated on the side streams; the concatenation reads them on the
        # current stream (ordered after the side streams by _pipelined): tell the allocator
        cur = self.torch.cuda.current_stream(self.device)
        for t in kept:
            t.record_stream(cur)
        return res, self.torch.cat(kept, dim=0)

    def powmod_nsquare_groups(self, jobs: Sequence[Tuple[Sequence[int], int, int]]) -> List[List[int]]:
        """[[pow_mod(b, exp, n*n) for b in bases] for (bases, exp, n) in jobs] with the jobs' launches SIDE BY SIDE on
        separate streams: the partial decryptions of several keys — or of the parties of one key that share this
        process and GPU (``distributed=False``: same N, every party its own exponent, hence its own tape) — that are
        pending at the same time (coalesce.Coalescer).  A launch of up to ~1000 ciphertexts lasts as long as one
        wavefront's dependent chain whatever its size, so k small jobs one after the other cost k chains and side by
        side one.  Every job is launched in the shape that suits the SUM in flight (``saturating_shape``)."""
        jobs = [(b if isinstance(b, list) else list(b), int(e), int(n)) for b, e, n in jobs]
        live = [k for k, (b, _, _) in enumerate(jobs) if len(b)]
        total = sum(len(jobs[k][0]) for k in live)
        if len(live) <= 1 or total >= self.PIPELINE_MIN:
            return [self.powmod_nsquare_batch(b, e, n) if len(b) else [] for b, e, n in jobs]
        torch = self.torch
        streams = self._chunk_streams(min(len(live), self.PIPELINE_STREAMS))
        cur = torch.cuda.current_stream(self.device)
        n_bits = max(jobs[k][2].bit_length() for k in live)
        shape = self.saturating_shape(n_bits, total)
        outs: Dict[int, Any] = {}
        for j, k in enumerate(live):
            bases, exp, n = jobs[k]
            n2, limbs2 = _nsquare(n)
            rows = _limbs.pack_reduced(bases, limbs2, n2)
            self.nsquare_plan(n, exp)                     # prepared on the caller's stream, before the fan-out
            side = streams[j % len(streams)]
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                outs[k] = self.powmod_nsquare_t(self.to_device(rows), n, exp, segments=1, shape=shape)
        res: List[List[int]] = [[] for _ in jobs]
        for j, k in enumerate(live):
            with torch.cuda.stream(streams[j % len(streams)]):
                res[k] = self._download_ints(outs[k])     # copied on, and waited for through, the producing stream
        for side in streams[: len(live)]:
            cur.wait_stream(side)
        return res

    # ------------------------------------------------------------------ chunked execution on several streams
    PIPELINE_MIN = 20000       # elements from which an int-level batch is cut into chunks
    PIPELINE_STREAMS = 8

    def stream_concurrency(self, streams: Sequence[Any], spin_us: int = 400) -> List[Any]:
        """The largest prefix-greedy subset of `streams` whose kernels demonstrably run side by side.
        The HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the variable was
        set before the runtime initialised — it cannot be queried or changed afterwards) and two streams
        on one queue serialise.  Measured, not assumed: every candidate stream gets one idle one-wavefront
        kernel (mx_spin) together with the streams accepted so far; if the set takes about one spin it is
        concurrent, if it takes two the newcomer shares a queue with an accepted stream and is dropped.
        The measurement is the native library's (mx_stream_census: C callers get the same answer; it also names the
        stream a dropped one serialises with, which costs a dropped stream log2(accepted) + 1 short probes more than
        the prefix test alone — a few milliseconds, on the set-up path of _chunk_streams only).
        Waits for the device first (one-time cost when the chunk streams are created)."""
        streams = list(streams)
        return [st for k, (st, g) in enumerate(zip(streams, self.stream_census(streams, spin_us))) if g == k]

    def stream_census(self, streams: Sequence[Any], spin_us: int = 400) -> List[int]:
        """mx_stream_census (include/mxpaillier.h) over torch streams: for every stream its own index if it runs beside
        the streams accepted before it, else the index of the first accepted stream it serialises with (-1: with none
        of them alone, only with the set).  Waits for the device and the streams."""
        import ctypes as _ctypes

        streams = list(streams)
        if not streams:
            return []
        ptrs = (_ctypes.c_void_p * len(streams))(*[int(st.cuda_stream) for st in streams])
        groups = (_ctypes.c_int * len(streams))()
        with self.torch.cuda.device(self.device):
            _lib.check(self.lib.mx_stream_census(ptrs, len(streams), int(spin_us), groups), "mx_stream_census")
        return list(groups)

    RECHECK_CAPPED_EVERY = 16       # a capped engine probes again every so many long batches (the cap may have been a hiccup)

    def _chunk_streams(self, wanted: int) -> List[Any]:
        """`wanted` streams for the chunks of a long int-level batch — or fewer, if the process does not have
        that many concurrently running queues (one warning, then larger chunks on the streams that do run
        side by side).  The verdict is a wall-clock measurement on a GPU that others may be using, so a capped
        engine does not keep it forever: it measures again every RECHECK_CAPPED_EVERY requests."""
        torch = self.torch
        if self._side_streams_capped:
            self._capped_calls += 1
            if self._capped_calls % self.RECHECK_CAPPED_EVERY == 0:
                self._side_streams_capped = False
        if len(self._side_streams) < wanted and not self._side_streams_capped:
            with torch.cuda.device(self.device):
                # high-priority streams are served by their own set of hardware queues: the chunks do not
                # collide with (and serialise behind) the caller's other streams even when the process runs
                # with few hardware queues (profiles/r02_hw_queue_collisions.txt)
                pool = self._side_stream_pool
                while len(pool) < wanted:
                    # (the runtime serves at most four high-priority streams side by side whatever GPU_MAX_HW_QUEUES says —
                    # measured: 4 of 7 with 16 queues —, so the streams beyond four are ordinary ones, which do get queues
                    # of their own when the process was started with enough of them)
                    pool.append(torch.cuda.Stream(device=self.device, priority=-1 if len(pool) < 4 else 0))
                cands = self._side_streams + [st for st in pool if st not in self._side_streams][: wanted - len(self._side_streams)]
            ok = self.stream_concurrency(cands)
            if len(ok) < len(cands):
                import warnings

                if not self._capped_warned:
                    self._capped_warned = True
                    # what the PROBE measured, and only then a guess at why: with enough hardware queues configured the
                    # shortfall is the runtime's own stream-to-queue mapping (streams of the process created earlier hold
                    # queues too), not something the caller did
                    import os

                    queues = os.environ.get("GPU_MAX_HW_QUEUES")
                    if queues is None or not queues.isdigit() or int(queues) < 8:
                        why = (f"GPU_MAX_HW_QUEUES is {queues or 'unset (runtime default: 4)'}; call protocols.distributed_keygen_amd."
                               "configure_hw_queues() before the first GPU call, or set GPU_MAX_HW_QUEUES=16")
                    else:
                        why = (f"GPU_MAX_HW_QUEUES={queues} was in effect, so this is the runtime's mapping of this process's streams "
                               "onto its hardware queues, not a missing setting; the engine probes again later")
                    warnings.warn(
                        f"protocols.distributed_keygen_amd: the concurrency probe measured {len(ok)} of {len(cands)} side streams "
                        f"running side by side ({why}): long batches are cut into {max(1, len(ok))} chunks instead of {wanted}",
                        RuntimeWarning, stacklevel=3)
                self._side_streams_capped = True
            self._side_streams = ok
        return self._side_streams[: max(1, min(wanted, len(self._side_streams)))]

    def _pinned(self, which: str, rows: int, limbs: int):
        buf = self._pin.get(which)
        if buf is None or buf.numel() < rows * limbs:
            buf = self.torch.empty(rows * limbs, dtype=self.torch.int32, pin_memory=True)
            self._pin[which] = buf
        return buf[: rows * limbs].view(rows, limbs)

    def _packed_rows(self, which: str, values, limbs: int, moduli, nested: int = 0):
        """ints -> rows [len(values), limbs] of their residues (limbs.pack_reduced) packed in place into the page-locked
        buffer `which`, which is returned.  `nested` = n: `values` is one list per group, every group `n` rows (its first n
        values, zero padded) — limbs.pack_nested_into, no flattened copy."""
        if nested:
            lists = values if isinstance(values, (list, tuple)) else list(values)
            count = len(lists) * nested
        else:
            vals = values if isinstance(values, (list, tuple)) else list(values)
            count = len(vals)
        pin = self._pinned(which, count, limbs)
        rows = pin.numpy().view(np.uint32)
        try:
            if nested:
                _limbs.pack_nested_into(lists, nested, limbs, rows, 0)
            else:
                _limbs.pack_into(vals, limbs, rows, 0)
            _limbs.reduce_rows(rows, moduli)
        except ValueError:                              # a value that does not fit the rows, or a negative one
            if nested:
                vals = [v for g in lists for v in (list(g)[:nested] + [0] * (nested - min(nested, len(g))))]
            rows[:] = _limbs.pack_reduced(vals, limbs, moduli)
        return pin

    def _staged_rows(self, which: str, values, limbs: int, moduli, nested: int = 0):
        """_packed_rows and one asynchronous copy: the device rows.  The caller synchronises with the stream before it
        returns (every int-level entry point fetches a result), so the buffer is free again by the time anybody packs
        into it."""
        return self._packed_rows(which, values, limbs, moduli, nested).to(self.device, non_blocking=True)

    def _fetched_rows(self, which: str, rows_t) -> np.ndarray:
        """Device rows -> host rows in the page-locked buffer `which` (waits for the current stream)."""
        pin = self._pinned(which, rows_t.shape[0], rows_t.shape[1])
        pin.copy_(rows_t, non_blocking=True)
        self.torch.cuda.current_stream(self.device).synchronize()
        return pin.numpy().view(np.uint32)

    def _fetched_ints(self, which: str, rows_t, groups=None):
        """Device rows -> ints through the page-locked buffer `which` (waits for the current stream).  `groups` =
        (counts, stride): one list per group instead (limbs.unpack_groups)."""
        rows = self._fetched_rows(which, rows_t)
        return _limbs.unpack(rows) if groups is None else _limbs.unpack_groups(rows, groups[0], groups[1])

    def _pipelined(self, vals: List[int], limbs_in: int, limbs_out: int, launch, modulus: int = 0) -> List[int]:
        """ints -> ints through `launch(device rows) -> device rows`, chunked over side streams with
        pinned staging buffers: pack chunk k+1 on the host while chunk k is copied and computed.  With
        `modulus` the packed rows are reduced modulo it (bulk: limbs.reduce_rows)."""
        import time as _t

        torch = self.torch
        total = len(vals)
        streams = self._chunk_streams(max(4, min(self.PIPELINE_STREAMS, total // 10000)))
        nchunks = len(streams)
        per = -(-total // nchunks)
        in_pin = self._pinned("in", total, limbs_in)
        out_pin = self._pinned("out", total, limbs_out)
        in_np = in_pin.numpy().view(np.uint32)
        out_np = out_pin.numpy().view(np.uint32)
        cur = torch.cuda.current_stream(self.device)
        events, bounds, keep = [], [], []
        pack_s = 0.0
        t_start = _t.perf_counter()
        for k in range(nchunks):
            lo, hi = k * per, min(total, (k + 1) * per)
            if lo >= hi:
                break
            t0 = _t.perf_counter()
            try:
                _limbs.pack_into(vals[lo:hi], limbs_in, in_np, lo)
            except ValueError:
                if not modulus:
                    raise
                _limbs.pack_into([int(v) % modulus for v in vals[lo:hi]], limbs_in, in_np, lo)
            if modulus:
                _limbs.reduce_rows(in_np[lo:hi], modulus)
            pack_s += _t.perf_counter() - t0
            side = streams[k]
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                d_in = in_pin[lo:hi].to(self.device, non_blocking=True)
                d_out = launch(d_in)
                out_pin[lo:hi].copy_(d_out, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(side)
            keep.append((d_in, d_out))
            events.append(ev)
            bounds.append((lo, hi))
        out: List[int] = []
        wait_s = unpack_s = 0.0
        for ev, (lo, hi) in zip(events, bounds):
            t0 = _t.perf_counter()
            ev.synchronize()
            t1 = _t.perf_counter()
            out.extend(_limbs.unpack(out_np[lo:hi]))
            wait_s += t1 - t0
            unpack_s += _t.perf_counter() - t1
        for side in streams[: len(events)]:
            cur.wait_stream(side)
        self.last_timing = {"chunks": len(events), "pack_s": pack_s, "wait_for_gpu_s": wait_s, "unpack_s": unpack_s,
                            "total_s": _t.perf_counter() - t_start}
        return out

    # ------------------------------------------------------------------ modexp, int level
    @_int_args
    def powmod_batch(self, bases: Sequence[int], exp: int, mod: int) -> List[int]:
        """[pow_mod(b, exp, mod) for b in bases] on the GPU (exp >= 0)."""
        if len(bases) == 0:
            return []
        _check_modulus(mod)
        limbs = _limbs.limbs_for(mod)
        return self._download_ints(self.powmod_shared_t(self._upload_ints(bases, limbs, mod), mod, exp))

    @_int_args
    def powmod_batch_multi(
        self, bases: Sequence[Sequence[int]], exps: Sequence[int], mods: Sequence[int]
    ) -> List[List[int]]:
        """[[pow_mod(b, exps[g], mods[g]) for b in bases[g]] for g]; ragged groups are padded."""
        groups = len(mods)
        if groups == 0:
            return []
        if len(bases) != groups or len(exps) != groups:
            raise ValueError("bases, exps and mods must have one entry per group")
        for m in mods:
            _check_modulus(m)
        gsize = max(len(b) for b in bases)
        if gsize == 0:
            return [[] for _ in bases]
        limbs = _limbs.limbs_for_bits(_limbs.max_bits(mods))
        flat = []
        for b in bases:
            flat.extend(b)
            flat.extend([0] * (gsize - len(b)))
        vals = self._download_ints(self.powmod_multi_t(self._upload_ints(flat, limbs, list(mods)), list(mods), list(exps), gsize))
        return [vals[g * gsize : g * gsize + len(bases[g])] for g in range(groups)]


    # ------------------------------------------------------------------ homomorphic linear maps modulo N^2
    def multiexp_nsquare_shape(self, n: int, n_inputs: int, n_outputs: int, terms: int, weight_bits: int,
                               window: int = 0) -> Tuple[int, int, int]:
        """(window, split-K chunk in terms, table bytes per input and entry) of mx_multiexp_nsquare_shape."""
        k, l, w, chunk = self._query("mx_multiexp_nsquare_shape", int(n).bit_length(), n_inputs, n_outputs, terms, weight_bits, 0,
                                     int(window), outs=_INTS[:3] + (_ctypes.c_int64,))
        return w, int(chunk), 2 * k * l * 4

    def multiexp_nsquare_t(self, inputs_t, weights, n: int, bias: Optional[Sequence[int]] = None, window: int = 0):
        """y_j = (1 + (b_j mod n) n) * prod_i inputs[i]^W[j][i]  mod n^2 on the device (csrc/mx_multiexp_n2.hpp).

        ``inputs_t``: ``[n_inputs, limbs2]`` rows of residues below n^2; ``weights``: one row per output, a dense sequence
        of ``n_inputs`` signed ints or a sparse ``{input: weight}``; ``bias``: one plaintext per output or None.  A negative
        weight uses the input's inverse (computed once on the device; ValueError like ``pow`` if it has none), a zero
        weight gives 1 even for a zero input.  ``window`` > 0 overrides the library's window.  Returns ``[n_outputs,
        limbs2]`` canonical residues — not fresh ciphertexts (re-randomise before they leave the party).  The planning
        (sign split, bias, split-K, buckets, stages) is multiexp_plan.py."""
        from . import multiexp_plan as mp

        n = int(n)
        _check_modulus(n)
        n_inputs, limbs2 = inputs_t.shape
        _check_rows_n2(n, limbs2)
        nb = n.bit_length()
        plan = mp.plan_call(weights, n_inputs, n, bias, lambda a, b, c, d: self.multiexp_nsquare_shape(n, a, b, c, d),
                            window=int(window))
        return mp.execute(plan, _MultiexpBackend(self, n, limbs2, nb), inputs_t)

    def _linear_map_ints(self, cts: Sequence[int], weights, n: int, bias=None, fixed_base=None) -> List[int]:
        if not weights:
            return []
        n2, limbs2 = _nsquare(n)
        if not len(cts):
            from . import multiexp_plan as mp

            mp.normalize_rows(weights, 0, n)          # (a map of no inputs: every row must be empty)
        vals = list(cts) if len(cts) else [0]
        x_t = self._upload_ints(vals, limbs2, n2)
        return self._download_ints(self._freshened(self.multiexp_nsquare_t(x_t, weights, n, bias), fixed_base))

    @_int_args
    def ciphertext_scale_batch(self, cts: Sequence[int], scalars: Sequence[int], n: int, fixed_base=None) -> List[int]:
        """[pow(c, k, n^2) for c, k in zip(cts, scalars)] — ``ciphertext *= k`` with a scalar per ciphertext (any sign).
        ``fixed_base`` (here and in the functions below): see _freshened."""
        if len(cts) != len(scalars):
            raise ValueError("one scalar per ciphertext")
        return self._linear_map_ints(cts, [{k: s} for k, s in enumerate(scalars)], n, fixed_base=fixed_base)

    @_int_args
    def ciphertext_sum_batch(self, groups: Sequence[Sequence[int]], n: int, fixed_base=None) -> List[int]:
        """[prod(g) mod n^2 for g in groups] — the homomorphic sum of every group (an empty group gives 1)."""
        flat: List[int] = []
        rows = []
        for g in groups:
            g = list(g)
            rows.append({len(flat) + t: 1 for t in range(len(g))})
            flat.extend(g)
        return self._linear_map_ints(flat, rows, n, fixed_base=fixed_base)

    @_int_args
    def ciphertext_linear_map_batch(self, cts: Sequence[int], weights, n: int, bias: Optional[Sequence[int]] = None,
                                    fixed_base=None) -> List[int]:
        """The encrypted W x + b: [(1 + (b_j mod n) n) prod_i cts[i]^W[j][i] mod n^2 for j] (rows dense or {index: weight})."""
        return self._linear_map_ints(cts, list(weights), n, bias, fixed_base=fixed_base)

    # ------------------------------------------------------------------ encrypted matrix products over a batch of vectors
    def matmul_nsquare_shape(self, n: int, n_cols: int, n_rows: int, terms: int, weight_bits: int, batch: int,
                             table_budget: int, window: int = 0) -> Tuple[int, int, int]:
        """(window, samples per tile, split-K chunk in terms) of mx_matmul_nsquare_shape."""
        k, l, w, tile, chunk = self._query("mx_matmul_nsquare_shape", int(n).bit_length(), n_cols, n_rows, terms, weight_bits,
                                           int(batch), int(table_budget), 0, int(window),
                                           outs=_INTS[:3] + (_ctypes.c_int64, _ctypes.c_int64))
        return w, int(tile), int(chunk)

    def _matmul_plan(self, n: int, n_inputs: int, batch: int, weights, bias, window: int = 0, table_budget=None):
        from . import multiexp_plan as mp

        _check_modulus(n)
        return mp.plan_matmul(weights, n_inputs, n, bias, batch,
                              lambda *a: self.matmul_nsquare_shape(n, *a),
                              table_budget=_table_budget(table_budget), window=int(window))

    def matmul_nsquare_t(self, x_t, batch: int, weights, n: int, bias: Optional[Sequence[int]] = None, window: int = 0,
                         table_budget: Optional[int] = None):
        """Y[b][j] = (1 + (bias_j mod n) n) * prod_i X[b][i]^W[j][i]  mod n^2 for a batch of ciphertext vectors and ONE
        public matrix W, on the device (csrc/mx_matmul_n2.hpp).

        ``x_t``: ``[batch * n_inputs, limbs2]`` rows of residues below n^2, sample-major; ``weights``: one row per output,
        a dense sequence of ``n_inputs`` signed ints or a sparse ``{column: weight}`` — PUBLIC values: the kernel skips
        their zero digits; ``bias``: one plaintext per output or None.  A negative weight uses the inverses of its column
        (one product tree per call; ValueError like ``pow`` if a sample has none), a zero weight gives 1 even for a zero
        input.  ``window`` > 0 overrides the library's window, ``table_budget`` the bytes of tables one tile of samples may
        take (multiexp_plan.TABLE_BUDGET_BYTES).  Returns ``[batch * n_outputs, limbs2]`` canonical residues, sample-major,
        on the current stream — not fresh ciphertexts.  The planning (column sign split, shared bias tables, tiles,
        split-K, buckets) is multiexp_plan.plan_matmul: once per call, whatever the batch."""
        n, batch = int(n), int(batch)
        _check_modulus(n)
        rows = x_t.shape[0]
        if batch < 0 or (batch == 0 and rows) or (batch and rows % batch):
            raise ValueError("x_t must hold batch * n_inputs rows")
        n_inputs = rows // batch if batch else 0
        return self._matmul_run_t(x_t, batch, n, self._matmul_plan(n, n_inputs, batch, weights, bias, window, table_budget))

    def _matmul_run_t(self, x_t, batch: int, n: int, plan):
        """matmul_nsquare_t with the plan of _matmul_plan already made (for the same n, batch and row width)."""
        from . import multiexp_plan as mp

        limbs2 = x_t.shape[1]
        _check_rows_n2(n, limbs2)
        if x_t.shape[0] != batch * plan.n_inputs:
            raise ValueError("x_t must hold batch * n_inputs rows")
        return mp.execute_matmul(plan, _MatmulBackend(self, n, limbs2, n.bit_length()), x_t, batch)

    @_int_args
    def ciphertext_matmul_batch(self, samples: Sequence[Sequence[int]], weights, n: int, bias: Optional[Sequence[int]] = None,
                                fixed_base=None) -> List[List[int]]:
        """The encrypted W x_b + bias of every sample: [[(1 + (bias_j mod n) n) prod_i samples[b][i]^W[j][i] mod n^2 for j]
        for b] — one public W (rows dense or {column: weight}) over a batch of ciphertext vectors of equal length."""
        samples = [list(smp) for smp in samples]
        if not samples:
            return []
        n_inputs = len(samples[0])
        for b, smp in enumerate(samples):
            if len(smp) != n_inputs:
                raise ValueError(f"sample {b} has {len(smp)} ciphertexts, sample 0 has {n_inputs}")
        weights = weights if isinstance(weights, np.ndarray) else list(weights)
        n2, limbs2 = _nsquare(n)
        plan = self._matmul_plan(n, n_inputs, len(samples), weights, bias)         # every refusal of W and bias: before any launch
        if plan.n_rows == 0:
            return [[] for _ in samples]
        x_t = self._upload_ints([c for smp in samples for c in smp], limbs2, n2) if n_inputs else self._empty_rows(limbs2)
        flat = self._download_ints(self._freshened(self._matmul_run_t(x_t, len(samples), n, plan), fixed_base))
        return [flat[b * plan.n_rows : (b + 1) * plan.n_rows] for b in range(len(samples))]

    # ------------------------------------------------------------------ encrypted convolutions with a public kernel
    def _conv_plan(self, n: int, shape, weights, bias, stride, padding, dilation, window: int = 0, table_budget=None):
        from . import conv_plan as cp

        _check_modulus(n)
        return cp.plan_conv(weights, shape, n, bias, lambda a, b, c, d, w: self.multiexp_nsquare_shape(n, a, b, c, d, w),
                            stride=stride, padding=padding, dilation=dilation,
                            table_budget=_table_budget(table_budget), window=int(window))

    def conv2d_nsquare_t(self, x_t, shape, weights, n: int, bias: Optional[Sequence[int]] = None, stride=1, padding=0,
                         dilation=1, window: int = 0, table_budget: Optional[int] = None):
        """Y[b][o][y][x] = (1 + (bias_o mod n) n) * prod_(c,i,j) X[b][c][y sh - ph + i dh][x sw - pw + j dw]^w[o][c][i][j]
        mod n^2: B grids of ciphertexts under ONE public kernel, on the device (csrc/mx_matmul_n2.hpp).
        Cross-correlation, the convention of torch.nn.functional.conv2d; a tap outside the grid contributes 1.

        ``x_t``: ``[B * C * H * W, limbs2]`` rows of residues below n^2 with ``shape = (B, C, H, W)``; ``weights``:
        ``[O][C][kh][kw]`` signed ints — PUBLIC values: the kernel skips their zero digits; ``bias``: one plaintext per
        kernel or None; ``stride``, ``padding`` (zeros) and ``dilation``: an int or a pair (rows, columns).  A negative tap
        uses the inverses of its channel (one product tree per call; ValueError like ``pow`` if a pixel has none), a zero
        tap gives 1 even on a zero input.  ``window`` > 0 overrides the library's window, ``table_budget`` the bytes of
        tables one tile (whole images, or a band of output rows of one image) may take.  Returns ``[B * O * H' * W',
        limbs2]`` canonical residues on the current stream — not fresh ciphertexts.  The planning is
        conv_plan.plan_conv: once per call, whatever B and H' W'."""
        n = int(n)
        return self._conv_run_t(x_t, n, self._conv_plan(n, tuple(shape), weights, bias, stride, padding, dilation, window, table_budget))

    def _conv_run_t(self, x_t, n: int, plan):
        from . import conv_plan as cp

        limbs2 = x_t.shape[1]
        _check_rows_n2(n, limbs2)
        b, c, h, w = plan.shape
        if x_t.shape[0] != b * c * h * w:
            raise ValueError("x_t must hold B * C * H * W rows")
        return cp.execute_conv(plan, _ConvBackend(self, n, limbs2, n.bit_length()), x_t.contiguous())

    @_int_args
    def ciphertext_conv2d_batch(self, x, weights, n: int, bias: Optional[Sequence[int]] = None, stride=1, padding=0,
                                dilation=1, fixed_base=None) -> List[List[List[List[int]]]]:
        """The encrypted convolution of every grid x[b] ([C][H][W] ciphertexts) with the public kernel ``weights``
        ([O][C][kh][kw]): nested lists [B][O][H'][W'] of the values conv2d_nsquare_t describes."""
        shape, flat = _grid_shape(x)
        n2, limbs2 = _nsquare(n)
        plan = self._conv_plan(n, shape, weights, bias, stride, padding, dilation)      # every refusal of the kernel: before any launch
        x_t = self._upload_ints(flat, limbs2, n2) if flat else self._empty_rows(limbs2)
        vals = self._download_ints(self._freshened(self._conv_run_t(x_t, n, plan), fixed_base)) if shape[0] and plan.n_rows else []
        o, oh, ow = plan.n_rows, plan.out_h, plan.out_w
        return [[[vals[((b * o + j) * oh + y) * ow : ((b * o + j) * oh + y + 1) * ow] for y in range(oh)] for j in range(o)]
                for b in range(shape[0])]

    # ------------------------------------------------------------------ encrypted histograms by a public bin index
    def histogram_nsquare_shape(self, n: int, n_samples: int, n_segments: int, total_terms: int,
                                chunk: int = 0) -> Tuple[int, int, int, int]:
        """(lanes, limbs per lane, terms per piece, row bytes per sample) of mx_histogram_nsquare_shape."""
        k, l, c, row_bytes = self._query("mx_histogram_nsquare_shape", int(n).bit_length(), int(n_samples), int(n_segments),
                                         int(total_terms), 0, int(chunk), outs=_INTS[:3] + (_ctypes.c_int64,))
        return k, l, c, int(row_bytes)

    def histogram_nsquare_t(self, cts_t, bins_t, n_bins: int, n: int, chunk: int = 0, table_budget_bytes: int = 0):
        """H[f][b] = prod_{i : bins[f][i] == b} cts[i]  mod n^2 on the device (csrc/mx_hist_n2.hpp): the
        sums of ciphertexts by a PUBLIC bin index, weight-1 products only — no inverse is needed, of any input.

        ``cts_t``: ``[n_samples, limbs2]`` rows of residues below n^2; ``bins_t``: an integer tensor ``[F, n_samples]``
        with values in [0, n_bins), or -1 for a sample that is not in this feature's histogram (a missing value, a sample
        outside the node).  Returns ``[F * n_bins, limbs2]`` canonical residues on the current stream (row f * n_bins + b;
        an empty bin is 1) — not fresh ciphertexts — and never leaves the device.  ``chunk`` > 0 overrides the terms per
        piece, ``table_budget_bytes`` > 0 the bytes one stage of samples may take for its rows and index arrays
        (hist_plan.TABLE_BUDGET_BYTES): for tests and probes.  ValueError, before any launch, for bins of another
        shape or dtype, a bin outside [-1, n_bins) (one reduction on the device), n_bins < 1, or a modulus the pair kernel
        refuses.  The planning (sorting, pieces, levels, stages, slices) is hist_plan.py."""
        from . import hist_plan as hp

        n, n_bins, chunk = int(n), int(n_bins), int(chunk)
        _check_modulus(n)
        n_samples, limbs2 = cts_t.shape
        _check_rows_n2(n, limbs2)
        if not 0 <= chunk <= hp.MAX_CHUNK:
            raise ValueError(f"chunk must lie in [0, {hp.MAX_CHUNK}]")
        bins_t = hp.as_bins(bins_t, n_samples, self.device)
        hp.check_bins(bins_t, n_samples, n_bins)
        return self._histogram_run_t(cts_t, bins_t, n_bins, n, chunk, int(table_budget_bytes))

    def _histogram_run_t(self, cts_t, bins_t, n_bins: int, n: int, chunk: int = 0, table_budget_bytes: int = 0):
        """histogram_nsquare_t for a device bin tensor that check_bins has passed (on either side of the upload)."""
        from . import hist_plan as hp

        with self.torch.cuda.device(self.device):
            return hp.histogram(_HistogramBackend(self, n, cts_t.shape[1], n.bit_length()), cts_t.contiguous(), bins_t, n_bins,
                                chunk, table_budget_bytes)

    @_int_args
    def ciphertext_histogram_batch(self, cts: Sequence[int], bins, n_bins: int, n: int, fixed_base=None) -> List[List[int]]:
        """[[prod(c_i for i with bins[f][i] == b) mod n^2 for b in range(n_bins)] for f] — the histogram of the
        ciphertexts by every feature's public bin index (nested lists, a numpy array or a torch tensor ``[F][len(cts)]``
        with values in [0, n_bins), or -1: not in this feature's histogram).  An empty bin gives 1."""
        from . import hist_plan as hp

        n2, limbs2 = _nsquare(n)
        vals = cts if isinstance(cts, (list, tuple)) else list(cts)
        bins_t = hp.as_bins(bins, len(vals))
        hp.check_bins(bins_t, len(vals), n_bins)                    # every refusal: before anything is uploaded
        feats = bins_t.shape[0]
        if feats == 0:
            return []
        x_t = self._upload_ints(vals, limbs2, n2) if vals else self._empty_rows(limbs2)
        flat = self._download_ints(self._freshened(self._histogram_run_t(x_t, bins_t.to(self.device), n_bins, n), fixed_base))
        return [flat[f * n_bins : (f + 1) * n_bins] for f in range(feats)]

    # ------------------------------------------------------------------ encrypted sparse matrix products (public CSR matrix)
    def spmm_nsquare_shape(self, n: int, n_tables: int, n_rows: int, nnz: int, weight_bits: int,
                           window: int = 0) -> Tuple[int, int, int]:
        """(window, digit positions, row bytes per table entry) of mx_spmm_nsquare_shape: the library's window for
        `n_tables` tables (the inputs plus the inverted columns), `n_rows` output rows and `nnz` stored terms of weights
        below 2^weight_bits; ``window`` > 0 overrides it."""
        k, l, w, positions, row_bytes = self._query("mx_spmm_nsquare_shape", int(n).bit_length(), int(n_tables), int(n_rows),
                                                    int(nnz), int(weight_bits), 0, int(window),
                                                    outs=_INTS[:4] + (_ctypes.c_int64,))
        return w, positions, int(row_bytes)

    def spmm_nsquare_t(self, cts_t, crow_t, col_t, val_t, n: int, bias: Optional[Sequence[int]] = None, window: int = 0,
                       chunk: int = 0, table_budget_bytes: int = 0):
        """y_r = (1 + (bias_r mod n) n) * prod_{t in [crow[r], crow[r+1])} cts[col[t]]^val[t]  mod n^2 on the device
        (csrc/mx_spmm_n2.hpp): the product of a PUBLIC sparse matrix in CSR form with a vector of
        ciphertexts, as a histogram over the windowed digits of the weights and Horner's rule over the digit positions.

        ``cts_t``: ``[n_in, limbs2]`` rows of residues below n^2; ``crow_t`` ``[R + 1]``, ``col_t`` ``[nnz]`` and signed
        ``val_t`` ``[nnz]`` (|val| <= 2^63 - 1): integer tensors on the device or the host (lists and numpy arrays are
        taken too); ``bias``: one plaintext per row or None.  A negative weight uses the inverse of its input (one product
        tree for all such columns; ValueError like ``pow`` if one has none — under positive weights only, a
        non-invertible input is legal), duplicate (row, column) entries are terms of their own, a stored 0 is no term, an
        empty row gives 1 or its bias factor.  Returns ``[R, limbs2]`` canonical residues on the current stream — not
        fresh ciphertexts.  ``window`` in 1..8 overrides the library's window, ``chunk`` > 0 the terms per piece,
        ``table_budget_bytes`` > 0 the bytes one stage of tables may take with its index arrays
        (spmm_plan.TABLE_BUDGET_BYTES): for tests and probes.  ValueError, before any launch, for arrays of another
        shape or dtype, a crow that does not run from 0 to nnz without decreasing, a column outside [0, n_in), a value
        of -2^63, a bias of another length, or a modulus the pair kernel refuses.  The planning (digits, tables, sorting,
        pieces, levels, stages) is spmm_plan.py."""
        from . import spmm_plan as sp

        n, window, chunk = int(n), int(window), int(chunk)
        _check_modulus(n)
        n_in, limbs2 = cts_t.shape
        _check_rows_n2(n, limbs2)
        if not 0 <= window <= sp.MAX_WINDOW:
            raise ValueError(f"window must lie in [0, {sp.MAX_WINDOW}]")
        if not 0 <= chunk <= sp.hp.MAX_CHUNK:
            raise ValueError(f"chunk must lie in [0, {sp.hp.MAX_CHUNK}]")
        crow_t, col_t, val_t = (t.to(self.device) for t in sp.as_matrix((crow_t, col_t, val_t), n_in))
        sp.check_bias(bias, crow_t.numel() - 1)
        sp.check_matrix(crow_t, col_t, val_t, n_in)
        return self._spmm_run_t(cts_t, crow_t, col_t, val_t, n, bias, window, chunk, int(table_budget_bytes))

    def _spmm_run_t(self, cts_t, crow_t, col_t, val_t, n: int, bias=None, window: int = 0, chunk: int = 0,
                    table_budget_bytes: int = 0):
        """spmm_nsquare_t for device index tensors that check_matrix has passed (on either side of the upload)."""
        from . import spmm_plan as sp

        with self.torch.cuda.device(self.device):
            return sp.spmm(_SpmmBackend(self, n, cts_t.shape[1], n.bit_length()), cts_t.contiguous(), cts_t.shape[0], crow_t,
                           col_t, val_t, bias, window, chunk, table_budget_bytes)

    @_int_args
    def ciphertext_spmm_batch(self, cts: Sequence[int], crow, col, val, n: int, bias: Optional[Sequence[int]] = None,
                              fixed_base=None) -> List[int]:
        """[(1 + (bias_r mod n) n) * prod(pow(cts[col[t]], val[t], n^2) for t in range(crow[r], crow[r+1])) mod n^2 for r]
        — the product of the public sparse matrix (crow, col, val) in CSR form (lists, numpy arrays or torch tensors)
        with the ciphertexts.  ``pow`` with a negative weight is the inverse; an empty row gives 1 or its bias factor."""
        from . import spmm_plan as sp

        n2, limbs2 = _nsquare(n)
        vals = cts if isinstance(cts, (list, tuple)) else list(cts)
        crow_t, col_t, val_t = sp.as_matrix((crow, col, val), len(vals))
        sp.check_bias(bias, crow_t.numel() - 1)
        sp.check_matrix(crow_t, col_t, val_t, len(vals))            # every refusal: before anything is uploaded
        if crow_t.numel() == 1:
            return []
        x_t = self._upload_ints(vals, limbs2, n2) if vals else self._empty_rows(limbs2)
        out_t = self._spmm_run_t(x_t, crow_t.to(self.device), col_t.to(self.device), val_t.to(self.device), n, bias)
        return self._download_ints(self._freshened(out_t, fixed_base))

    # ------------------------------------------------------------------ encrypted prefix sums over series of ciphertexts
    def cumsum_nsquare_t(self, cts_t, lengths, n: int, exclusive: bool = False, reverse: bool = False, chunk: int = 0,
                         table_budget_bytes: int = 0):
        """out[j] = the product modulo n^2 of cts[first .. j] over the segment that holds j, on the device
        (csrc/mx_scan_n2.hpp): the running totals of series of ciphertexts laid one behind the other.

        ``cts_t``: ``[count, limbs2]`` rows of residues below n^2; ``lengths``: the PUBLIC lengths of the series (a
        sequence, a numpy array or an integer tensor; they sum to count, 0 is legal; None: one series).  ``exclusive``
        leaves cts[j] itself out (the first output of a series is 1), ``reverse`` runs every series from its end.
        Returns ``[count, limbs2]`` canonical residues on the current stream — not fresh ciphertexts — and never leaves
        the device.  Weight-1 products only: no input needs an inverse, and a 0 makes every later prefix of its series
        0.  ``chunk`` > 0 overrides the rows per piece, ``table_budget_bytes`` > 0 the bytes one stage of elements may
        take (scan_plan.TABLE_BUDGET_BYTES): for tests and probes.  ValueError, before any launch, for lengths that are
        negative, not integers, not one-dimensional or do not sum to count, or a modulus the pair kernel refuses.  The
        planning (pieces, levels, carries, stages) is scan_plan.py."""
        from . import scan_plan as sp

        n, chunk = int(n), int(chunk)
        _check_modulus(n)
        count, limbs2 = cts_t.shape
        _check_rows_n2(n, limbs2)
        if not 0 <= chunk <= sp.MAX_CHUNK:
            raise ValueError(f"chunk must lie in [0, {sp.MAX_CHUNK}]")
        lengths_t = sp.as_lengths(lengths, count, self.device)
        with self.torch.cuda.device(self.device):
            return sp.cumsum(_ScanBackend(self, n, limbs2, n.bit_length()), cts_t.contiguous(), lengths_t, bool(exclusive),
                             bool(reverse), chunk, int(table_budget_bytes))

    @_int_args
    def ciphertext_cumsum_batch(self, cts: Sequence[int], lengths, n: int, exclusive: bool = False, reverse: bool = False,
                                fixed_base=None) -> List[int]:
        """[prod(cts[first .. j]) mod n^2 for every j] over the series of the given public lengths laid one behind the
        other (None: one series) — cumsum_nsquare_t, ints to ints."""
        from . import scan_plan as sp

        n2, limbs2 = _nsquare(n)
        vals = cts if isinstance(cts, (list, tuple)) else list(cts)
        lengths_t = sp.as_lengths(lengths, len(vals))               # every refusal: before anything is uploaded
        _check_modulus(n)
        if not vals:
            return []
        x_t = self._upload_ints(vals, limbs2, n2)
        return self._download_ints(self._freshened(self.cumsum_nsquare_t(x_t, lengths_t, n, exclusive, reverse), fixed_base))

    # ------------------------------------------------------------------ packing: many small plaintexts per ciphertext
    def pack_nsquare_t(self, cts_t, n: int, slot_bits: int, slots: int):
        """out[j] = prod_{i < slots} cts[j * slots + i]^(2^(slot_bits * i)) mod n^2 on the device (csrc/mx_pack_n2.hpp):
        one ciphertext of sum_i m_i 2^(slot_bits i) per ``slots`` inputs, the last one holding the rest.

        ``cts_t``: ``[count, limbs2]`` rows of residues below n^2; returns ``[ceil(count / slots), limbs2]`` canonical
        residues — not fresh ciphertexts.  ``slot_bits * slots`` must not exceed bits(n) - 2 (ValueError); the slot
        layout of a protocol is packing.py's."""
        n, slot_bits, slots = int(n), int(slot_bits), int(slots)
        _check_modulus(n)
        count, limbs2 = cts_t.shape
        _check_rows_n2(n, limbs2)
        if slot_bits < 1 or slots < 1 or slot_bits * slots > n.bit_length() - 2:
            raise ValueError(f"{slots} slots of {slot_bits} bits do not fit a plaintext of {n.bit_length()} bits")
        torch = self.torch
        out_t = torch.empty((-(-count // slots), limbs2), dtype=torch.int32, device=self.device)
        if count == 0:
            return out_t
        cts_t = cts_t.contiguous()
        plan = self.nsquare_plan(n, 1)          # the constants of mx_powmod_nsquare_prepare (its exponent is not read)
        self._call("mx_pack_nsquare_run", plan.desc, cts_t.data_ptr(), count, limbs2, slot_bits, slots, out_t.data_ptr(), 0, plans=(plan,))
        return out_t

    @_int_args
    def ciphertext_pack_batch(self, cts: Sequence[int], n: int, slot_bits: int, slots: int, fixed_base=None) -> List[int]:
        """[prod_{i < slots} cts[j * slots + i]^(2^(slot_bits * i)) mod n^2 for j < ceil(len(cts) / slots)]
        (pack_nsquare_t).  Inputs are reduced modulo n^2; any residue is valid, 0 and multiples of n included (nothing
        is inverted)."""
        n2, limbs2 = _nsquare(n)
        if not len(cts):
            return []
        x_t = self._upload_ints(cts if isinstance(cts, list) else list(cts), limbs2, n2)
        return self._download_ints(self._freshened(self.pack_nsquare_t(x_t, n, slot_bits, slots), fixed_base))

    # ------------------------------------------------------------------ slot-packed plaintexts: the codec on the device
    def _slot_layout(self, n: int, slot_bits: int, signed: bool) -> Tuple[int, int, Any]:
        """(k, limbs(n), N as a host array of words) of packing.py's layout; ValueError for a slot the int64 codec does not take."""
        from .packing import slots_per_ciphertext

        _check_modulus(n)
        top = 64 if signed else 63
        if not 1 <= slot_bits <= top:
            raise ValueError(f"the device codec takes {'signed' if signed else 'unsigned'} slots of 1 .. {top} bits (int64 values); "
                             "wider slots stay with packing.unpack")
        k = slots_per_ciphertext(n, slot_bits)
        limbs = _limbs.limbs_for(n)
        return k, limbs, np.ascontiguousarray(_limbs.pack_one(n, limbs))

    def _slot_values(self, values_t):
        """An int64 vector on this engine's device: a device tensor as it is, a host tensor or numpy array uploaded."""
        torch = self.torch
        if isinstance(values_t, np.ndarray):
            if values_t.dtype.kind not in "iu" or (values_t.dtype.kind == "u" and values_t.dtype.itemsize == 8 and values_t.size
                                                   and int(values_t.max()) >> 63):
                raise ValueError("an integer array within int64 expected")
            values_t = torch.from_numpy(np.ascontiguousarray(values_t, dtype=np.int64))
        if torch.is_tensor(values_t) and values_t.dtype in (torch.int8, torch.uint8, torch.int16, torch.int32):
            values_t = values_t.to(torch.int64)
        if not torch.is_tensor(values_t) or values_t.dtype != torch.int64 or values_t.dim() != 1:
            raise ValueError("a one-dimensional integer tensor (int64 or narrower) expected")
        if values_t.is_cuda and values_t.device != self.device:
            raise ValueError(f"the values live on {values_t.device}, the operation runs on {self.device}")
        return values_t.to(self.device).contiguous()

    @_int_args
    def slots_encode_t(self, values_t, n: int, slot_bits: int, signed: bool = True, row_words: Optional[int] = None):
        """int64 values -> ``[ceil(count / k), limbs(n)]`` int32 plaintext rows of packing.py's layout on the device
        (csrc/mx_slots.hpp): value j k + i in bits [b i, b (i + 1)) of plaintext j, k = slots_per_ciphertext(n, b);
        signed plaintexts are (sum_i m_i 2^(b i)) mod n.  The rows are what fixed_base_encrypt_t takes as messages.

        ``values_t``: an int64 tensor on this engine's device, or a host tensor or numpy integer array, which is
        uploaded.  ``row_words`` > limbs(n) widens the rows with zero words.  ValueError naming the first offending
        index when a value lies outside [-2^(b-1), 2^(b-1)) (signed) or [0, 2^b) (unsigned); no rows are returned then.
        Reading the status bytes waits for the kernel."""
        signed = bool(signed)
        k, limbs, n_words = self._slot_layout(n, slot_bits, signed)
        torch = self.torch
        v_t = self._slot_values(values_t)
        count = v_t.shape[0]
        outputs = -(-count // k)
        stride = limbs if row_words is None else int(row_words)
        if stride < limbs:
            raise ValueError("rows narrower than N")
        out_t = torch.empty((outputs, stride), dtype=torch.int32, device=self.device)
        if count == 0:
            return out_t
        status_t = torch.empty(outputs, dtype=torch.uint8, device=self.device)
        self._call("mx_slots_encode", v_t.data_ptr(), count, n_words.ctypes.data, limbs, slot_bits, k, int(signed), out_t.data_ptr(), stride,
                   status_t.data_ptr())
        if bool(status_t.any()):
            j = int(torch.nonzero(status_t)[0])
            part = v_t[j * k : (j + 1) * k]
            lo, hi = (-(1 << (slot_bits - 1)), (1 << (slot_bits - 1)) - 1) if signed else (0, (1 << slot_bits) - 1)
            idx = j * k + int(torch.nonzero((part < lo) | (part > hi))[0])
            raise ValueError(f"value {idx} ({int(v_t[idx])}) does not fit a {'signed' if signed else 'unsigned'} slot of {slot_bits} bits")
        return out_t

    @_int_args
    def slots_decode_t(self, rows_t, n: int, slot_bits: int, count: int, signed: bool = True):
        """Plaintext rows -> the ``count`` int64 slot values, on the device: packing.unpack for slots of up to 64 (unsigned:
        63) bits.  ``rows_t``: ``[ceil(count / k), >= limbs(n)]`` int32 residues in [0, n) — words beyond limbs(n) are
        ignored, so the rows of ``combine_t(..., packed=True)`` are taken as they are.  Enqueues on the current stream and
        does not wait; ValueError for a wrong number of rows or rows narrower than n."""
        signed = bool(signed)
        k, limbs, n_words = self._slot_layout(n, slot_bits, signed)
        torch = self.torch
        outputs = -(-count // k)
        if count < 0 or rows_t.dim() != 2 or rows_t.shape[0] != outputs:
            raise ValueError(f"{count} values of {slot_bits} bits need {outputs} packed plaintext rows, got {tuple(rows_t.shape)}")
        if rows_t.shape[1] < limbs:
            raise ValueError("plaintext rows narrower than N")
        if rows_t.dtype != torch.int32 or rows_t.device != self.device:
            raise ValueError(f"int32 plaintext rows on {self.device} expected")
        out_t = torch.empty(count, dtype=torch.int64, device=self.device)
        if count == 0:
            return out_t
        rows_t = rows_t.contiguous()
        self._call("mx_slots_decode", rows_t.data_ptr(), rows_t.shape[1], count, n_words.ctypes.data, limbs, slot_bits, k, int(signed),
                   out_t.data_ptr())
        return out_t

    # ------------------------------------------------------------------ fixed base: encryption and re-randomisation
    def fixed_base_shape(self, n: int, exp_bits: int, count: int, window: int = 0, table_budget_bytes: int = 0) -> Tuple[int, int, int]:
        """(window, windows, table bytes) of mx_fixedbase_nsquare_shape for `count` outputs per call."""
        nb = int(n).bit_length()
        _, _, w, nw = self._query("mx_fixedbase_nsquare_shape", nb, int(exp_bits), int(count), int(table_budget_bytes), 0, int(window),
                                  outs=_INTS[:4])
        nbytes = _lib.check(self.lib.mx_fixedbase_nsquare_table_bytes(nb, int(exp_bits), 0, w), "mx_fixedbase_nsquare_table_bytes")
        return w, nw, int(nbytes)

    FIXED_BASE_MODEL_COUNT = 100000      # outputs per call the automatic window is chosen for (the table is per key)

    @_int_args
    def fixed_base_table(self, n: int, base: int, exp_bits: int, window: int = 0) -> FixedBaseTable:
        """The table of ``base^(d 2^(w i)) mod n^2`` (csrc/mx_fixedbase_n2.hpp) for exponents below ``2^exp_bits``,
        built on first use and cached per (n, base, exp_bits, window) beside the N^2 plans, with _cache_plan's eviction
        discipline.  ``window`` = 0: the library's choice for FIXED_BASE_MODEL_COUNT outputs per call.  ``base`` is
        reduced modulo n^2; any residue is valid."""
        key = (n, base, exp_bits, window)
        tab = self._cached(self._fixed_base_tables, key)
        if tab is not None:
            return tab
        n2, limbs2 = _nsquare(n)
        if exp_bits < 1 or exp_bits > 2 * n.bit_length() + 64:
            raise ValueError(f"exp_bits must lie in 1 .. 2 bits(n) + 64 = {2 * n.bit_length() + 64}")
        if not 0 <= window <= 8:
            raise ValueError("window must lie in 1 .. 8 (0 = automatic)")
        w, windows, nbytes = self.fixed_base_shape(n, exp_bits, self.FIXED_BASE_MODEL_COUNT, window)
        plan = self.nsquare_plan(n, 1)          # the constants of mx_powmod_nsquare_prepare (its exponent is not read)
        with self.torch.cuda.device(self.device):
            self._use_plan(plan)
            base_t = self._upload_ints([base], limbs2, n2)
        return self._prepare(self._fixed_base_tables, key, nbytes, "mx_fixedbase_nsquare_prepare",
                             (plan.desc, base_t.data_ptr(), limbs2, exp_bits, 0, w),
                             lambda *made: FixedBaseTable(plan, *made, n, base % n2, exp_bits, w, windows, nbytes))

    def _freshened(self, rows_t, fixed_base):
        """``rows_t`` (ciphertext rows modulo n^2, on the device) re-randomised there before they are fetched:
        ``fixed_base`` = (n, base, exp_bits, window, exponents) multiplies row r by base^(e_r) mod n^2 through the
        table of fixed_base_table (exponents as fixed_base_exponent_rows takes them); None returns the rows as they are."""
        if fixed_base is None:
            return rows_t
        n, base, exp_bits, window, exps = fixed_base
        table = self.fixed_base_table(n, base, exp_bits, window)
        if rows_t.shape[1] != _limbs.limbs_for(table.n * table.n):
            raise ValueError("the rows are not residues modulo the randomiser's N^2")
        return self.fixed_base_randomize_t(table, self.fixed_base_exponent_rows(exps, exp_bits), rows_t)

    def _fixed_base_run(self, table: FixedBaseTable, mode: int, exps_t, operand_t):
        torch = self.torch
        count, ewords = exps_t.shape
        if ewords != (table.exp_bits + 31) // 32:
            raise ValueError(f"exponent rows of {(table.exp_bits + 31) // 32} words expected for {table.exp_bits} bits")
        limbs2 = _limbs.limbs_for(table.n * table.n)
        op_limbs = 0
        if operand_t is not None:
            if operand_t.shape[0] != count:
                raise ValueError("one operand row per exponent row expected")
            op_limbs = operand_t.shape[1]
            if mode != _lib.MX_FIXEDBASE_ENCRYPT:
                _check_rows_n2(table.n, op_limbs)
            elif op_limbs < _limbs.limbs_for(table.n):
                raise ValueError("operand rows narrower than N")
            operand_t = operand_t.contiguous()
        out_t = torch.empty((count, limbs2), dtype=torch.int32, device=self.device)
        if count == 0:
            return out_t
        exps_t = exps_t.contiguous()
        self._call("mx_fixedbase_nsquare_run", table.desc, table.block.data_ptr(), table.exp_bits, table.window, mode,
                   exps_t.data_ptr(), operand_t.data_ptr() if operand_t is not None else None,
                   op_limbs, out_t.data_ptr(), count, limbs2, 0, plans=(table.plan, table))
        return out_t

    def fixed_base_power_t(self, table: FixedBaseTable, exps_t):
        """out[r] = base^(e_r) mod n^2 — a batch of randomisers.  ``exps_t``: ``[count, ceil(exp_bits / 32)]`` little-endian
        words on the device; bits at ``exp_bits`` and above are ignored.  No squaring: one pair product per window."""
        return self._fixed_base_run(table, _lib.MX_FIXEDBASE_POWER, exps_t, None)

    def fixed_base_encrypt_t(self, table: FixedBaseTable, exps_t, messages_t):
        """out[r] = (1 + m_r n) * base^(e_r) mod n^2; ``messages_t``: ``[count, limbs(n)]`` (or wider) rows below n."""
        return self._fixed_base_run(table, _lib.MX_FIXEDBASE_ENCRYPT, exps_t, messages_t)

    def fixed_base_randomize_t(self, table: FixedBaseTable, exps_t, cts_t):
        """out[r] = c_r * base^(e_r) mod n^2; ``cts_t``: ``[count, limbs(n^2)]`` rows of any residues below n^2."""
        return self._fixed_base_run(table, _lib.MX_FIXEDBASE_RANDOMIZE, exps_t, cts_t)

    def fixed_base_exponent_rows(self, exponents, exp_bits: int):
        """Exponents -> device rows ``[count, ceil(exp_bits / 32)]``: a sequence of ints below ``2^exp_bits`` (ValueError
        otherwise), or a uint32 numpy array of that shape taken as it is (drawn bytes; the kernel masks the top bits),
        or an int32 tensor of that shape already on this engine's device (random_rows_t), returned as it is — ValueError
        if it lives on another device."""
        ewords = (int(exp_bits) + 31) // 32
        if _is_device_rows(exponents):
            if exponents.dim() != 2 or exponents.shape[1] != ewords or exponents.dtype != self.torch.int32:
                raise ValueError(f"int32 exponent rows of {ewords} words expected")
            if exponents.device != self.device:
                raise ValueError(f"the exponent rows were drawn on {exponents.device}, the operation runs on {self.device}")
            return exponents
        if isinstance(exponents, np.ndarray):
            if exponents.ndim != 2 or exponents.shape[1] != ewords:
                raise ValueError(f"exponent rows of {ewords} words expected")
            return self.to_device(exponents)
        vals = [int(e) for e in exponents]
        if any(e < 0 or e >> exp_bits for e in vals):
            raise ValueError(f"exponents must lie in [0, 2^{exp_bits})")
        return self.to_device(_limbs.pack(vals, ewords))

    def _fixed_base_ints(self, mode: int, exponents, operands, n: int, base: int, exp_bits: int, window: int) -> List[int]:
        if operands is not None and len(operands) != len(exponents):
            raise ValueError("one exponent per operand expected")
        if len(exponents) == 0:
            return []
        _check_modulus(n)
        table = self.fixed_base_table(n, base, exp_bits, window)
        e_t = self.fixed_base_exponent_rows(exponents, exp_bits)
        op_t = None
        if operands is not None:
            mod = n if mode == _lib.MX_FIXEDBASE_ENCRYPT else n * n          # messages modulo N, ciphertexts modulo N^2
            op_t = self._upload_ints(operands if isinstance(operands, list) else list(operands), _limbs.limbs_for(mod), mod)
        return self._download_ints(self._fixed_base_run(table, mode, e_t, op_t))

    @_int_args
    def fixed_base_power_batch(self, exponents, n: int, base: int, exp_bits: int, window: int = 0) -> List[int]:
        """[pow(base, e, n^2) for e in exponents] through the table of (n, base, exp_bits, window)."""
        return self._fixed_base_ints(_lib.MX_FIXEDBASE_POWER, exponents, None, n, base, exp_bits, window)

    @_int_args
    def fixed_base_encrypt_batch(self, messages: Sequence[int], exponents, n: int, base: int, exp_bits: int, window: int = 0) -> List[int]:
        """[(1 + (m mod n) n) * pow(base, e, n^2) mod n^2 for m, e] — Paillier encryption with g = n + 1 and the
        randomiser base^e (randomizer.py says what that randomiser is and is not).  Negative messages work as in encrypt_batch."""
        return self._fixed_base_ints(_lib.MX_FIXEDBASE_ENCRYPT, exponents, messages, n, base, exp_bits, window)

    @_int_args
    def fixed_base_randomize_batch(self, ciphertexts: Sequence[int], exponents, n: int, base: int, exp_bits: int, window: int = 0) -> List[int]:
        """[(c mod n^2) * pow(base, e, n^2) mod n^2 for c, e] — re-randomisation with the randomiser base^e."""
        return self._fixed_base_ints(_lib.MX_FIXEDBASE_RANDOMIZE, exponents, ciphertexts, n, base, exp_bits, window)

    # ------------------------------------------------------------------ modular multiplication / inversion / encryption
    @_int_args
    def mulmod_t(self, a_t, b_t, mod: int, out_t=None):
        """out[e] = a[e]*b[e] mod `mod`; int32 rows [batch, limbs]; out_t may alias an input."""
        batch, limbs = a_t.shape
        if tuple(b_t.shape) != (batch, limbs):
            raise ValueError("operands must have the same shape")
        h_mod = _limbs.pack_one(mod, limbs)
        if out_t is None:
            out_t = self.torch.empty_like(a_t)
        self._call("mx_mulmod_shared", a_t.data_ptr(), b_t.data_ptr(), out_t.data_ptr(), h_mod.ctypes.data, limbs, batch,
                   workspace=("mx_mulmod_workspace_bytes", limbs))
        return out_t

    @_int_args
    def mulmod_batch(self, a: Sequence[int], b: Sequence[int], mod: int, fixed_base=None) -> List[int]:
        if len(a) != len(b):
            raise ValueError("operands must have the same length")
        if len(a) == 0:
            return []
        _check_modulus(mod)
        limbs = _limbs.limbs_for(mod)
        at, bt = self._upload_ints(a, limbs, mod), self._upload_ints(b, limbs, mod)
        return self._download_ints(self._freshened(self.mulmod_t(at, bt, mod), fixed_base))

    DIRECT_MODINV_MAX = 4      # elements inverted directly (one wavefront each); longer batches use the product tree

    @_int_args
    def modinv_direct_t(self, x_t, mod: int):
        """Row-wise modular inverse on the device, one wavefront per row (mx_modinv): for the few
        values that need it (the root of the product tree, theta of a key).  Raises ValueError (like
        ``pow(v, -1, m)``) if some row is not invertible."""
        batch, limbs = x_t.shape
        _check_modulus(mod)
        h_mod = _limbs.pack_one(mod, limbs)
        out_t = self.torch.empty_like(x_t)
        status_t = self.torch.empty(batch, dtype=self.torch.uint8, device=self.device)
        self._call("mx_modinv", x_t.data_ptr(), out_t.data_ptr(), status_t.data_ptr(), h_mod.ctypes.data, limbs, batch,
                   workspace=("mx_modinv_workspace_bytes", limbs))
        if int(status_t.sum().item()) != 0:
            raise ValueError("base is not invertible for the given modulus")
        return out_t

    @_int_args
    def modinv_t(self, x_t, mod: int):
        """Row-wise modular inverse by Montgomery's trick as a product tree on the device: 3 modular
        multiplications per element in ~2 log2(batch) launches, and the root inverted on the device too
        (mx_modinv) — no host big-integer step (PSK:89-91 over a batch).
        Raises ValueError (like ``pow(v, -1, m)``) if some row is not invertible."""
        torch = self.torch
        levels = [x_t.contiguous()]
        while levels[-1].shape[0] > self.DIRECT_MODINV_MAX:
            cur = levels[-1]
            m = cur.shape[0]
            prod = self.mulmod_t(cur[0 : m - (m & 1) : 2].contiguous(), cur[1:m:2].contiguous(), mod)
            if m & 1:
                prod = torch.cat([prod, cur[m - 1 : m]], dim=0)
            levels.append(prod)
        inv = self.modinv_direct_t(levels[-1], mod)        # ValueError if not invertible
        for cur in reversed(levels[:-1]):
            m = cur.shape[0]
            half = m // 2
            left, right = cur[0 : 2 * half : 2].contiguous(), cur[1 : 2 * half : 2].contiguous()
            nxt = torch.empty_like(cur)
            nxt[0 : 2 * half : 2] = self.mulmod_t(inv[:half].contiguous(), right, mod)
            nxt[1 : 2 * half : 2] = self.mulmod_t(inv[:half].contiguous(), left, mod)
            if m & 1:
                nxt[m - 1] = inv[half]
            inv = nxt
        return inv

    @_int_args
    def modinv_batch(self, values: Sequence[int], mod: int, fixed_base=None) -> List[int]:
        """[mod_inv(v, mod) for v in values] (PSK:90 over a batch)."""
        if len(values) == 0:
            return []
        _check_modulus(mod)
        limbs = _limbs.limbs_for(mod)
        x_t = self._upload_ints(values, limbs, mod)
        return self._download_ints(self._freshened(self.modinv_t(x_t, mod), fixed_base))

    @_int_args
    def encrypt_batch(self, messages: Sequence[int], randomness: Sequence[int], n: int) -> List[int]:
        """Paillier encryption with g = n + 1:  c = (1 + m n) * r^n mod n^2 for every (m, r)."""
        return self._times_rn(messages, "message", randomness, n,
                              lambda limbs, n2: _limbs.pack([(1 + (m % n) * n) % n2 for m in messages], limbs))

    @_int_args
    def randomize_batch(self, ciphertexts: Sequence[int], randomness: Sequence[int], n: int) -> List[int]:
        """Re-randomisation of Paillier ciphertexts, c * r^n mod n^2 for every (c, r) — what the
        un-vendored scheme's ``randomize`` does before a ciphertext is sent (README.md:165-171 of the
        reference: a ciphertext must be fresh when it leaves); r^n through the N^2 pair kernel."""
        return self._times_rn(ciphertexts, "ciphertext", randomness, n,
                              lambda limbs, n2: _limbs.pack_reduced(ciphertexts, limbs, n2))

    def _times_rn(self, values, what: str, randomness, n: int, rows) -> List[int]:
        """[v * r^n mod n^2 for v, r]: r^n through the N^2 pair kernel, times the rows ``rows(limbs, n^2)`` packs of `values`."""
        if len(values) != len(randomness):
            raise ValueError(f"one randomness per {what} expected")
        if len(values) == 0:
            return []
        n2, limbs = _nsquare(n)
        rn_t = self.powmod_nsquare_t(self._upload_ints(randomness, limbs, n2), n, n)
        return self._download_ints(self.mulmod_t(rn_t, self.to_device(rows(limbs, n2)), n2, out_t=rn_t))

    # ------------------------------------------------------------------ randomness drawn on the device
    def chacha20_rows_t(self, key: Sequence[int], nonce: Sequence[int], counter0: int, count: int, bits: int,
                        row_words: Optional[int] = None):
        """``[count, row_words]`` int32 rows of the ChaCha20 keystream (mx_chacha20_rows, csrc/mx_chacha.hpp) for the
        eight key words, three nonce words and first block counter given: keystream word r * w + j in out[r][j] for
        j < w = ceil(bits / 32), the top word masked to `bits`, zero beyond w.  The raw kernel call — the nonce
        discipline that makes the rows fit for use as secrets is device_rng.DeviceRng's (random_rows_t)."""
        count, bits, counter0 = int(count), int(bits), int(counter0)
        words = (bits + 31) // 32
        row_words = words if row_words is None else int(row_words)
        if len(key) != 8 or len(nonce) != 3:
            raise ValueError("eight key words and three nonce words expected")
        if count < 0 or bits < 1 or row_words < words:
            raise ValueError("count >= 0 and 1 <= bits <= 32 * row_words expected")
        if not 0 <= counter0 <= 0xFFFFFFFF or counter0 + (count * words + 15) // 16 > 1 << 32:
            raise ValueError("the request does not fit the 32-bit block counter")
        out_t = self.torch.empty((count, row_words), dtype=self.torch.int32, device=self.device)
        if count:
            self._call("mx_chacha20_rows", (_ctypes.c_uint32 * 8)(*key), (_ctypes.c_uint32 * 3)(*nonce), counter0,
                       out_t.data_ptr(), count, row_words, bits)
        return out_t

    def random_rows_t(self, rng, count: int, bits: int, row_words: Optional[int] = None):
        """``count`` rows of ``bits`` random bits from the device generator `rng` (device_rng.DeviceRng), drawn on this
        engine's current stream: ``[count, row_words]`` int32, what the ``*_t`` functions take as exponents or bases."""
        return rng.rows_t(self, count, bits, row_words)

    @_int_args
    def encrypt_fresh_batch(self, messages: Sequence[int], n: int, rng, return_randomness: bool = False):
        """Paillier encryption with g = n + 1 and randomness of the library's own: c = (1 + m n) * r^n mod n^2 with r
        drawn on the device by `rng` (device_rng.DeviceRng) — ``encrypt_batch`` without the list of r.

        r is drawn as bits(n) + 64 random bits in a row of the width of n^2.  Since (r + k n)^n = r^n (mod n^2), the
        pair kernel computes (r mod n)^n without a reduction, and r mod n is uniform on [0, n) up to a bias below 2^-64.
        ValueError for an n so small that bits(n) + 64 > bits(n^2) - 1 (r must stay below n^2).

        NO coprimality check is made: r mod n shares a factor with n with probability about 2^(1 - bits(n) / 2) (it is
        then a multiple of p or q, or 0), the ciphertext would not decrypt, and the event would factor n — at the key
        lengths in use it does not happen.  The reference's scheme rejects such an r; a caller who must do the same
        asks for the randomness and checks it.

        ``return_randomness``: the result is ``(ciphertexts, [r, ...])`` with the drawn r as ints (not reduced modulo
        n) — for tests and for callers who must log their randomness."""
        return self._fresh_rn(messages, n, rng, return_randomness,
                              lambda limbs, n2: _limbs.pack([(1 + (m % n) * n) % n2 for m in messages], limbs))

    @_int_args
    def randomize_fresh_batch(self, ciphertexts: Sequence[int], n: int, rng, return_randomness: bool = False):
        """Re-randomisation c * r^n mod n^2 with r drawn on the device by `rng` — ``randomize_batch`` without the list
        of r; what is drawn, what is not checked and ``return_randomness`` as in encrypt_fresh_batch."""
        return self._fresh_rn(ciphertexts, n, rng, return_randomness,
                              lambda limbs, n2: _limbs.pack_reduced(ciphertexts, limbs, n2))

    def _fresh_rn(self, values, n: int, rng, return_randomness: bool, rows):
        n2, limbs = _nsquare(n)
        r_bits = n.bit_length() + 64
        if r_bits > n2.bit_length() - 1:
            raise ValueError(f"a modulus of {n.bit_length()} bits leaves no room for 64 extra bits of randomness below n^2")
        if len(values) == 0:
            return ([], []) if return_randomness else []
        r_t = self.random_rows_t(rng, len(values), r_bits, limbs)
        rn_t = self.powmod_nsquare_t(r_t, n, n)      # leaves r_t as it is; the rows are packed while it runs, as in _times_rn
        out = self._download_ints(self.mulmod_t(rn_t, self.to_device(rows(limbs, n2)), n2, out_t=rn_t))
        return (out, self._download_ints(r_t)) if return_randomness else out

    # ------------------------------------------------------------------ Shamir field of the key generation
    @_int_args
    def shamir_fma_t(self, a_t, b_t, c_t, prime: int, out_t=None):
        """out[e] = (a[e]*b[e] + c[e]) mod prime — this party's share of every candidate modulus
        (`p * q` then `+= zero`, DK:1274-1277); int32 rows [batch, limbs]."""
        batch, limbs = a_t.shape
        if tuple(b_t.shape) != (batch, limbs) or tuple(c_t.shape) != (batch, limbs):
            raise ValueError("operands must have the same shape")
        _check_modulus(prime)
        h_mod = _limbs.pack_one(prime, limbs)
        if out_t is None:
            out_t = self.torch.empty_like(a_t)
        self._call("mx_fma_mod", a_t.data_ptr(), b_t.data_ptr(), c_t.data_ptr(), out_t.data_ptr(), h_mod.ctypes.data, limbs, batch,
                   workspace=("mx_field_workspace_bytes", limbs, 0))
        return out_t

    @_int_args
    def shamir_lincomb_t(self, x_t, coeffs: Sequence[int], prime: int, out_t=None):
        """out[e] = sum_t coeffs[t] * x[t][e] mod prime; x_t int32 [terms, batch, limbs].  With the
        Lagrange coefficients at 0 this is `candidate_n.reconstruct()` (DK:1284) for a whole round; the
        result rows are the candidate moduli, ready for sieve_t / biprime_v_t on the device."""
        terms, batch, limbs = x_t.shape
        if len(coeffs) != terms:
            raise ValueError("one coefficient per term expected")
        _check_modulus(prime)
        h_mod = _limbs.pack_one(prime, limbs)
        h_cf = _limbs.pack([c % prime for c in coeffs], limbs)
        if out_t is None:
            out_t = self.torch.empty((batch, limbs), dtype=self.torch.int32, device=self.device)
        self._call("mx_lincomb_mod", x_t.data_ptr(), h_cf.ctypes.data, out_t.data_ptr(), h_mod.ctypes.data, limbs, terms, batch,
                   workspace=("mx_field_workspace_bytes", limbs, terms))
        return out_t

    @_int_args
    def shamir_fma_batch(self, a: Sequence[int], b: Sequence[int], c: Sequence[int], prime: int) -> List[int]:
        if not (len(a) == len(b) == len(c)):
            raise ValueError("operands must have the same length")
        if len(a) == 0:
            return []
        limbs = _limbs.limbs_for(prime)
        ts = [self._upload_ints(col, limbs, prime) for col in (a, b, c)]
        return self._download_ints(self.shamir_fma_t(ts[0], ts[1], ts[2], prime))

    @_int_args
    def shamir_lincomb_batch(self, columns: Sequence[Sequence[int]], coeffs: Sequence[int], prime: int) -> List[int]:
        """[sum_t coeffs[t] * columns[t][e] mod prime for e]; one column per term."""
        if len(columns) == 0 or len(columns[0]) == 0:
            return []
        if any(len(c) != len(columns[0]) for c in columns):
            raise ValueError("columns must have the same length")
        limbs = _limbs.limbs_for(prime)
        x = np.stack([_limbs.pack_reduced(col, limbs, prime) for col in columns])
        return self._download_ints(self.shamir_lincomb_t(self.to_device(x), coeffs, prime))

    # ------------------------------------------------------------------ additive shares and their sharings (DK:718-853)
    def prime_candidates_t(self, count: int, prime_length: int, first_party: bool, rng=None, random_t=None,
                           row_words: Optional[int] = None):
        """``[count, row_words]`` int32 rows of the additive shares 2^(L-1) + (r << 2) + m4 of a round's prime candidates
        (`_generate_prime_candidate`, DK:874-875): L = `prime_length`, m4 = 3 for the first party and 0 for the others,
        r a row of L - 3 random bits — ``random_t`` (``[count, ceil((L - 3) / 32)]``, zero above bit L - 3) or ONE call
        ``rng.rows_t(self, count, L - 3)`` of a device_rng.DeviceRng.  ``row_words`` defaults to ceil(L / 32); wider rows
        are zero-filled.  ValueError — nothing launched, no call number taken — for prime_length < 8, rows narrower than
        L bits, neither or both of `rng` and `random_t`, or a `random_t` of another shape."""
        from . import shamir as _shamir

        count, prime_length = int(count), int(prime_length)
        in_words, row_words = _shamir.check_candidate_args(count, prime_length, row_words)
        if (rng is None) == (random_t is None):
            raise ValueError("exactly one of rng and random_t expected")
        if random_t is not None and (tuple(random_t.shape) != (count, in_words) or not random_t.is_contiguous()):
            raise ValueError(f"random_t must be contiguous rows of the shape ({count}, {in_words})")
        if random_t is None:
            random_t = rng.rows_t(self, count, prime_length - 3)
        out_t = self._empty_rows(row_words, count)
        if count:
            self._call("mx_share_candidates", random_t.data_ptr(), out_t.data_ptr(), count, prime_length, 1 if first_party else 0, row_words)
        return out_t

    def shamir_share_t(self, secrets_t, prime: int, degree: int, points: Sequence[int], batch: Optional[int] = None, rng=None,
                       draws_t=None, out_t=None):
        """Shamir sharings of a batch of secrets modulo `prime` (`ShamirVariable.share()`, utils.py:253-260, for every
        candidate of a round): ``out[j][e] = secrets[e] + sum_{k=1..degree} a_k[e] * points[j]^k mod prime`` as int32 rows
        ``[len(points), batch, limbs]`` of canonical residues — party j's rows contiguous, the layout shamir_lincomb_t
        reads.  ``secrets_t``: ``[batch, limbs]`` rows below the prime, or None with ``batch=`` for a sharing of zero.

        The coefficients are a_k[e] = D mod prime for draws D of bits(prime) + 64 bits: ``draws_t`` ``[degree, batch,
        cw]`` with cw = ceil((bits(prime) + 64) / 32), or ONE call ``rng.rows_t(self, degree * batch, bits(prime) + 64,
        cw)`` whose row (k - 1) * batch + e is the draw of coefficient k of element e.

        ValueError — nothing launched, no call number taken — for degree < 1 (or above MX_SHARE_MAX_DEGREE), points that
        are not distinct integers in [1, 2^16), fewer than degree + 1 points, an even prime, neither or both of `rng`
        and `draws_t`, or rows of another shape."""
        from . import shamir as _shamir

        prime, degree = int(prime), int(degree)
        points = _shamir.check_share_args(prime, degree, points)
        if secrets_t is not None:
            if secrets_t.dim() != 2 or (batch is not None and int(batch) != secrets_t.shape[0]):
                raise ValueError("secrets_t must be [batch, limbs]")
            batch, limbs = secrets_t.shape
        else:
            if batch is None:
                raise ValueError("a sharing of zero needs batch=")
            batch, limbs = int(batch), (_limbs.limbs_for(prime) if out_t is None else out_t.shape[-1])
        if batch < 0 or limbs < _limbs.limbs_for(prime):
            raise ValueError("rows narrower than the prime")
        bits = prime.bit_length() + 64
        cw = (bits + 31) // 32
        if (rng is None) == (draws_t is None):
            raise ValueError("exactly one of rng and draws_t expected")
        if draws_t is not None and tuple(draws_t.shape) != (degree, batch, cw):
            raise ValueError(f"draws_t must have the shape ({degree}, {batch}, {cw})")
        if out_t is not None and tuple(out_t.shape) != (len(points), batch, limbs):
            raise ValueError(f"out_t must have the shape ({len(points)}, {batch}, {limbs})")
        if any(x is not None and not x.is_contiguous() for x in (secrets_t, draws_t, out_t)):
            raise ValueError("contiguous rows expected")
        if draws_t is None:
            draws_t = rng.rows_t(self, degree * batch, bits, cw)
        if out_t is None:
            out_t = self.torch.empty((len(points), batch, limbs), dtype=self.torch.int32, device=self.device)
        if batch:
            h_mod = _limbs.pack_one(prime, limbs)
            h_points = np.asarray(points, dtype="<u4")
            self._call("mx_shamir_share", secrets_t.data_ptr() if secrets_t is not None else None, draws_t.data_ptr(),
                       h_points.ctypes.data, len(points), degree, out_t.data_ptr(), h_mod.ctypes.data, limbs, batch,
                       workspace=("mx_share_workspace_bytes", limbs, len(points)))
        return out_t

    def prime_candidates_batch(self, count: int, prime_length: int, first_party: bool, rng) -> List[int]:
        """prime_candidates_t with the candidates as Python ints."""
        return self._download_ints(self.prime_candidates_t(count, prime_length, first_party, rng=rng))

    def shamir_share_batch(self, secrets: Optional[Sequence[int]], prime: int, degree: int, points: Sequence[int], rng,
                           batch: Optional[int] = None) -> Dict[int, List[int]]:
        """shamir_share_t over Python ints: ``{point: [share of every secret]}``; ``secrets=None`` with ``batch=`` shares
        zero.  ValueError for a secret outside [0, prime)."""
        from . import shamir as _shamir

        prime = int(prime)
        points = _shamir.check_share_args(prime, int(degree), points)
        limbs = _limbs.limbs_for(prime)
        secrets_t = None
        if secrets is not None:
            secrets = [int(s) for s in secrets]
            if any(not 0 <= s < prime for s in secrets):
                raise ValueError("secrets must lie in [0, prime)")
            if batch is not None and int(batch) != len(secrets):
                raise ValueError("batch differs from the number of secrets")
            batch = len(secrets)
            if batch:
                secrets_t = self.to_device(_limbs.pack(secrets, limbs))
        if batch is None:
            raise ValueError("a sharing of zero needs batch=")
        if not batch:
            return {x: [] for x in points}
        out_t = self.shamir_share_t(secrets_t, prime, degree, points, batch=batch, rng=rng)
        vals = self._download_ints(out_t.view(len(points) * batch, limbs))
        return {x: vals[j * batch : (j + 1) * batch] for j, x in enumerate(points)}

    # ------------------------------------------------------------------ jointly random generators (DK:1001-1054)
    def _generator_operands(self, mods, group_size: int, limbs: Optional[int] = None):
        """(device moduli rows [S, limbs], host copy or None, max bits, limbs) of the generator entry points.  `mods`: a
        sequence of ints (checked odd and >= 3, uploaded, and handed to the library a second time as the host rows it
        checks) or a device (rows, bits) pair; `limbs` defaults to the rows of the widest modulus."""
        if int(group_size) < 1:
            raise ValueError("group_size must be at least 1")
        if _is_device_pair(mods):
            rows_t, bits = mods[0], int(mods[1])
            if limbs is not None and rows_t.shape[1] != limbs:
                raise ValueError("device moduli must have the row width of the operands")
            if not rows_t.is_contiguous():
                raise ValueError("contiguous rows expected")
            if not 2 <= bits <= 32 * rows_t.shape[1]:
                raise ValueError("modulus wider than the limb rows")
            return rows_t, None, bits, rows_t.shape[1]
        mods = [int(m) for m in mods]
        for m in mods:
            _check_modulus(m)
        bits = _limbs.max_bits(mods)
        limbs = _limbs.limbs_for_bits(bits) if limbs is None else int(limbs)
        if bits > 32 * limbs:
            raise ValueError("modulus wider than the limb rows")
        h_mods = _limbs.pack(mods, limbs)
        return self.to_device(h_mods), h_mods, bits, limbs

    def generator_shares_t(self, mods, group_size: int, rng=None, draws_t=None, out_t=None):
        """This party's additive shares of the jointly random generators of a round's biprimality tests
        (`__biprime_test_g_generation`, DK:1030-1044), for S candidate moduli with `group_size` = G generators each:
        ``out[c * G + k] = D[c * G + k] mod mods[c]`` as int32 rows ``[S * G, limbs]`` of canonical residues.

        The draws D have B + 64 bits, B the bit length of the widest modulus: ``draws_t`` ``[S * G, cw]`` with
        cw = ceil((B + 64) / 32), or ONE call ``rng.rows_t(self, S * G, B + 64, cw)`` whose row c * G + k is the draw of
        generator k of candidate c.  A share is uniform on [0, N_c) up to a bias below 2^-64 (the convention of
        shamir_share_t and encrypt_fresh_batch).  The reference draws ``randint(0, N_c)`` on [0, N_c] INCLUSIVE; only
        the sum of the parties' shares modulo N_c is ever used, so parties on either path interoperate.

        ``mods``: a sequence of ints or a device ``(rows, bits)`` pair.  ValueError — nothing launched, no call number
        taken — for group_size < 1, an even modulus or one below 3, neither or both of `rng` and `draws_t`, or rows of
        another shape."""
        group_size = int(group_size)
        mods_t, h_mods, bits, limbs = self._generator_operands(mods, group_size, None if out_t is None else out_t.shape[-1])
        groups = mods_t.shape[0]
        total = groups * group_size
        cw = (bits + 64 + 31) // 32
        if (rng is None) == (draws_t is None):
            raise ValueError("exactly one of rng and draws_t expected")
        if draws_t is not None and tuple(draws_t.shape) != (total, cw):
            raise ValueError(f"draws_t must have the shape ({total}, {cw})")
        if out_t is not None and tuple(out_t.shape) != (total, limbs):
            raise ValueError(f"out_t must have the shape ({total}, {limbs})")
        if any(x is not None and not x.is_contiguous() for x in (draws_t, out_t)):
            raise ValueError("contiguous rows expected")
        if out_t is None:
            out_t = self._empty_rows(limbs, total)
        if total:
            if draws_t is None:
                draws_t = rng.rows_t(self, total, bits + 64, cw)
            self._call("mx_generator_shares", draws_t.data_ptr(), out_t.data_ptr(), mods_t.data_ptr(),
                       h_mods.ctypes.data if h_mods is not None else None, limbs, bits, groups, group_size,
                       workspace=("mx_generator_workspace_bytes", limbs, groups))
        return out_t

    def generator_sum_t(self, shares_t, mods, group_size: int, out_t=None):
        """The generators themselves (DK:1051-1053, ``AdditiveVariable.reconstruct``): ``out[c * G + k] = sum_j
        shares[j][c * G + k] mod mods[c]`` as canonical residues, ``[S * G, limbs]`` — the rows biprime_v_t reads.
        ``shares_t``: ``[parties, S * G, limbs]``; any row is a valid share (N_c itself, unreduced values).  ValueError —
        nothing launched — for group_size < 1, an even modulus, no party or more than MX_GEN_MAX_PARTIES, or rows of
        another shape."""
        group_size = int(group_size)
        if shares_t.dim() != 3 or not shares_t.is_contiguous():
            raise ValueError("shares_t must be contiguous rows [parties, S * G, limbs]")
        parties, total, limbs = shares_t.shape
        if not 1 <= parties <= _lib.MX_GEN_MAX_PARTIES:
            raise ValueError(f"1 .. {_lib.MX_GEN_MAX_PARTIES} parties expected")
        mods_t, h_mods, bits, _ = self._generator_operands(mods, group_size, limbs)
        groups = mods_t.shape[0]
        if total != groups * group_size:
            raise ValueError("shares_t must hold groups * group_size rows per party")
        if out_t is not None and (tuple(out_t.shape) != (total, limbs) or not out_t.is_contiguous()):
            raise ValueError(f"out_t must be contiguous rows of the shape ({total}, {limbs})")
        if out_t is None:
            out_t = self._empty_rows(limbs, total)
        if total:
            self._call("mx_generator_sum", shares_t.data_ptr(), parties, out_t.data_ptr(), mods_t.data_ptr(),
                       h_mods.ctypes.data if h_mods is not None else None, limbs, bits, groups, group_size,
                       workspace=("mx_generator_workspace_bytes", limbs, groups))
        return out_t

    def generator_shares_batch(self, mods: Sequence[int], group_size: int, rng, mods_rows: Any = None, keep_rows: bool = False):
        """generator_shares_t with the shares as Python ints, one list of `group_size` per modulus (what the reference
        exchanges, DK:1046-1049).  ``mods_rows``: the handle of exactly these moduli on the device; with ``keep_rows``
        the result is ``(lists, rows)`` where ``rows`` keeps the shares on the device for generator_sum_batch."""
        mods = [int(m) for m in mods]
        group_size = int(group_size)
        if group_size < 1:
            raise ValueError("group_size must be at least 1")
        for m in mods:
            _check_modulus(m)
        if not mods:
            return ([], None) if keep_rows else []
        limbs = _limbs.limbs_for_bits(_limbs.max_bits(mods))
        mods_op = mods_rows.operand(self, len(mods), limbs) if mods_rows is not None else mods
        rows_t = self.generator_shares_t(mods_op, group_size, rng=rng)
        lists = self._fetched_ints("generator_shares", rows_t, groups=([group_size] * len(mods), group_size))
        return (lists, rows_t) if keep_rows else lists

    def generator_sum_batch(self, shares: Sequence[Any], mods: Sequence[int], group_size: int, mods_rows: Any = None,
                            keep_rows: bool = False):
        """generator_sum_t over Python ints: ``shares`` holds one entry per party, each one list of `group_size` shares per
        modulus — or the device rows generator_shares_batch kept for that party.  A negative share or one wider than
        the rows is reduced with ``%`` on the host before packing, so the result is always the reference's
        ``sum(shares) % N``.  Returns the generators nested per modulus, or with ``keep_rows`` the device rows alone
        (``[S * G, limbs]``, what biprime_v_t reads: nothing is downloaded)."""
        mods = [int(m) for m in mods]
        group_size = int(group_size)
        if group_size < 1:
            raise ValueError("group_size must be at least 1")
        if not 1 <= len(shares) <= _lib.MX_GEN_MAX_PARTIES:
            raise ValueError(f"1 .. {_lib.MX_GEN_MAX_PARTIES} parties expected")
        for m in mods:
            _check_modulus(m)
        if any(not _is_device_rows(col) and (len(col) != len(mods) or any(len(row) != group_size for row in col)) for col in shares):
            raise ValueError("every party needs group_size shares per modulus")
        if not mods:
            return None if keep_rows else []
        limbs = _limbs.limbs_for_bits(_limbs.max_bits(mods))
        total = len(mods) * group_size
        shares_t = self.torch.empty((len(shares), total, limbs), dtype=self.torch.int32, device=self.device)
        for j, col in enumerate(shares):
            if _is_device_rows(col):
                if tuple(col.shape) != (total, limbs):
                    raise ValueError("the kept share rows do not belong to these candidates")
                shares_t[j].copy_(col)
            else:                      # (a staging buffer per party: the copies are asynchronous)
                shares_t[j].copy_(self._packed_rows(f"generator_shares_{j}", col, limbs, mods, nested=group_size), non_blocking=True)
        mods_op = mods_rows.operand(self, len(mods), limbs) if mods_rows is not None else mods
        g_t = self.generator_sum_t(shares_t, mods_op, group_size)
        if keep_rows:
            self.synchronize()         # the staging buffers are free again
            return g_t
        return self._fetched_ints("generators", g_t, groups=([group_size] * len(mods), group_size))

    @_int_args
    def shamir_reconstruct_sieve_batch(self, columns: Sequence[Sequence[int]], coeffs: Sequence[int], prime: int,
                                       primes: Sequence[int], keep_rows: bool = False):
        """The candidate moduli of a round and their small-prime verdicts in one device pass
        (DK:1284 + DK:1288-1292): reconstruction rows go straight into the sieve; only the verdict bytes
        and the moduli of the SURVIVORS (~2 % of a round) come back to the host.
        Returns (has_small_divisor per candidate, {candidate index: modulus} for the survivors); with
        ``keep_rows`` a third value: the survivors' moduli as device rows (in index order, an opaque
        handle for ``biprime_v_batch`` / ``biprime_verdict_columns``: the round's later steps take their moduli
        from it instead of packing them again), None if nothing survived."""
        if len(columns) == 0 or len(columns[0]) == 0:
            return ([], {}, None) if keep_rows else ([], {})
        limbs = _limbs.limbs_for(prime)
        # the parties' columns are packed side by side into ONE page-locked buffer (no per-column array, no np.stack of
        # 5 x 65 536 x 2100-bit shares, no pageable copy: 38 -> 28 ms of host time per 65 536-candidate round)
        ncols, count = len(columns), len(columns[0])
        if any(len(col) != count for col in columns):
            raise ValueError("columns must have the same length")
        pin = self._pinned("shares", ncols * count, limbs)
        rows = pin.numpy().view(np.uint32)
        for i, col in enumerate(columns):
            try:
                _limbs.pack_into(col if isinstance(col, (list, tuple)) else list(col), limbs, rows, i * count)
            except ValueError:                      # a share that does not fit the field's rows, or a negative one
                rows[i * count : (i + 1) * count] = _limbs.pack_reduced(col, limbs, prime)
        _limbs.reduce_rows(rows, prime)
        x_t = pin.to(self.device, non_blocking=True).view(ncols, count, limbs)
        mods_t = self.shamir_lincomb_t(x_t, coeffs, prime)
        primes = [int(q) for q in primes]
        if len(primes) == 0:
            bad = np.zeros(mods_t.shape[0], dtype=np.uint8)
        else:
            bad = self.sieve_t(mods_t, primes).cpu().numpy()
        keep = np.nonzero(bad == 0)[0]
        survivors: Dict[int, int] = {}
        rows = None
        if len(keep):
            idx = self.torch.from_numpy(keep.astype(np.int64)).to(self.device)
            rows_t = mods_t.index_select(0, idx)
            vals = self._download_ints(rows_t)
            survivors = {int(k): v for k, v in zip(keep, vals)}
            rows = _ModulusRows(rows_t, _limbs.max_bits(vals))
        flags = bad.astype(bool).tolist()
        return (flags, survivors, rows) if keep_rows else (flags, survivors)

    # ------------------------------------------------------------------ Jacobi symbol
    def jacobi_t(self, values_t, mods, group_size: int, out_t=None, first: int = 0, count: Optional[int] = None,
                 skip_counts_t=None, skip_threshold: int = 0):
        """int8 [groups*group_size]: Jacobi symbol (values[g*group_size+k] / mods[g]) (DK:1089).
        `mods`: sequence of ints or a device-resident (rows, max bits) pair.  With first / count only
        the rows [first, first+count) of every group are evaluated (the other entries of out_t are left
        as they are); groups with skip_counts_t[g] >= skip_threshold are skipped."""
        total, limbs = values_t.shape
        if not _is_device_pair(mods):
            _check_jacobi_moduli(mods)
        mods_t, _ = self._mods_operand(mods, limbs, odd_only=False)
        groups = mods_t.shape[0]
        if total != groups * group_size:
            raise ValueError("values must hold groups*group_size rows")
        if count is None:
            count = group_size - first
        if out_t is None:
            full = first == 0 and count == group_size and skip_counts_t is None
            out_t = (self.torch.empty if full else self.torch.zeros)(total, dtype=self.torch.int8, device=self.device)
        self._call("mx_jacobi_dev_range", values_t.data_ptr(), out_t.data_ptr(), mods_t.data_ptr(), limbs, groups, group_size, first,
                   count, skip_counts_t.data_ptr() if skip_counts_t is not None else None, skip_threshold)
        return out_t

    @_int_args
    def jacobi_batch(self, values: Sequence[Sequence[int]], mods: Sequence[int]) -> List[List[int]]:
        """[[jacobi_symbol(v, mods[g]) for v in values[g]] for g]; ragged groups are padded."""
        groups = len(mods)
        if groups == 0:
            return []
        _check_jacobi_moduli(mods)
        gsize = max(len(v) for v in values)
        if gsize == 0:
            return [[] for _ in values]
        limbs = _limbs.limbs_for_bits(_limbs.max_bits(mods))
        flat = []
        for vs in values:
            flat.extend(vs)
            flat.extend([0] * (gsize - len(vs)))
        out = self.jacobi_t(self._upload_ints(flat, limbs, list(mods)), list(mods), gsize)
        arr = out.cpu().numpy()
        return [[int(x) for x in arr[g * gsize : g * gsize + len(values[g])]] for g in range(groups)]

    def select_first_t(self, rows_t, flags_t, group_size: int, keep: int):
        """rows_t int32 [groups*group_size, limbs], flags_t int8 [groups*group_size] -> (int32
        [groups*keep, limbs] with the first `keep` flag==1 rows of every group, int32 counts [groups])."""
        total, limbs = rows_t.shape
        groups = total // group_size
        out_t = self.torch.empty((groups * keep, limbs), dtype=self.torch.int32, device=self.device)
        cnt_t = self.torch.empty(groups, dtype=self.torch.int32, device=self.device)
        self._call("mx_select_first", rows_t.data_ptr(), flags_t.data_ptr(), out_t.data_ptr(), cnt_t.data_ptr(), limbs, groups,
                   group_size, keep)
        return out_t, cnt_t

    JACOBI_ONE_LAUNCH_SYMBOLS = 16384        # 256 wavefronts: a quarter of the SIMDs

    def biprime_v_t(self, g_t, mods, exps, group_size: int, keep: int):
        """Tensor-level v-calculation of DK:1084-1099 for many candidates, nothing leaving the device:
        g_t int32 [groups*group_size, limbs] (the jointly random generators, reduced) -> (v rows int32
        [groups*keep, limbs], counts int32 [groups]): Jacobi symbols of all generators, selection of the
        first `keep` with symbol 1 (in order), v = g^exp mod N for those; rows beyond a candidate's count
        are the modexp of a zero row and are ignored by the caller."""
        limbs = g_t.shape[1]
        mods_op = self._mods_operand(mods, limbs)
        # The selection stops at `keep` generators with symbol 1 (DK:1086) and a symbol is 1 for about
        # half of them: the first 2.6 * keep generators yield `keep` ones for > 99 % of the candidates,
        # and the tail of the list is evaluated only for the candidates where they did not.
        head = min(group_size, (13 * keep + 4) // 5)
        # ... unless the launch is so small that it lasts as long as ONE thread's symbol whatever its size (a round at the
        # reference's batch sizes: 0.8 ms for 1 .. 20 candidates x 104 or x 160 symbols at key_length 2048,
        # profiles/r05_keygen_round_small.txt): a second launch would only add its latency
        if mods_op[0].shape[0] * group_size <= self.JACOBI_ONE_LAUNCH_SYMBOLS:
            head = group_size

        def filter_and_select():
            j_t = self.jacobi_t(g_t, mods_op, group_size, first=0, count=head)
            sel_t, cnt_t = self.select_first_t(g_t, j_t, group_size, keep)
            if head < group_size:
                self.jacobi_t(g_t, mods_op, group_size, out_t=j_t, first=head, count=group_size - head,
                              skip_counts_t=cnt_t, skip_threshold=keep)
                sel_t, cnt_t = self.select_first_t(g_t, j_t, group_size, keep)
            return sel_t, cnt_t

        sel_t, cnt_t = self._small(filter_and_select)
        v_t = self.powmod_multi_t(sel_t, mods_op, exps, keep)
        return v_t, cnt_t

    @_int_args
    def biprime_v_batch(
        self, g_values: Sequence[Sequence[int]], exps: Sequence[int], mods: Sequence[int], keep: int,
        mods_rows: Any = None, keep_rows: bool = False, g_rows: Any = None,
    ):
        """The whole v-calculation of DK:1084-1099 for many candidates on the device: Jacobi symbols of
        all generators, selection of the first `keep` with symbol 1, v = g^exp mod N for those.
        Returns per candidate the list of v values (shorter than `keep` if fewer symbols were 1).
        `mods_rows`: the handle ``shamir_reconstruct_sieve_batch(..., keep_rows=True)`` returned for exactly these
        moduli — they are then not packed and uploaded again.  With ``keep_rows`` the result is
        ``(lists, rows)`` where ``rows`` keeps this party's v values on the device for ``biprime_verdict_columns``.
        ``g_rows`` = (device rows ``[groups * group_size, limbs]`` of reduced generators, group_size), what
        ``generator_sum_batch(..., keep_rows=True)`` returned for these moduli: `g_values` is then not read, and nothing
        is packed or uploaded for the generators."""
        groups = len(mods)
        if groups == 0:
            return ([], None) if keep_rows else []
        for m in mods:          # the int moduli are passed either way: an even N reconstructed from malformed shares (the
            _check_modulus(m)   # sieve's list starts at 3) must raise here, not reach the Montgomery and Jacobi kernels
        gsize = int(g_rows[1]) if g_rows is not None else max(len(g) for g in g_values)
        if gsize == 0 or keep == 0:
            return ([[] for _ in mods], None) if keep_rows else [[] for _ in mods]
        limbs = _limbs.limbs_for_bits(_limbs.max_bits(mods))
        if g_rows is not None:
            g_t = g_rows[0]
            if tuple(g_t.shape) != (groups * gsize, limbs):
                raise ValueError("the kept generator rows do not belong to these candidates")
        else:
            # one list per candidate straight into the staging buffer (short lists zero padded: symbol (0/N) = 0, never selected)
            g_t = self._staged_rows("generators", g_values, limbs, mods, nested=gsize)
        mods_op = mods_rows.operand(self, groups, limbs) if mods_rows is not None else mods
        v_t, cnt_t = self.biprime_v_t(g_t, mods_op, exps, gsize, keep)
        counts = cnt_t.cpu().numpy()
        lists = self._fetched_ints("v", v_t, groups=(counts.tolist(), keep))      # per candidate, built in one pass
        return (lists, _VRows(v_t, counts, keep)) if keep_rows else lists

    # ------------------------------------------------------------------ sieve
    @_int_args
    def sieve_t(self, cands_t, primes: Sequence[int], out_t=None):
        """uint8 [batch]: 1 iff some prime divides candidate e (distributed_keygen.py:1197-1209)."""
        batch, limbs = cands_t.shape
        h_primes = np.ascontiguousarray(np.asarray(list(primes), dtype=np.uint32))
        if out_t is None:
            out_t = self.torch.empty(batch, dtype=self.torch.uint8, device=self.device)
        self._call("mx_sieve", cands_t.data_ptr(), out_t.data_ptr(), h_primes.ctypes.data, len(h_primes), limbs, batch,
                   workspace=("mx_sieve_workspace_bytes", limbs, len(h_primes)))
        return out_t

    @_int_args
    def sieve_batch(self, candidates: Sequence[int], primes: Sequence[int]) -> List[bool]:
        """[__small_prime_divisors_test(primes, n) for n in candidates]."""
        if len(candidates) == 0:
            return []
        primes = [int(p) for p in primes]
        if len(primes) == 0:
            return [False] * len(candidates)
        if any(c < 0 for c in candidates):
            raise ValueError("candidates must be non-negative")
        limbs = _limbs.limbs_for_bits(_limbs.max_bits(candidates))
        out = self.sieve_t(self.to_device(_limbs.pack(candidates, limbs)), primes)
        return [bool(x) for x in out.cpu().numpy()]

    # ------------------------------------------------------------------ Miller-Rabin and the prime search (primes.py)
    def mr_split_t(self, cands_t, bits: Optional[int] = None, _checked: bool = False):
        """n - 1 = 2^s d, d odd, for S odd candidates n >= 3 as int32 rows ``[S, limbs]`` (of any mix of bit lengths):
        ``(d_t [S, limbs], s_t int32 [S])`` (mx_mr_split, csrc/mx_mr.hpp).  ValueError — nothing launched — for an even
        candidate, one below 3 or rows of another shape."""
        rows, limbs, bits = self._mr_candidates(cands_t, bits, checked=_checked)
        d_t = self._empty_rows(limbs, rows)
        s_t = self.torch.empty(rows, dtype=self.torch.int32, device=self.device)
        if rows:
            self._call("mx_mr_split", cands_t.data_ptr(), None, d_t.data_ptr(), s_t.data_ptr(), limbs, bits, rows)
        return d_t, s_t

    def miller_rabin_t(self, cands_t, bases_t, group_size: int, out_t=None, bits: Optional[int] = None, _checked: bool = False):
        """The strong-pseudoprime test of S candidates to `group_size` = G bases each: uint8 ``[S * G]``, 1 where the
        round of candidate c to the base ``bases_t[c * G + k]`` passes.  ``bases_t``: canonical residues ``[S * G,
        limbs]``, for example ``generator_shares_t((cands_t, bits), G, rng)``; a base that is 0 modulo its candidate
        tests nothing and passes, 1 and n - 1 pass by themselves.  Three launches: mr_split_t, the generic modexp
        b^d mod n with one modulus and one exponent per group (powmod_multi_t), and the witness loop (mx_mr_tail).
        ``bits``: the bit length of the widest candidate, 32 * limbs when not given.  ValueError — nothing launched —
        for an even candidate, one below 3, group_size < 1 or rows of another shape."""
        group_size = int(group_size)
        if group_size < 1:
            raise ValueError("group_size must be at least 1")
        rows, limbs, bits = self._mr_candidates(cands_t, bits, checked=_checked)
        total = rows * group_size
        if not _is_device_rows(bases_t) or tuple(bases_t.shape) != (total, limbs) or not bases_t.is_contiguous():
            raise ValueError(f"bases_t must be contiguous rows of the shape ({total}, {limbs})")
        out_t = self._flags_out(out_t, total)
        if total:
            d_t, s_t = self.mr_split_t(cands_t, bits, _checked=True)
            x0_t = self.powmod_multi_t(bases_t, (cands_t, bits), (d_t, bits), group_size)
            self._call("mx_mr_tail", x0_t.data_ptr(), bases_t.data_ptr(), s_t.data_ptr(), out_t.data_ptr(), cands_t.data_ptr(),
                       None, limbs, bits, rows, group_size)
        return out_t

    def miller_rabin_base2_t(self, cands_t, bits: Optional[int] = None, out_t=None, _checked: bool = False):
        """The strong-pseudoprime test to the base 2 from the candidates alone: uint8 ``[S]`` (mx_mr_base2: one launch,
        one squaring and one selected doubling per bit of `bits`, no table — primes.py has the side-channel note).
        ``bits``: the bit length of the widest candidate, 32 * limbs when not given.  ValueError — nothing launched —
        for an even candidate, one below 3 or rows of another shape."""
        rows, limbs, bits = self._mr_candidates(cands_t, bits, checked=_checked)
        out_t = self._flags_out(out_t, rows)
        if rows:
            self._call("mx_mr_base2", cands_t.data_ptr(), None, out_t.data_ptr(), limbs, bits, rows)
        return out_t

    # ------------------------------------------------------------------ safe primes p = 2h + 1 (primes.py)
    def safe_sieve_t(self, halves_t, primes: Sequence[int], out_t=None):
        """The joint sieve of h and 2h + 1 over rows of h: uint8 ``[S]``, 1 iff some listed prime l has h = 0 (l divides
        h) or h = (l - 1) / 2 (l divides 2h + 1) modulo l — ``sieve_t(h) | sieve_t(2h + 1)`` from one pass over limbs and
        tables (mx_safe_sieve, csrc/mx_sieve.hpp).  ValueError — nothing launched — for an empty list, a listed prime
        that is even, below 3 or not below 2^31, or rows of another shape."""
        rows, limbs = self._word_rows(halves_t, "halves")
        primes = [int(p) for p in primes]
        if not primes or any(p < 3 or p % 2 == 0 or p >= 1 << 31 for p in primes):
            raise ValueError("a list of odd primes in [3, 2^31) expected")
        out_t = self._flags_out(out_t, rows)
        if rows:
            h_primes = np.ascontiguousarray(np.asarray(primes, dtype=np.uint32))
            self._call("mx_safe_sieve", halves_t.data_ptr(), out_t.data_ptr(), h_primes.ctypes.data, len(h_primes), limbs, rows,
                       workspace=("mx_safe_sieve_workspace_bytes", limbs, len(h_primes)))
        return out_t

    def safe_double_t(self, halves_t, _checked: bool = False):
        """2h + 1 for rows of h, as rows of the same width (mx_safe_double: one launch).  ValueError — nothing launched —
        when a row has its top bit (bit 32 * limbs - 1) set, so that 2h + 1 would not fit the width, or for rows of
        another shape."""
        rows, limbs = self._word_rows(halves_t, "halves")
        if rows and not _checked and bool((halves_t[:, limbs - 1] < 0).any()):      # the top bit is the int32's sign
            raise ValueError("2h + 1 does not fit the rows' width")
        out_t = self._empty_rows(limbs, rows)
        if rows:
            self._call("mx_safe_double", halves_t.data_ptr(), out_t.data_ptr(), limbs, rows)
        return out_t

    # ------------------------------------------------------------------ decryption proofs of a dealt threshold key (threshold.py)
    def sha256_rows_t(self, prefix: bytes, row_sets: Sequence[Any], count: Optional[int] = None):
        """digest[r] = SHA-256(prefix | BE(rows_0[r]) | .. | BE(rows_{k-1}[r])) on the device (mx_sha256_rows,
        csrc/mx_sha256.hpp): ``prefix`` 32 bytes, ``row_sets`` up to eight int32 device tensors ``[count, limbs_s]`` of
        any widths, BE(row) the row as a big-endian integer of 4 * limbs_s bytes.  Returns ``[count, 8]`` int32 rows
        whose integer is ``int.from_bytes(digest, "big")``.  ``count`` is needed only when there is no set (the prefix
        alone, hashed `count` times).  ValueError — nothing launched — for anything else."""
        prefix = bytes(prefix)
        if len(prefix) != 32:
            raise ValueError("the prefix must have 32 bytes")
        sets = list(row_sets)
        if len(sets) > _lib.MX_SHA256_MAX_SETS:
            raise ValueError(f"at most {_lib.MX_SHA256_MAX_SETS} row sets")
        shapes = [self._word_rows(t, "hashed rows") for t in sets]
        if not sets and count is None:
            raise ValueError("count expected when there is no row set")
        rows = int(count) if count is not None else shapes[0][0]
        if rows < 0 or any(s[0] != rows for s in shapes):
            raise ValueError("every row set must have the same number of rows")
        out_t = self.torch.empty((rows, 8), dtype=self.torch.int32, device=self.device)
        if rows:
            ptrs = (_ctypes.c_void_p * max(1, len(sets)))(*[t.data_ptr() for t in sets])
            widths = (_ctypes.c_int * max(1, len(sets)))(*[s[1] for s in shapes])
            self._call("mx_sha256_rows", prefix, ptrs, widths, len(sets), rows, out_t.data_ptr())
        return out_t

    def dleq_response_t(self, rho_t, e_t, x_t, out_t=None):
        """(z, status): z[r] = rho[r] + e[r] * x over the integers on the device (mx_dleq_response, csrc/mx_response.hpp).
        ``rho_t`` ``[count, wz]``, ``e_t`` ``[count, ew]``, ``x_t`` ONE row ``[wx]`` or ``[1, wx]`` — the secret exponent,
        which stays on the device —, z ``[count, wz]`` (``out_t``; it may be ``rho_t``), status uint8 ``[count]``: 1 where
        the sum does not fit wz words (z then holds its low words).  The caller sizes wz so that it never happens and
        reads the status when it cannot be sure."""
        if not _is_device_rows(x_t) or x_t.dim() not in (1, 2) or (x_t.dim() == 2 and x_t.shape[0] != 1):
            raise ValueError("ONE exponent row on the device expected")
        return self._response("mx_dleq_response", rho_t, e_t, x_t.view(1, -1), out_t, shared=True)

    def _response(self, symbol: str, rho_t, e_t, x_t, out_t, shared: bool):
        """dleq_response_t (`shared`: ONE secret row ``[1, wx]``) and response_rows_t (one per rho row) behind their checks."""
        count, wz = self._word_rows(rho_t, "rho rows")
        _, ew = self._word_rows(e_t, "challenge rows")
        _, wx = self._word_rows(x_t, "the exponent row" if shared else "secret rows")
        if e_t.shape[0] != count or (not shared and x_t.shape[0] != count):
            raise ValueError(f"one challenge row{'' if shared else ' and one secret row'} per rho row expected")
        if out_t is None:
            out_t = self.torch.empty_like(rho_t)
        elif self._word_rows(out_t, "z rows", wz)[0] != count:
            raise ValueError("one z row per rho row expected")
        status_t = self.torch.empty(count, dtype=self.torch.uint8, device=self.device)
        if count:
            self._call(symbol, rho_t.data_ptr(), e_t.data_ptr(), x_t.data_ptr(), out_t.data_ptr(), status_t.data_ptr(), wz, ew, wx, count)
        return out_t, status_t

    def _multiexp_operands(self, inputs_t, index_t, weights_t, terms: int, weight_bits: int, window: int, checked: bool) -> Tuple[int, int, int]:
        """(n_inputs, limbs, rows) of the device operands of a multi-exponentiation whose `terms` and `weight_bits` the
        caller has bounded; ValueError for anything else, the index read for its range last and only when not `checked`."""
        n_inputs, limbs = self._word_rows(inputs_t, "inputs")
        if not 0 <= window <= 8:
            raise ValueError("window must lie in 1 .. 8 (0 = automatic)")
        rows, _ = self._word_rows(index_t, "the index", terms)
        ww = (weight_bits + 31) // 32
        if (not _is_device_rows(weights_t) or weights_t.dtype != self.torch.int32 or not weights_t.is_contiguous()
                or weights_t.device != self.device or weights_t.dim() < 2 or weights_t.shape[0] != rows or weights_t.numel() != rows * terms * ww):
            raise ValueError(f"contiguous int32 device weights of {terms} x {ww} words per row expected")
        if n_inputs < 1:
            raise ValueError("at least one input expected")
        if rows and not checked and bool(((index_t < 0) | (index_t >= n_inputs)).any()):
            raise ValueError("index out of range")
        return n_inputs, limbs, rows

    @_int_args
    def multiexp_nsquare_rows_t(self, inputs_t, index_t, weights_t, terms: int, weight_bits: int, n: int, window: int = 0,
                                _checked: bool = False):
        """out[r] = prod_{t < terms} inputs[index[r][t]] ^ w[r][t] mod n^2 with the index and the weights ALREADY ON THE
        DEVICE: ``index_t`` int32 ``[rows, terms]`` in [0, n_inputs), ``weights_t`` int32 ``[rows, terms * ww]`` (or any
        contiguous view of it, such as ``[rows, terms, ww]``) of non-negative weights of ww = ceil(weight_bits / 32)
        little-endian words, weight_bits <= 2 bits(n) + 64.  One launch of mx_multiexp_nsquare_run behind its table
        pass: no plan, no sign split, no split-K — the thin entry for weights that are secret or were made on the device
        (``multiexp_nsquare_t`` plans public ones).  Canonical residues ``[rows, limbs2]``."""
        _check_modulus(n)
        nb = n.bit_length()
        if terms < 1 or weight_bits < 1 or weight_bits > 2 * nb + 64:
            raise ValueError(f"terms >= 1 and weight_bits in 1 .. 2 bits(n) + 64 = {2 * nb + 64} expected")
        n_inputs, limbs2, rows = self._multiexp_operands(inputs_t, index_t, weights_t, terms, weight_bits, window, _checked)
        _check_rows_n2(n, limbs2)
        out_t = self._empty_rows(limbs2, rows)
        if rows == 0:
            return out_t
        if window == 0:
            window = self.multiexp_nsquare_shape(n, n_inputs, rows, terms, weight_bits)[0]
        plan = self.nsquare_plan(n, 1)          # the constants of mx_powmod_nsquare_prepare (its exponent is not read)
        self._call("mx_multiexp_nsquare_run", plan.desc, inputs_t.data_ptr(), n_inputs, limbs2, index_t.data_ptr(), weights_t.data_ptr(),
                   terms, weight_bits, out_t.data_ptr(), rows, 0, window,
                   workspace=("mx_multiexp_nsquare_workspace_bytes", nb, n_inputs, 0, window), plans=(plan,))
        return out_t

    # ------------------------------------------------------------------ range proofs of ciphertexts (range_proof.py)
    def multiexp_mod_shape(self, mod: int, n_inputs: int, n_outputs: int, terms: int, weight_bits: int, window: int = 0) -> Tuple[int, int, int]:
        """(lanes per element, limbs per lane, window) of mx_multiexp_shape for the modulus `mod`."""
        return self._query("mx_multiexp_shape", int(mod).bit_length(), n_inputs, n_outputs, terms, weight_bits, int(window), outs=_INTS[:3])

    @_int_args
    def multiexp_mod_t(self, inputs_t, index_t, weights_t, terms: int, weight_bits: int, mod: int, window: int = 0,
                       term_bits: Optional[Sequence[int]] = None, _checked: bool = False):
        """out[r] = prod_{j < terms} inputs[index[r][j]] ^ w[r][j] mod `mod` for ANY odd modulus >= 3 (mx_multiexp_run,
        csrc/mx_multiexp.hpp: the Straus form on the generic Montgomery arithmetic, a table pass and a main pass).
        ``inputs_t`` ``[n_inputs, limbs]`` residues below `mod`, ``index_t`` int32 ``[rows, terms]`` in [0, n_inputs),
        ``weights_t`` int32 ``[rows, terms * ww]`` (or any contiguous view of it) of non-negative weights of
        ww = ceil(weight_bits / 32) little-endian words whose bits at and above ``weight_bits`` are 0; ``weight_bits``
        in 1 .. 16384 whatever bits(mod) is.  ``term_bits``: one length per term, 0 .. weight_bits — the caller's promise
        that the weights of term j are below 2^term_bits[j] in EVERY row; the windows above it skip that term (put the
        longest term first: its table entry is fetched ahead of the squarings).  0^0 = 1.  Shared bases (every row the
        same index) and per-row bases go through the same kernel.  Canonical residues ``[rows, limbs]``."""
        _check_modulus(mod)
        if terms < 1 or not 1 <= weight_bits <= _lib.MX_MULTIEXP_MAX_WEIGHT_BITS:
            raise ValueError(f"terms >= 1 and weight_bits in 1 .. {_lib.MX_MULTIEXP_MAX_WEIGHT_BITS} expected")
        c_term_bits = None
        if term_bits is not None:
            if len(term_bits) != terms or any(not 0 <= int(b) <= weight_bits for b in term_bits):
                raise ValueError("one length in 0 .. weight_bits per term expected")
            c_term_bits = (_ctypes.c_int32 * terms)(*[int(b) for b in term_bits])
        n_inputs, limbs, rows = self._multiexp_operands(inputs_t, index_t, weights_t, terms, weight_bits, window, _checked)
        if _limbs.limbs_for(mod) > limbs:
            raise ValueError("rows narrower than the modulus")
        out_t = self._empty_rows(limbs, rows)
        if rows == 0:
            return out_t
        bits = mod.bit_length()
        if window == 0:
            window = self.multiexp_mod_shape(mod, n_inputs, rows, terms, weight_bits)[2]
        h_mod = _limbs.pack_one(mod, limbs)
        self._call("mx_multiexp_run", h_mod.ctypes.data, limbs, inputs_t.data_ptr(), n_inputs, index_t.data_ptr(), weights_t.data_ptr(),
                   terms, weight_bits, c_term_bits, out_t.data_ptr(), rows, window,
                   workspace=("mx_multiexp_workspace_bytes", bits, limbs, n_inputs, terms, window))
        return out_t

    @_int_args
    def multiexp_mod_batch(self, bases: Sequence[Sequence[int]], weights: Sequence[Sequence[int]], mod: int, window: int = 0) -> List[int]:
        """[prod_j bases[r][j] ^ weights[r][j] mod `mod` for r]: every row its own bases (taken modulo `mod`) and
        non-negative weights, the same number of terms in every row — the int-level entry of ``multiexp_mod_t``."""
        _check_modulus(mod)
        if len(bases) != len(weights):
            raise ValueError("one row of weights per row of bases expected")
        if not bases:
            return []
        terms = len(bases[0])
        if terms < 1 or any(len(b) != terms for b in bases) or any(len(w) != terms for w in weights):
            raise ValueError("the same number of terms (at least one) in every row expected")
        flat_w = [int(w) for row in weights for w in row]
        if any(w < 0 for w in flat_w):
            raise ValueError("non-negative weights expected")
        weight_bits = max(1, max(w.bit_length() for w in flat_w))
        ww = (weight_bits + 31) // 32
        limbs = _limbs.limbs_for(mod)
        rows = len(bases)
        inputs_t = self._upload_ints([b for row in bases for b in row], limbs, mod)
        index_t = self.torch.arange(rows * terms, device=self.device, dtype=self.torch.int32).view(rows, terms).contiguous()
        weights_t = self.to_device(_limbs.pack(flat_w, ww).reshape(rows, terms * ww))
        return self._download_ints(self.multiexp_mod_t(inputs_t, index_t, weights_t, terms, weight_bits, mod, window, _checked=True))

    def response_rows_t(self, rho_t, e_t, x_t, out_t=None):
        """(z, status): z[r] = rho[r] + e[r] * x[r] over the integers on the device (mx_response_rows,
        csrc/mx_response.hpp) — ``dleq_response_t`` with a secret row PER PROOF: ``rho_t`` ``[count, wz]``, ``e_t``
        ``[count, ew]``, ``x_t`` ``[count, wx]``, z ``[count, wz]`` (``out_t``), status uint8 ``[count]``: 1 where the sum
        does not fit wz words (z then holds its low words)."""
        return self._response("mx_response_rows", rho_t, e_t, x_t, out_t, shared=False)

    # ------------------------------------------------------------------ one-of-k membership proofs (membership.py)
    def member_challenges_t(self, e_t, sim_t, index_t, mode: int, out_t=None):
        """The challenge arithmetic of the one-of-k proofs on the device (mx_member_challenges, csrc/mx_member.hpp):
        ``sim_t`` ``[count, 4 k]`` rows of k challenges of four words, 2 <= k <= 16, ``e_t`` ``[count, 4]``, ``index_t``
        int32 ``[count]`` in [0, k) — the REAL slot of each row, the prover's secret.  mode 0 (mask): slot index[r] zeroed
        (``e_t`` may be None); mode 1 (split): slot index[r] = e[r] - the sum of the others mod 2^128; both return
        ``[count, 4 k]`` rows (``out_t``; it may be ``sim_t``).  mode 2 (sum): uint8 ``[count]``, 1 where the sum of the
        row mod 2^128 differs from e[r] (``index_t`` may be None: none is read).  Control flow and addresses of the
        kernel do not depend on the index; it is read here once, for its range."""
        torch = self.torch
        mode = int(mode)
        if mode not in (_lib.MX_MEMBER_MASK, _lib.MX_MEMBER_SPLIT, _lib.MX_MEMBER_SUM):
            raise ValueError("mode 0 (mask), 1 (split) or 2 (sum) expected")
        count, words = self._word_rows(sim_t, "challenge slots")
        k = words // 4
        if words % 4 or not _lib.MX_MEMBER_MIN_K <= k <= _lib.MX_MEMBER_MAX_K:
            raise ValueError(f"rows of {_lib.MX_MEMBER_MIN_K} .. {_lib.MX_MEMBER_MAX_K} slots of four words expected")
        if mode != _lib.MX_MEMBER_MASK and self._word_rows(e_t, "challenge rows", 4)[0] != count:
            raise ValueError("one challenge row per row of slots expected")
        if mode == _lib.MX_MEMBER_SUM:
            status_t = torch.empty(count, dtype=torch.uint8, device=self.device)
            if count:
                self._call("mx_member_challenges", e_t.data_ptr(), sim_t.data_ptr(), None, None, status_t.data_ptr(), k, count, mode)
            return status_t
        if (not _is_device_rows(index_t) or index_t.dtype != torch.int32 or index_t.dim() != 1 or not index_t.is_contiguous()
                or index_t.device != self.device or index_t.shape[0] != count):
            raise ValueError("a contiguous int32 device index [count] expected")
        if count and bool(((index_t < 0) | (index_t >= k)).any()):
            raise ValueError("index out of range")
        if out_t is None:
            out_t = torch.empty_like(sim_t)
        elif self._word_rows(out_t, "output slots", words)[0] != count:
            raise ValueError("one output row per row of slots expected")
        if count:
            self._call("mx_member_challenges", None if e_t is None else e_t.data_ptr(), sim_t.data_ptr(), index_t.data_ptr(), out_t.data_ptr(),
                       None, k, count, mode)
        return out_t

    # ------------------------------------------------------------------ multiplication proofs (multiplication.py)
    @staticmethod
    def response_mod_constants(mod: int, wn: int) -> Tuple[int, int]:
        """(recip, shift) of mx_response_mod_rows for a modulus of ``wn`` words whose top word is non-zero: shift = the
        leading zeros of the top word, recip = floor(2^96 / (Md + 1)) for Md = the top 64 bits of mod << shift
        (tools/mul_model.py: response_mod_constants)."""
        mod, wn = int(mod), int(wn)
        top = mod >> (32 * (wn - 1)) if wn >= 1 else 0
        if not 0 < top < 1 << 32:
            raise ValueError("a modulus of wn words whose top word is non-zero expected")
        shift = 32 - top.bit_length()
        md = (mod << shift) >> (32 * (wn - 2)) if wn >= 2 else (mod << shift) << 32
        return (1 << 96) // (md + 1), shift

    @_int_args
    def response_mod_rows_t(self, rho_t, e_t, x_t, mod: int, out_t=None):
        """(w, t, status): w[r] = (rho[r] + e[r] x[r]) mod ``mod`` and t[r] = (rho[r] + e[r] x[r]) // ``mod`` on the
        device (mx_response_mod_rows, csrc/mx_response_mod.hpp) — the response of a Sigma-protocol whose exponent lives
        modulo N, with the quotient that corrects the second response.  ``rho_t`` and ``x_t`` ``[count, wn]`` (x: a
        secret row per proof), ``e_t`` ``[count, ew]``, ``mod`` of exactly wn words (``limbs.limbs_for(mod) == wn``), odd
        or even; w ``[count, wn]`` (``out_t``), canonical; t ``[count, ew]``; status uint8 ``[count]``: 1 where the
        quotient does not fit ew words — only when rho or x is not below ``mod`` —, t then holds its low words and w is
        still the residue.  Control flow and addresses of the kernel depend on the shapes only.  The outputs are the
        kernel's temporaries: ``out_t`` sharing storage with an input is a ValueError."""
        count, wn = self._word_rows(rho_t, "rho rows")
        _, ew = self._word_rows(e_t, "challenge rows")
        if self._word_rows(x_t, "secret rows", wn)[0] != count or e_t.shape[0] != count:
            raise ValueError("one challenge row and one secret row per rho row expected")
        if mod < 1 or _limbs.limbs_for(mod) != wn:
            raise ValueError("a modulus of exactly the width of the rows expected")
        recip, shift = self.response_mod_constants(mod, wn)
        if out_t is None:
            out_t = self.torch.empty_like(rho_t)
        else:
            if self._word_rows(out_t, "w rows", wn)[0] != count:
                raise ValueError("one w row per rho row expected")
            mine = out_t.untyped_storage().data_ptr()
            if any(mine == t.untyped_storage().data_ptr() for t in (rho_t, e_t, x_t)):
                raise ValueError("the output must not alias an input: its rows are the kernel's temporaries")
        t_t = self.torch.empty((count, ew), dtype=self.torch.int32, device=self.device)
        status_t = self.torch.empty(count, dtype=self.torch.uint8, device=self.device)
        if count:
            mod_t = self._const_rows([mod], wn)
            self._call("mx_response_mod_rows", rho_t.data_ptr(), e_t.data_ptr(), x_t.data_ptr(), mod_t.data_ptr(), recip, shift,
                       out_t.data_ptr(), t_t.data_ptr(), status_t.data_ptr(), wn, ew, count)
        return out_t, t_t, status_t

    # ------------------------------------------------------------------ share recombination
    @_int_args
    def combine_t(self, partials_t, n: int, theta_inv: int, out_t=None, status_t=None, packed: bool = False):
        """partials_t int32 [n_partials, batch, limbs2] (players 1..degree+1 in order) ->
        (plaintext rows int32 [batch, limbs(N)], status uint8 [batch], 1 = not divisible by N).
        With ``packed=True`` the result is ONE tensor [batch, limbs(N)+1] whose last word is the
        status — plaintext and status as one row (one all-gather when ciphertexts are sharded)."""
        n_partials, batch, limbs2 = partials_t.shape
        plan = self.combine_plan(n, theta_inv, limbs2)
        limbs = plan.desc.limbs
        stride = limbs + 1 if packed else limbs
        if out_t is None:
            out_t = self.torch.empty((batch, stride), dtype=self.torch.int32, device=self.device)
        if tuple(out_t.shape) != (batch, stride):
            raise ValueError("output rows of the wrong shape")
        if status_t is None and not packed:
            status_t = self.torch.empty(batch, dtype=self.torch.uint8, device=self.device)
        self._small(lambda: self._call("mx_combine_run", plan.desc, partials_t.data_ptr(), out_t.data_ptr(), stride,
                                       status_t.data_ptr() if status_t is not None else None, n_partials, batch, plans=(plan,)))
        return out_t if packed else (out_t, status_t)

    @_int_args
    def combine_batch(
        self, partials: Sequence[Sequence[int]], n: int, theta_inv: int
    ) -> Tuple[List[int], List[bool]]:
        """partials[e] = the degree+1 partial decryptions of ciphertext e (player 1 first).
        Returns (messages, ok); ok[e] False where the reference raises ValueError (PSK:119-123)."""
        if len(partials) == 0:
            return [], []
        n_partials = len(partials[0])
        if any(len(p) != n_partials for p in partials):
            raise ValueError("every ciphertext needs the same number of partial decryptions")
        n2 = n * n
        limbs2 = _limbs.limbs_for(n2)
        rows = np.stack([_limbs.pack_reduced([p[i] for p in partials], limbs2, n2) for i in range(n_partials)])
        out_t, status_t = self.combine_t(self.to_device(rows), n, theta_inv)
        ok = [not bool(x) for x in status_t.cpu().numpy()]
        return self._download_ints(out_t), ok

    @_int_args
    def combine_columns(self, columns: Sequence[Any], n: int, theta_inv: int) -> Tuple[List[int], List[bool]]:
        """Share recombination from one COLUMN per player (players 1..degree+1 in order): a column is the
        device rows kept by ``powmod_nsquare_batch(..., keep_rows=True)`` or a received list of partial
        decryptions (plain ints or wire-form ``{"type": "int", "data": bytes}`` entries, DK:496-505) —
        received values reach the device through codec.rows_from_wire, i.e. without a per-element
        Python conversion and without the per-ciphertext dictionaries of DK:477-505.
        Returns (messages, ok) like ``combine_batch``."""
        from . import codec

        if len(columns) == 0:
            return [], []
        n2, limbs2 = _nsquare(n)
        torch = self.torch
        cols = []
        for col in columns:
            if hasattr(col, "data_ptr"):
                if col.shape[1] != limbs2:
                    raise ValueError("device column of the wrong row width")
                cols.append(col)
            else:
                cols.append(self.to_device(codec.rows_from_wire(col, limbs2, modulus=n2)))
        batch = cols[0].shape[0]
        if any(c.shape[0] != batch for c in cols):
            raise ValueError("every player's column needs one partial decryption per ciphertext")
        if batch == 0:
            return [], []
        out_t, status_t = self.combine_t(torch.stack(cols, dim=0), n, theta_inv)
        msgs = self._fetched_ints("messages", out_t)
        ok = [not bool(x) for x in status_t.cpu().numpy()]
        return msgs, ok

    # ------------------------------------------------------------------ private-key (CRT) decryption
    @_int_args
    def crt_plan(self, p: int, q: int, limbs2: int = 0) -> _Plan:
        """The plan of the decryption with the primes p, q of N (mx_crt_prepare), cached like combine_plan: Montgomery
        constants of p^2, q^2, p and q for ciphertext rows of `limbs2` words (0 = the words of N^2).  h_p, h_q and
        p^-1 mod q are computed here, on the host (private_key.crt_constants: ValueError for a pair that is no key)."""
        from .private_key import crt_constants

        need = _limbs.limbs_for((p * q) ** 2)
        limbs2 = int(limbs2) or need
        key = (p, q, limbs2)
        plan = self._cached(self._crt_plans, key)
        if plan is not None:
            return plan
        h_p, h_q, p_inv = crt_constants(p, q)
        if limbs2 < need:
            raise ValueError("rows narrower than N^2")
        limbs = _limbs.limbs_for(max(p, q))
        rows = [_limbs.pack_one(v, limbs) for v in (p, q, h_p, h_q, p_inv)]
        desc = _lib.CrtPlan()
        nbytes = _lib.check(self.lib.mx_crt_plan_bytes(limbs, limbs2), "mx_crt_plan_bytes")
        return self._prepare(self._crt_plans, key, nbytes, "mx_crt_prepare",
                             (desc, *(r.ctypes.data for r in rows), limbs, limbs2), lambda *made: _Plan(desc, *made))

    @_int_args
    def crt_split_t(self, cts_t, p: int, q: int):
        """cts_t int32 [batch, limbs2] (any value of that width) -> int32 [2, batch, limbs_half]: the rows modulo p^2, then
        modulo q^2; ``out[0]`` and ``out[1]`` are the contiguous operands of ``powmod_nsquare_t(.., p, p - 1)`` and
        ``(.., q, q - 1)``."""
        _, limbs2 = cts_t.shape
        return self._crt_split(self.crt_plan(p, q, limbs2), "mx_crt_split_run", cts_t)

    def _crt_split(self, plan: _Plan, symbol: str, rows_t):
        """crt_split_t and crt_prime_split_t: the rows modulo the two moduli of `plan`, int32 [2, batch, limbs_half]."""
        batch = rows_t.shape[0]
        out_t = self.torch.empty((2, batch, plan.desc.limbs_half), dtype=self.torch.int32, device=self.device)
        if batch:
            rows_t = rows_t.contiguous()
            self._small(lambda: self._call(symbol, plan.desc, rows_t.data_ptr(), out_t.data_ptr(), batch, plans=(plan,)))
        return out_t

    @_int_args
    def crt_recombine_t(self, xp_t, xq_t, p: int, q: int, packed: bool = False, limbs2: int = 0):
        """xp_t, xq_t int32 [batch, limbs_half] (x_p = c^(p-1) mod p^2, x_q = c^(q-1) mod q^2) -> (plaintext rows int32
        [batch, limbs(N)], status uint8 [batch]): bit 0 = x_p is not 1 modulo p, bit 1 = x_q is not 1 modulo q, the row is
        zero then.  With ``packed=True`` ONE tensor [batch, limbs(N) + 1] whose last word is the status — the formats of
        combine_t.  `limbs2`: the row width the plan was made for (0 = the words of N^2)."""
        plan = self.crt_plan(p, q, limbs2)
        batch, half = xp_t.shape
        if half != plan.desc.limbs_half or tuple(xq_t.shape) != (batch, half):
            raise ValueError("x rows of the wrong shape")
        limbs = plan.desc.limbs_n
        stride = limbs + 1 if packed else limbs
        out_t = self.torch.empty((batch, stride), dtype=self.torch.int32, device=self.device)
        status_t = None if packed else self.torch.empty(batch, dtype=self.torch.uint8, device=self.device)
        if batch:
            xp_t, xq_t = xp_t.contiguous(), xq_t.contiguous()
            self._small(lambda: self._call("mx_crt_recombine_run", plan.desc, xp_t.data_ptr(), xq_t.data_ptr(), out_t.data_ptr(),
                                           stride, status_t.data_ptr() if status_t is not None else None, batch, plans=(plan,)))
        return out_t if packed else (out_t, status_t)

    def _crt_pair(self, run_p, run_q, side_by_side: bool):
        """(run_p(), run_q()) — the chains modulo p^2 and q^2 of a private-key operation: one after the other on the
        caller's stream, or run_q on the caller's companion stream (one per stream, kept) beside run_p, joined again
        before this returns.  Plans are prepared by the caller, on its stream, before the fan-out."""
        if not side_by_side:
            return run_p(), run_q()
        torch = self.torch
        cur = torch.cuda.current_stream(self.device)
        side = self._crt_streams.get(int(cur.cuda_stream))
        if side is None:
            with torch.cuda.device(self.device):
                side = self._crt_streams[int(cur.cuda_stream)] = torch.cuda.Stream(device=self.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            xq_t = run_q()
        xp_t = run_p()
        cur.wait_stream(side)
        xq_t.record_stream(cur)                    # allocated on the companion, read by the caller's stream from here on
        return xp_t, xq_t

    # ------------------------------------------------------------------ private-key (CRT) encryption
    @_int_args
    def crt_enc_plan(self, p: int, q: int, limbs_r: int = 0) -> _Plan:
        """The plan of the encryption with the primes p, q of N (mx_crt_enc_prepare), cached next to crt_plan: Montgomery
        constants of p and q for randomness rows of `limbs_r` words (0 = the words of N) and of p^2 and q^2 for the lift.
        (p^2)^-1 mod q^2 is computed here, on the host; ValueError for a pair that is no key (private_key.crt_constants)."""
        from .private_key import crt_constants

        limbs_r = int(limbs_r) or _limbs.limbs_for(p * q)
        key = (p, q, limbs_r)
        plan = self._cached(self._crt_enc_plans, key)
        if plan is not None:
            return plan
        crt_constants(p, q)
        if limbs_r < 1:
            raise ValueError("randomness rows need a word")
        limbs = _limbs.limbs_for(max(p, q))
        rows = [_limbs.pack_one(p, limbs), _limbs.pack_one(q, limbs), _limbs.pack_one(pow(p * p, -1, q * q), 2 * limbs)]
        desc = _lib.CrtEncPlan()
        nbytes = _lib.check(self.lib.mx_crt_enc_plan_bytes(limbs, limbs_r), "mx_crt_enc_plan_bytes")
        return self._prepare(self._crt_enc_plans, key, nbytes, "mx_crt_enc_prepare",
                             (desc, *(r.ctypes.data for r in rows), limbs, limbs_r), lambda *made: _Plan(desc, *made))

    @_int_args
    def crt_prime_split_t(self, rows_t, p: int, q: int):
        """rows_t int32 [batch, limbs_r] (any value of that width) -> int32 [2, batch, limbs_half]: the rows modulo p, then
        modulo q, zero above the prime; ``out[0]`` and ``out[1]`` are the contiguous operands of
        ``powmod_shared_t(.., p, q mod (p-1))`` and ``(.., q, p mod (q-1))``, whose results ``powmod_nsquare_t(.., p, p)``
        and ``(.., q, q)`` take as they are."""
        _, limbs_r = rows_t.shape
        return self._crt_split(self.crt_enc_plan(p, q, limbs_r), "mx_crt_prime_split_run", rows_t)

    @_int_args
    def crt_lift_t(self, rho_p_t, rho_q_t, p: int, q: int, messages_t=None, halves_t=None, packed: bool = False):
        """The noise halves rho_p_t, rho_q_t int32 [batch, limbs_half] (below p^2 and q^2) -> (rows int32 [batch,
        limbs(N^2)], status uint8 [batch]) of c = v rho mod N^2, canonical, with rho = CRT(rho_p, rho_q) and
        v = 1 + m N for ``messages_t`` [batch, >= limbs(N)] (m below N), v = the ciphertexts whose halves ``halves_t``
        [2, batch, limbs_half] holds (crt_split_t), or v = 1 for neither.  Status bit 0 = rho_p is 0, bit 1 = rho_q is 0
        — p or q divides the randomness — and the row is zero then.  With ``packed=True`` ONE tensor [batch,
        limbs(N^2) + 1] whose last word is the status."""
        plan = self.crt_enc_plan(p, q)
        batch, half = rho_p_t.shape
        if half != plan.desc.limbs_half or tuple(rho_q_t.shape) != (batch, half):
            raise ValueError("noise rows of the wrong shape")
        if messages_t is not None and halves_t is not None:
            raise ValueError("a message or a ciphertext, not both")
        if messages_t is not None and (messages_t.dim() != 2 or messages_t.shape[0] != batch or messages_t.shape[1] < plan.desc.limbs_n):
            raise ValueError("one message row per noise row expected, no narrower than N")
        if halves_t is not None and tuple(halves_t.shape) != (2, batch, half):
            raise ValueError("ciphertext halves of the wrong shape")
        limbs2 = plan.desc.limbs2
        stride = limbs2 + 1 if packed else limbs2
        out_t = self.torch.empty((batch, stride), dtype=self.torch.int32, device=self.device)
        status_t = None if packed else self.torch.empty(batch, dtype=self.torch.uint8, device=self.device)
        if batch:
            rho_p_t, rho_q_t = rho_p_t.contiguous(), rho_q_t.contiguous()
            m_t = None if messages_t is None else messages_t.contiguous()
            h_t = None if halves_t is None else halves_t.contiguous()
            self._small(lambda: self._call(
                "mx_crt_lift_run", plan.desc, rho_p_t.data_ptr(), rho_q_t.data_ptr(), m_t.data_ptr() if m_t is not None else None,
                m_t.shape[1] if m_t is not None else 0, h_t.data_ptr() if h_t is not None else None, out_t.data_ptr(), stride,
                status_t.data_ptr() if status_t is not None else None, batch, plans=(plan,)))
        return out_t if packed else (out_t, status_t)

    # ------------------------------------------------------------------ biprimality verdict
    def biprime_verdict_t(self, v_t, mods, pass_t=None):
        """v_t int32 [n_parties, groups, n_slots, limbs] (party 1 first) -> uint8 [groups, n_slots].
        `mods`: sequence of ints or a device-resident (rows, max bits) pair."""
        n_parties, groups, n_slots, limbs = v_t.shape
        mods_t, mod_bits = self._mods_operand(mods, limbs)
        if mods_t.shape[0] != groups:
            raise ValueError("one modulus per group expected")
        if pass_t is None:
            pass_t = self.torch.empty((groups, n_slots), dtype=self.torch.uint8, device=self.device)
        self._small(lambda: self._call("mx_biprime_verdict_dev", v_t.data_ptr(), pass_t.data_ptr(), mods_t.data_ptr(), limbs, mod_bits,
                                       n_parties, groups, n_slots,
                                       workspace=("mx_verdict_workspace_bytes", limbs, n_parties, groups, n_slots)))
        return pass_t

    @_int_args
    def biprime_verdict_columns(self, columns: Sequence[Any], mods: Sequence[int], n_slots: int, mods_rows: Any = None,
                                as_array: bool = False):
        """The slot tests DK:1147-1158 of many candidates from ONE COLUMN PER PARTY (party 1 first): a column is a flat
        list of groups * n_slots values (candidate-major; short candidates padded by the caller) — packed with one
        codec call — or the handle ``biprime_v_batch(..., keep_rows=True)`` returned for this party's own values,
        which are then taken from the device as they are.  `mods_rows` as in ``biprime_v_batch``.
        Returns per candidate the per-slot verdicts, like ``biprime_verdict_batch`` (``as_array``: as one numpy array)."""
        groups = len(mods)
        if groups == 0:
            return []
        if n_slots == 0:
            return [[] for _ in mods]
        for m in mods:
            _check_modulus(m)
        limbs = _limbs.limbs_for_bits(_limbs.max_bits(mods))
        torch = self.torch
        parts = []
        for col in columns:
            if isinstance(col, _VRows):
                parts.append(col.slots(self, groups, n_slots, limbs))
            elif isinstance(col, NestedColumn):
                if len(col.lists) != groups:
                    raise ValueError("a party's column needs one list per candidate")
                parts.append(self._staged_rows(f"column{len(parts)}", col.lists, limbs, mods, nested=n_slots).view(groups, n_slots, limbs))
            else:
                if len(col) != groups * n_slots:
                    raise ValueError("a party's column needs groups * n_slots values")
                parts.append(self._staged_rows(f"column{len(parts)}", col, limbs, mods).view(groups, n_slots, limbs))
        mods_op = mods_rows.operand(self, groups, limbs) if mods_rows is not None else mods
        pass_t = self.biprime_verdict_t(torch.stack(parts, dim=0), mods_op)
        arr = pass_t.cpu().numpy().astype(bool)
        return arr if as_array else arr.tolist()        # as_array: bool [groups, n_slots] for callers that reduce it with numpy

    @_int_args
    def biprime_verdict_batch(self, v: Sequence[Sequence[Sequence[int]]], mods: Sequence[int]) -> List[List[bool]]:
        """v[g][i][k]: share of party i+1 in test slot k of candidate g (all parties, equal slot counts).
        Returns per candidate the per-slot result of `v_1 == +-prod_{i>=2} v_i (mod N)` (DK:1147-1158)."""
        groups = len(mods)
        if groups == 0:
            return []
        n_parties = len(v[0])
        n_slots = len(v[0][0])
        if n_slots == 0:
            return [[] for _ in mods]
        for m in mods:
            _check_modulus(m)
        limbs = _limbs.limbs_for_bits(_limbs.max_bits(mods))
        rows = np.stack(
            [
                _limbs.pack_reduced([x for g in range(groups) for x in v[g][i][:n_slots]], limbs, list(mods))
                for i in range(n_parties)
            ]
        ).reshape(n_parties, groups, n_slots, limbs)
        pass_t = self.biprime_verdict_t(self.to_device(rows), list(mods))
        arr = pass_t.cpu().numpy().astype(bool)
        return [list(map(bool, arr[g])) for g in range(groups)]


class _N2Backend:
    """What the planners' backends share: device rows [*, limbs2] of one Engine and modulus."""

    def __init__(self, eng: "Engine", n: int, limbs2: int, n_bits: int) -> None:
        self.eng, self.n, self.limbs2, self.n_bits = eng, n, limbs2, n_bits
        self.torch = eng.torch
        self.plan = eng.nsquare_plan(n, 1)          # the constants of mx_powmod_nsquare_prepare (its exponent is not read)

    def _index(self, positions):
        return self.torch.as_tensor(np.asarray(positions, dtype=np.int64), device=self.eng.device)

    def _empty(self, rows: int = 0):
        return self.eng._empty_rows(self.limbs2, rows)

    def bias_rows(self, residues):
        return self.eng._upload_ints([1 + b * self.n for b in residues], self.limbs2, self.n * self.n)

    def _pooled_select(self, views, picks, dim, one_shape):
        """For picks = [(view, entry) or None]: the entries along `dim` of the views laid one behind the other; None picks
        the value one, a block of `one_shape` (1 along `dim`) laid behind them."""
        torch = self.torch
        first = [0]
        for v in views:
            first.append(first[-1] + v.shape[dim])
        if None in picks:
            one = torch.zeros(one_shape, dtype=torch.int32, device=self.eng.device)
            one[..., 0] = 1
            views = views + [one]
        pool = views[0] if len(views) == 1 else torch.cat(views, dim=dim)
        return pool.index_select(dim, self._index([first[-1] if pk is None else first[pk[0]] + pk[1] for pk in picks]))


class _MultiexpBackend(_N2Backend):
    """multiexp_plan.execute over device rows of one Engine and modulus."""

    def take(self, rows_t, positions):
        return rows_t.index_select(0, self._index(positions)).contiguous()

    def invert(self, rows_t):
        return self.eng.modinv_t(rows_t, self.n * self.n)

    def gather(self, inputs_t, inv_t, bias_t, parts):
        pools = [inputs_t] + [t for t in (inv_t, bias_t) if t is not None]
        base = {"x": 0}
        off = inputs_t.shape[0]
        if inv_t is not None:
            base["inv"] = off
            off += inv_t.shape[0]
        if bias_t is not None:
            base["bias"] = off
        pool = self.torch.cat(pools, dim=0) if len(pools) > 1 else inputs_t
        return self.take(pool, [base[kind] + k for kind, k in parts])

    def run(self, tables_t, n_tables, launch, window):
        eng = self.eng
        rows, terms = launch.index.shape
        out_t = self._empty(rows)
        idx_t = eng.to_device(launch.index.view(np.uint32))
        w_t = eng.to_device(launch.weights.reshape(rows, -1))
        eng._call("mx_multiexp_nsquare_run", self.plan.desc, tables_t.data_ptr() if tables_t is not None else None, n_tables, self.limbs2,
                  idx_t.data_ptr(), w_t.data_ptr(), terms, launch.weight_bits, out_t.data_ptr(), rows, 0, window,
                  workspace=("mx_multiexp_nsquare_workspace_bytes", self.n_bits, n_tables, 0, window), plans=(self.plan,))
        return out_t

    def _pick(self, picks):
        if not picks:
            return self._empty()
        views, pos = [], {}
        for pk in picks:
            if pk is not None and id(pk[0]) not in pos:
                pos[id(pk[0])] = len(views)
                views.append(pk[0])
        return self._pooled_select(views, [pk and (pos[id(pk[0])], pk[1]) for pk in picks], 0, (1, self.limbs2))

    rows_of = assemble = _pick          # the two names multiexp_plan.execute calls


class _MatmulBackend(_N2Backend):
    """multiexp_plan.execute_matmul over device rows of one Engine and modulus.  A column block is a tensor
    [columns, samples, limbs2]; the launch arrays go to the device once per call."""

    def __init__(self, eng: "Engine", n: int, limbs2: int, n_bits: int) -> None:
        super().__init__(eng, n, limbs2, n_bits)
        self._arrays: Dict[int, Tuple[Any, Any]] = {}

    def columns(self, inputs_t, n_inputs, batch, cols):
        return inputs_t.view(batch, n_inputs, self.limbs2).index_select(1, self._index(cols)).permute(1, 0, 2).contiguous()

    def invert(self, block_t):
        return self.eng.modinv_t(block_t.view(-1, self.limbs2), self.n * self.n).view_as(block_t)

    def tile(self, block_t, batch, lo, hi):
        return block_t[:, lo:hi, :].reshape(-1, self.limbs2)

    def concat(self, parts):
        return self._empty() if not parts else (parts[0] if len(parts) == 1 else self.torch.cat(parts, dim=0))

    def _launch_arrays(self, launch):
        """index and weights of `launch` on the device, uploaded once per call."""
        if id(launch) not in self._arrays:
            rows = launch.index.shape[0]
            self._arrays[id(launch)] = (self.eng.to_device(launch.index.view(np.uint32)),
                                        self.eng.to_device(launch.weights.reshape(rows, -1)))
        return self._arrays[id(launch)]

    def _table_rows(self, tables_t, n_tables):
        """The table inputs of a launch, contiguous and of the count the launch names (None stays None)."""
        if tables_t is not None:
            tables_t = tables_t.contiguous()
            if tables_t.shape[0] != n_tables:
                raise ValueError("table rows do not match the launch")
        return tables_t

    def run_matmul(self, tables_t, n_cols, n_shared, tile, launch, window):
        eng = self.eng
        rows, terms = launch.index.shape
        idx_t, w_t = self._launch_arrays(launch)
        out_t = self._empty(tile * rows)
        tables_t = self._table_rows(tables_t, n_cols * tile + n_shared)
        eng._call("mx_matmul_nsquare_run", self.plan.desc, tables_t.data_ptr() if tables_t is not None else None, n_cols, n_shared,
                  tile, self.limbs2, idx_t.data_ptr(), w_t.data_ptr(), terms, launch.weight_bits, out_t.data_ptr(), rows, 0, window,
                  workspace=("mx_matmul_nsquare_workspace_bytes", self.n_bits, n_cols, n_shared, tile, 0, window), plans=(self.plan,))
        return out_t

    def select(self, outs, picks, tile, column_major):
        if not picks:
            return self._empty()
        sel = self._pooled_select([o.view(tile, -1, self.limbs2) for o in outs], picks, 1, (tile, 1, self.limbs2))
        if column_major:
            sel = sel.permute(1, 0, 2)
        return sel.reshape(-1, self.limbs2)


class _ConvBackend(_MatmulBackend):
    """conv_plan.execute_conv over device rows of one Engine and modulus: the padded grids are one tensor
    [image, padded row, grid, padded column, limbs2], so the tables of a tile of whole images or of a band of rows are a
    slice of it.  The second pass of split kernels is _MatmulBackend.run_matmul."""

    def __init__(self, eng: "Engine", n: int, limbs2: int, n_bits: int) -> None:
        super().__init__(eng, n, limbs2, n_bits)
        self._origins: Dict[int, Any] = {}

    def grids(self, inputs_t, shape, x_ch, inverted, padding):
        torch = self.torch
        b, c, h, w = shape
        ph, pw = padding
        x = inputs_t.view(b, c, h, w, self.limbs2)
        parts = []
        if x_ch:
            parts.append(x.index_select(1, self._index(x_ch)))
        if inverted:
            parts.append(self.invert(x.index_select(1, self._index(inverted)).contiguous()))
        real = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        out = torch.zeros((b, h + 2 * ph, real.shape[1], w + 2 * pw, self.limbs2), dtype=torch.int32, device=self.eng.device)
        out[..., 0] = 1                                                       # a padded pixel: the ciphertext 1 of 0
        out[:, ph : ph + h, :, pw : pw + w] = real.permute(0, 2, 1, 3, 4)
        return out

    def window(self, grids_t, m0, m1, r0, r1):
        return grids_t[m0:m1, r0:r1].reshape(-1, self.limbs2)

    def run_conv(self, tables_t, n_local, n_shared, launch, window, origin, image_positions):
        eng = self.eng
        rows, terms = launch.index.shape
        idx_t, w_t = self._launch_arrays(launch)
        positions = len(origin)
        key = origin.__array_interface__["data"][0]            # a ragged tile's origins are a prefix of the full tile's
        if key not in self._origins or self._origins[key].numel() < positions:
            self._origins[key] = self.torch.from_numpy(np.ascontiguousarray(origin)).to(eng.device)
        org_t = self._origins[key]
        out_t = self._empty(positions * rows)
        tables_t = self._table_rows(tables_t, n_local + n_shared)
        eng._call("mx_conv_nsquare_run", self.plan.desc, tables_t.data_ptr() if tables_t is not None else None, n_local, n_shared,
                  self.limbs2, idx_t.data_ptr(), w_t.data_ptr(), terms, launch.weight_bits, org_t.data_ptr(), positions,
                  image_positions, out_t.data_ptr(), rows, 0, window,
                  workspace=("mx_conv_nsquare_workspace_bytes", self.n_bits, n_local, n_shared, 0, window), plans=(self.plan,))
        return out_t

    def select_conv(self, outs, outs2, picks, images, image_positions, as_columns):
        if not picks:
            return self._empty()
        if not as_columns and len(outs) == 1 and picks == [(1, 0, r) for r in range(outs[0].shape[0] // (images * image_positions))]:
            return outs[0]                                       # one launch whose rows are the kernels: the result as it stands
        views = [o.view(images, -1, image_positions, self.limbs2) for o in outs]
        views += [o.view(images, image_positions, -1, self.limbs2).permute(0, 2, 1, 3) for o in outs2]
        at = [pk and (pk[1] + (len(outs) if pk[0] == 2 else 0), pk[2]) for pk in picks]
        sel = self._pooled_select(views, at, 1, (images, 1, image_positions, self.limbs2))
        if as_columns:
            sel = sel.permute(1, 0, 2, 3)
        return sel.reshape(-1, self.limbs2)

    def assemble(self, tiles, batch, n_rows, out_h, out_w):
        if not tiles:
            return self._empty()
        if len(tiles) == 1:
            return tiles[0][1]
        out = self._empty(batch * n_rows * out_h * out_w).view(batch, n_rows, out_h, out_w, self.limbs2)
        for (m0, m1, y0, y1), rows_t in tiles:
            out[m0:m1, :, y0:y1] = rows_t.view(m1 - m0, n_rows, y1 - y0, out_w, self.limbs2)
        return out.view(-1, self.limbs2)


class _HistogramBackend(_N2Backend):
    """hist_plan.histogram over device rows of one Engine and modulus.  A row set is a tensor [rows + 1 or more,
    row words]: `rows` pair-form rows, then the one row (and whatever the library's size query rounds up to)."""

    def __init__(self, eng: "Engine", n: int, limbs2: int, n_bits: int) -> None:
        super().__init__(eng, n, limbs2, n_bits)
        self.row_bytes = eng.histogram_nsquare_shape(n, 0, 0, 0)[3]

    def chunk(self, n_rows, n_segments, total_terms, chunk):
        return self.eng.histogram_nsquare_shape(self.n, n_rows, n_segments, total_terms, chunk)[2]

    def _row_set(self, rows):
        need = _lib.check(self.eng.lib.mx_histogram_nsquare_workspace_bytes(self.n_bits, rows, 0), "mx_histogram_nsquare_workspace_bytes")
        return self.torch.empty((-(-need // self.row_bytes), self.row_bytes // 4), dtype=self.torch.int32, device=self.eng.device)

    def convert(self, cts_t, lo, hi):
        rows_t = self._row_set(hi - lo)
        self.eng._call("mx_histogram_nsquare_convert", self.plan.desc, cts_t[lo:hi].data_ptr(), hi - lo, self.limbs2,
                       rows_t.data_ptr(), rows_t.numel() * 4, 0, plans=(self.plan,))
        return rows_t

    def run(self, rows_t, n_rows, index_t, pair_out):
        pieces, chunk = index_t.shape
        out_t = self._row_set(pieces) if pair_out else self._empty(pieces)
        index_t = index_t.contiguous()
        self.eng._call("mx_histogram_nsquare_run", self.plan.desc, rows_t.data_ptr(), n_rows, index_t.data_ptr(), pieces, chunk,
                       out_t.data_ptr(), int(bool(pair_out)), self.limbs2, out_t.numel() * 4, 0, plans=(self.plan,))
        return out_t

    def join(self, row_sets, rows):
        out_t = self._row_set(len(row_sets) * rows)
        for t, part in enumerate(row_sets):
            out_t[t * rows : (t + 1) * rows] = part[:rows]
        out_t[len(row_sets) * rows] = row_sets[0][rows]
        return out_t

    def concat(self, results):
        return results[0] if len(results) == 1 else self.torch.cat(results, dim=0)

    def ones(self, count):
        one = self.torch.zeros((count, self.limbs2), dtype=self.torch.int32, device=self.eng.device)
        one[:, 0] = 1
        return one


class _SpmmBackend(_HistogramBackend):
    """spmm_plan.spmm over device rows: the histogram's row sets, conversion and accumulate run, and the two entries of
    csrc/mx_spmm_n2.hpp."""

    def shape(self, n_tables, n_rows, nnz, weight_bits, window):
        return self.eng.spmm_nsquare_shape(self.n, n_tables, n_rows, nnz, weight_bits, window)[:2]

    def pool(self, cts_t, plus, minus):
        parts = []
        if plus.numel():
            parts.append(cts_t.index_select(0, plus))
        if minus.numel():
            parts.append(self.eng.modinv_t(cts_t.index_select(0, minus), self.n * self.n))      # ValueError without an inverse
        return parts[0] if len(parts) == 1 else self.torch.cat(parts, dim=0)

    def tables(self, pool_t, lo, hi, window):
        rows_t = self._row_set((hi - lo) * ((1 << window) - 1))
        self.eng._call("mx_spmm_nsquare_tables", self.plan.desc, pool_t[lo:hi].data_ptr(), hi - lo, self.limbs2, window,
                       rows_t.data_ptr(), rows_t.numel() * 4, 0, plans=(self.plan,))
        return rows_t

    def bias(self, values):
        return self.bias_rows([int(b) % self.n for b in values])

    def horner(self, rows_t, n_rows, positions, window, bias_rows_t):
        out_t = self._empty(n_rows)
        self.eng._call("mx_spmm_nsquare_horner", self.plan.desc, rows_t.data_ptr(), n_rows, positions, window,
                       bias_rows_t.data_ptr() if bias_rows_t is not None else None, out_t.data_ptr(), self.limbs2,
                       out_t.numel() * 4, 0, plans=(self.plan,))
        return out_t


class _ScanBackend(_HistogramBackend):
    """scan_plan.cumsum over device rows: the histogram's row sets, conversion and accumulate run, and the two entries
    of csrc/mx_scan_n2.hpp."""

    def scan(self, rows_t, n_rows, index_t, carry, exclusive):
        pieces, chunk = index_t.shape
        out_t = self._row_set(n_rows)
        index_t = index_t.contiguous()
        carry_t, n_carry, carry_index_t = carry if carry is not None else (None, 0, None)
        if carry_index_t is not None:
            carry_index_t = carry_index_t.contiguous()
        self.eng._call("mx_scan_nsquare_run", self.plan.desc, rows_t.data_ptr(), n_rows, index_t.data_ptr(), pieces, chunk,
                       carry_t.data_ptr() if carry is not None else None, n_carry,
                       carry_index_t.data_ptr() if carry is not None else None, int(bool(exclusive)), out_t.data_ptr(),
                       self.limbs2, out_t.numel() * 4, 0, plans=(self.plan,))
        return out_t

    def store(self, rows_t, n_rows):
        out_t = self._empty(n_rows)
        self.eng._call("mx_scan_nsquare_store", self.plan.desc, rows_t.data_ptr(), n_rows, out_t.data_ptr(), self.limbs2,
                       out_t.numel() * 4, 0, plans=(self.plan,))
        return out_t

    def pick(self, rows_t, n_rows, row):
        out_t = self._row_set(1)
        out_t[0] = rows_t[row]
        out_t[1] = rows_t[n_rows]
        return out_t


def _grid_shape(x) -> Tuple[Tuple[int, int, int, int], List[Any]]:
    """((B, C, H, W), the entries in row-major order) of a nesting x[b][c][y][x]; ValueError if it is ragged.  A grid of no
    channels has no extent of its own: it is taken as 1 x 1."""
    x = [[[list(r) for r in ch] for ch in img] for img in x]
    b = len(x)
    c = len(x[0]) if b else 0
    h = len(x[0][0]) if c else 1
    w = len(x[0][0][0]) if c and h else 1
    for img in x:
        if len(img) != c or any(len(ch) != h for ch in img) or any(len(r) != w for ch in img for r in ch):
            raise ValueError("the grids must all have the same shape [C][H][W]")
    return (b, c, h, w), [v for img in x for ch in img for r in ch for v in r]


def _table_budget(table_budget: Optional[int]) -> int:
    """The bytes of tables one stage or tile may take: the planners' default unless the caller names one."""
    from . import multiexp_plan as mp

    return mp.TABLE_BUDGET_BYTES if table_budget is None else int(table_budget)


def _check_jacobi_moduli(mods) -> None:
    for m in mods:
        if m < 1 or m % 2 == 0:
            raise ValueError("n should be an odd positive integer")


def _is_device_pair(x) -> bool:
    """An operand that is already on the device: (rows, max bits)."""
    return isinstance(x, tuple) and len(x) == 2 and hasattr(x[0], "data_ptr")


_default_engine: Optional[Engine] = None


def default_engine() -> Engine:
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine()
    return _default_engine
