"""Multi-GPU sharding of the hot path: one process per GPU, contiguous slices, ONE all-gather.

Every unit of the path is independent: the modexps of a batch, the candidates of a
sieve, the ciphertexts of a recombination.  So each rank takes a contiguous 1/world slice, runs the
same single-GPU operator on it, and the per-rank result rows are all-gathered
(``torch.distributed.all_gather_into_tensor`` — RCCL over xGMI with the ``nccl`` backend) so that
every rank ends with the full result, exactly like the reference's list comprehensions return the
full list (distributed_keygen.py:463-466, 510-515, 1288-1292, 1313-1329).  The shared operands
(modulus, exponent, prime list) are small and passed by value on every rank; no other collective
is needed.  For the biprimality test a candidate's bases stay on one GPU (its modulus and
exponent are loaded once) and the verdict bytes are what is gathered — the "vote".

Two input forms.  Replicated (default): every rank passes the FULL batch and works on its slice —
for callers that hold the whole list anyway, as the reference's loops do.  Shard-only
(``total=<units of the whole batch>``): a rank passes ONLY rows [lo, hi) of
``shard_bounds(total, rank, world)`` (and only that slice's moduli / exponents), so it packs and
uploads 1/world of the batch; the result is the same full, ordered tensor on every rank.

The functions take the tensor-level engine API, so they are backend-agnostic: the tests drive
them with the ``gloo`` backend on CPU tensors and a test double of the engine.  All of them are
``_sharded`` below with what varies passed as data.
"""

from __future__ import annotations

from typing import Any, Callable, Optional, Sequence, Tuple


def shard_bounds(total: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous, near-equal slice [lo, hi) of range(total) for `rank`."""
    per = -(-total // world)
    lo = min(total, rank * per)
    return lo, min(total, lo + per)


def _dist():
    import torch.distributed as dist

    return dist


def _world(group: Any) -> Tuple[int, int]:
    dist = _dist()
    if not (dist.is_available() and dist.is_initialized()):
        return 0, 1
    return dist.get_rank(group), dist.get_world_size(group)


def _pad_rows(t, rows: int, dim: int = 0, empty: int = 0):
    """Pad dimension `dim` of `t` to `rows` by repeating its last row (padding results are discarded)."""
    import torch

    have = t.shape[dim]
    if have == rows:
        return t
    if have == 0:        # an empty shard (fewer rows than ranks): nothing to repeat
        return torch.full(tuple(t.shape[:dim]) + (rows,) + tuple(t.shape[dim + 1 :]), empty, dtype=t.dtype, device=t.device)
    return torch.cat([t, t.narrow(dim, have - 1, 1).repeat_interleave(rows - have, dim=dim)], dim=dim)


def _gather_rows(local, world: int, group: Any):
    import torch

    dist = _dist()
    out = torch.empty((world * local.shape[0],) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, local.contiguous(), group=group)
    return out


def all_gather_rows(local, total_rows: int, group: Any = None):
    """For callers that hold ONLY their shard (rows [lo, hi) of shard_bounds(total_rows, rank, world),
    padded to ceil(total_rows / world) rows): run the single-GPU operator on the shard, then this —
    the one all-gather — to give every rank the full result in order.  The sharded_* functions below
    are this plus the slicing of a replicated input."""
    rank, world = _world(group)
    if world == 1:
        return local[:total_rows]
    per = -(-total_rows // world)
    return _gather_rows(_pad_rows(local, per), world, group)[:total_rows]


def _check_shard(rows: int, total: int, rank: int, world: int, unit: int = 1) -> int:
    """Shard-only input: `rows` must be this rank's slice of `total` units (`unit` rows each); returns units per rank."""
    lo, hi = shard_bounds(total, rank, world)
    if rows != (hi - lo) * unit:
        raise ValueError(f"rank {rank} of {world} holds {rows} rows; its shard of {total} units is [{lo}, {hi}) = {(hi - lo) * unit} rows")
    return -(-total // world)


def _pad_list(seq: Sequence[int], n: int, filler: int = 3) -> list:
    """Pad per-unit host operands to `n` (results of padding units are discarded; an empty shard gets a valid odd modulus)."""
    seq = list(seq)
    return seq + [seq[-1] if seq else filler] * (n - len(seq))


def _sharded(group: Any, total: Optional[int], whole: Callable, run: Callable, t, *, dim: int = 0, unit: int = 1,
             out_unit: int = 1, lists: Sequence[Tuple[Sequence[int], int]] = (), empty: int = 0, per_unit: str = "",
             unpack: Optional[Callable] = None):
    """What every sharded_* function is.  World 1: ``whole()``, the engine call itself.  Otherwise this rank's units of
    `t` — `unit` rows of dimension `dim` each; the slice of a replicated `t` (total None), or a shard-only `t` checked
    against `total` — and of the per-unit host `lists` (pairs of a list and its filler for an empty shard), padded to
    ceil(total / world) units by repeating the last one, so that a padding unit is a valid operand (an empty shard has
    none to repeat: rows of `empty`, the fillers); ``run(rows, *lists)`` on them, whose result has `out_unit` rows per
    unit; ONE all-gather; the padding trimmed; ``unpack`` where the result travelled as one row.  `per_unit` ends the
    refusal of shard-only lists that do not match the shard's rows."""
    rank, world = _world(group)
    if world == 1:
        return whole()
    if total is None:
        total = t.shape[dim] // unit
        per = -(-total // world)
        t = _pad_rows(t, per * world * unit, dim, empty).narrow(dim, rank * per * unit, per * unit)
        lists = [_pad_list(seq, per * world, filler)[rank * per : (rank + 1) * per] for seq, filler in lists]
    else:
        per = _check_shard(t.shape[dim], total, rank, world, unit)
        if any(len(seq) * unit != t.shape[dim] for seq, _ in lists):
            raise ValueError("shard-only input: " + per_unit)
        t = _pad_rows(t, per * unit, dim, empty)
        lists = [_pad_list(seq, per, filler) for seq, filler in lists]
    full = _gather_rows(run(t.contiguous(), *lists), world, group)[: total * out_unit]
    return unpack(full) if unpack else full


def sharded_powmod_shared(engine: Any, bases_t, mod: int, exp: int, group: Any = None, total: Optional[int] = None):
    """Full-batch ``engine.powmod_shared_t`` computed as world slices + one all-gather."""
    return _sharded(group, total, lambda: engine.powmod_shared_t(bases_t, mod, exp),
                    lambda rows: engine.powmod_shared_t(rows, mod, exp), bases_t)


def sharded_powmod_nsquare(engine: Any, bases_t, n: int, exp: int, group: Any = None, total: Optional[int] = None):
    """Full-batch ``engine.powmod_nsquare_t`` (partial decryptions modulo n^2) as world slices + one
    all-gather — the multi-GPU form of the loop distributed_keygen.py:463-466."""
    return _sharded(group, total, lambda: engine.powmod_nsquare_t(bases_t, n, exp),
                    lambda rows: engine.powmod_nsquare_t(rows, n, exp), bases_t)


def sharded_powmod_multi(
    engine: Any, bases_t, mods: Sequence[int], exps: Sequence[int], group_size: int, group: Any = None,
    total: Optional[int] = None,
):
    """``engine.powmod_multi_t`` with the candidate groups split across ranks (`total` = candidate groups of the whole
    batch when the caller passes only its shard's bases, moduli and exponents)."""
    return _sharded(group, total, lambda: engine.powmod_multi_t(bases_t, mods, exps, group_size),
                    lambda rows, m, e: engine.powmod_multi_t(rows, m, e, group_size), bases_t,
                    unit=group_size, out_unit=group_size, lists=[(mods, 3), (exps, 1)],
                    per_unit="one modulus and one exponent per candidate group of the shard")


def sharded_sieve(engine: Any, cands_t, primes: Sequence[int], group: Any = None, total: Optional[int] = None):
    """uint8 verdict per candidate; candidates split across ranks, verdict bytes all-gathered."""
    return _sharded(group, total, lambda: engine.sieve_t(cands_t, primes), lambda rows: engine.sieve_t(rows, primes), cands_t)


def sharded_combine(engine: Any, partials_t, n: int, theta_inv: int, group: Any = None, total: Optional[int] = None):
    """``engine.combine_t`` with the ciphertexts (dim 1 of partials_t) split across ranks.  Plaintext
    and status travel as ONE row per ciphertext (mx_combine_run's packed output), so the exchange is a
    single all-gather.  An empty shard is ones: they recombine to status 1 rows that the trim discards."""
    import torch

    return _sharded(group, total, lambda: engine.combine_t(partials_t, n, theta_inv),
                    lambda rows: engine.combine_t(rows, n, theta_inv, packed=True), partials_t, dim=1, empty=1,
                    unpack=lambda full: (full[:, :-1].contiguous(), full[:, -1].to(torch.uint8)))


def sharded_biprime_v(engine: Any, g_t, mods: Sequence[int], exps: Sequence[int], group_size: int, keep: int,
                      group: Any = None, total: Optional[int] = None):
    """The v-calculation of a keygen round (distributed_keygen.py:1084-1099 looped at :1313-1329) with
    the candidates split contiguously across ranks: every rank runs the fused Jacobi filter ->
    selection of the first `keep` generators -> `keep` modexps on ITS candidates
    (``engine.biprime_v_t``; a candidate's modulus, exponent and generators stay on one GPU), then ONE
    all-gather whose rows carry a candidate's `keep` v values and its count of valid ones.
    g_t: int32 [groups*group_size, limbs].  Returns (v rows [groups*keep, limbs], counts [groups])."""
    import torch

    limbs = g_t.shape[1]

    def run(rows, m, e):
        v_t, cnt_t = engine.biprime_v_t(rows, m, e, group_size, keep)
        return torch.cat([v_t.reshape(len(m), keep * limbs), cnt_t.reshape(len(m), 1).to(v_t.dtype)], dim=1)

    return _sharded(group, total, lambda: engine.biprime_v_t(g_t, list(mods), list(exps), group_size, keep), run, g_t,
                    unit=group_size, lists=[(mods, 3), (exps, 1)],
                    per_unit="one modulus and one exponent per candidate of the shard",
                    unpack=lambda full: (full[:, : keep * limbs].reshape(len(full) * keep, limbs).contiguous(), full[:, -1].contiguous()))


def sharded_biprime_vote(engine: Any, v_t, mods: Sequence[int], group: Any = None, total: Optional[int] = None):
    """Per-slot pass bytes [groups, n_slots] of ``engine.biprime_verdict_t`` with candidates split
    across ranks (v_t [parties, candidates, slots, limbs]); the pass bytes are all-gathered (the biprimality vote)."""
    return _sharded(group, total, lambda: engine.biprime_verdict_t(v_t, mods),
                    lambda rows, m: engine.biprime_verdict_t(rows, m), v_t, dim=1, lists=[(mods, 3)],
                    per_unit="one modulus per candidate of the shard")
