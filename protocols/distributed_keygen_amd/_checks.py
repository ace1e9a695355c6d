"""Argument coercion and the operand checks that the engine (engine.py), the proof compositions (proof_flows.py) and the
private-key compositions (key_flows.py) share.  Imports neither torch nor the native library."""

from __future__ import annotations

from typing import Optional, Tuple

from . import limbs as _limbs


def _int_args(fn):
    """Coerce the integer operands of an entry point once: parameters annotated ``int`` become Python ints and the
    per-group operand lists (``mods``, ``exps``, ``coeffs``, ``primes`` annotated ``Sequence[int]``) lists of Python
    ints, so that int-like values — gmpy2.mpz when the reference's utils run on gmpy2, numpy integers — behave like the
    ints the reference passes (its own leaf accepts them)."""
    import functools
    import inspect

    params = inspect.signature(fn).parameters
    names = list(params)
    scalars = {k for k, q in params.items() if q.annotation == "int"}
    lists = {k for k, q in params.items() if q.annotation == "Sequence[int]" and k in ("mods", "exps", "coeffs", "primes")}
    if not scalars and not lists:
        return fn

    def conv(name, v):
        if name in scalars:
            return v if type(v) is int else int(v)
        if name in lists and not (isinstance(v, list) and all(type(x) is int for x in v[:1])):
            return [int(x) for x in v]
        return v

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        args = tuple(conv(names[i], a) if i < len(names) else a for i, a in enumerate(args))
        kwargs = {k: conv(k, v) for k, v in kwargs.items()}
        return fn(*args, **kwargs)

    return wrapper


def _check_modulus(mod: int) -> None:
    if mod < 3 or mod % 2 == 0:
        raise ValueError("modulus must be odd and >= 3 (Paillier moduli N and N^2 are)")


def _check_rows_n2(n: int, limbs2: int) -> None:
    if _limbs.limbs_for(n * n) > limbs2:
        raise ValueError("rows narrower than N^2")


def _is_device_rows(x) -> bool:
    """Rows that are already a device tensor (not a numpy array, not a sequence of ints)."""
    return hasattr(x, "data_ptr") and hasattr(x, "device")


def _nsquare(n: int) -> Tuple[int, int]:
    """(N^2, limbs of its rows) for a valid Paillier modulus N."""
    _check_modulus(n)
    n2 = n * n
    return n2, _limbs.limbs_for(n2)


class RowChecks:
    """The row check both mix-ins (proof_flows.ProofFlows, key_flows.PrivateKeyFlows) and the engine inherit; it reads
    ``self.torch`` and ``self.device``."""

    def _word_rows(self, rows_t, what: str, width: Optional[int] = None) -> Tuple[int, int]:
        if not _is_device_rows(rows_t) or rows_t.dim() != 2 or rows_t.dtype != self.torch.int32 or not rows_t.is_contiguous():
            raise ValueError(f"{what} must be contiguous int32 device rows [count, words]")
        if rows_t.device != self.device:
            raise ValueError(f"{what} live on {rows_t.device}, the operation runs on {self.device}")
        rows, words = rows_t.shape
        if words < 1 or (width is not None and words != width):
            raise ValueError(f"{what} must have {'at least one word' if width is None else f'{width} words'}")
        return rows, words
