"""Homomorphic operations on Paillier ciphertexts, batched on the GPU engine.

With g = N + 1 a ciphertext c of m satisfies  c1 * c2 = Enc(m1 + m2),  c^k = Enc(k m)  and  (1 + b N) c = Enc(m + b)
(mod N^2).  The reference's README shows them as ``ciphertext += 100`` and ``ciphertext *= 3``; this module applies
them to many ciphertexts at once:

  * ``scale``: c_i^(k_i) — a scalar of any sign per ciphertext;
  * ``add`` / ``neg``: c_i * d_i and c_i^-1;
  * ``sum_groups``: the product of every group (ragged groups, any size);
  * ``linear_map``: the encrypted W x + b (dense rows or sparse ``{index: weight}`` rows, optional plaintext bias);
  * ``matmul``: the same public W applied to a BATCH of ciphertext vectors (encrypted scoring, linear layers): W is
    planned and uploaded once, and the kernel reads every weight row once per wavefront of samples.  The weights are
    public plaintexts — the kernel's control flow depends on them;
  * ``conv2d`` / ``conv1d``: a public kernel slid over grids (or series) of ciphertexts — FIR filters and moving sums
    over an encrypted time series, a convolution layer over an encrypted image.  Every pixel gets one table however
    many windows cover it.  Cross-correlation, as ``torch.nn.functional.conv2d``; the kernel is public;
  * ``histogram``: the product of the ciphertexts of every (feature, bin) for a PUBLIC bin index per feature and
    sample — the per-feature, per-bin sums of encrypted gradients that gradient-boosted trees are built on, grouped
    encrypted statistics by public categories.  Weight-1 products only: no ciphertext needs an inverse;
  * ``sparse_matmul``: a public sparse matrix in CSR form (arrays the caller already holds, or a torch sparse tensor)
    times a vector of ciphertexts — the gradient X^T Enc(d) over sparse features, neighbourhood sums over a public
    adjacency matrix, weighted GROUP BY.  Planned with array operations, however many non-zeros there are;
  * ``cumsum``: the running totals along series of ciphertexts, c_0 c_1 ... c_j for every j — the left and right
    gradient sums of every split threshold straight from ``histogram`` output, cumulative distributions and running
    totals over an encrypted time series, summed-area rows.  One product per element and level, exclusive and
    reverse forms, no inverse of any input.

Ciphertexts are ints or objects with ``get_value()`` (the reference's ``PaillierCiphertext``); for objects the modulus
comes from ``.scheme.public_key.n`` unless ``n`` is given, and ``get_value()`` is called once per distinct object.  The
results are ints: canonical residues in [0, N^2), NOT fresh ciphertexts (every prefix of ``cumsum`` included) —
re-randomise them
(``Engine.randomize_batch``) before they leave the party.  ``engine`` is injected for tests; the default is the
process-wide HIP engine.

Every function takes ``randomizer=None``: given a ``randomizer.FastRandomizer`` of the same N, every result is
multiplied by a power h_s^a of the randomiser's fixed base on the device, before the rows are fetched — see that
module for what this randomiser is and is not.  Without one, behaviour and results are unchanged.
"""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence


def _engine(engine: Any) -> Any:
    if engine is not None:
        return engine
    from .engine import default_engine

    return default_engine()


def _values(cts: Sequence[Any], n: Optional[int]):
    """(ints, n): get_value() once per distinct object."""
    cache: Dict[int, int] = {}
    out: List[int] = []
    for c in cts:
        if isinstance(c, int):
            out.append(c)
            continue
        key = id(c)
        if key not in cache:
            cache[key] = int(c.get_value())
            if n is None:
                n = int(c.scheme.public_key.n)
        out.append(cache[key])
    if n is None:
        raise ValueError("the modulus n is needed when the ciphertexts are plain ints")
    return out, int(n)


def _fresh(randomizer: Any, n: int, count: int) -> Dict[str, Any]:
    """The engine keyword that re-randomises `count` results with `randomizer` (nothing without one)."""
    if randomizer is None:
        return {}
    return {"fixed_base": randomizer.spec(n, count)}


def scale(cts: Sequence[Any], scalars: Sequence[int], n: Optional[int] = None, engine: Any = None,
          randomizer: Any = None) -> List[int]:
    """[c^k mod N^2] for every (c, k) — the plaintexts multiplied by k."""
    vals, n = _values(cts, n)
    return _engine(engine).ciphertext_scale_batch(vals, [int(k) for k in scalars], n, **_fresh(randomizer, n, len(vals)))


def add(a: Sequence[Any], b: Sequence[Any], n: Optional[int] = None, engine: Any = None, randomizer: Any = None) -> List[int]:
    """[c * d mod N^2] for every pair — the plaintexts added."""
    if len(a) != len(b):
        raise ValueError("operands must have the same length")
    va, n = _values(list(a) + list(b), n)
    k = len(a)
    if k == 0:
        return []
    n2 = n * n
    return _engine(engine).mulmod_batch([v % n2 for v in va[:k]], [v % n2 for v in va[k:]], n2, **_fresh(randomizer, n, k))


def neg(cts: Sequence[Any], n: Optional[int] = None, engine: Any = None, randomizer: Any = None) -> List[int]:
    """[c^-1 mod N^2] — the plaintexts negated (ValueError, as pow, for a ciphertext without an inverse)."""
    vals, n = _values(cts, n)
    if not vals:
        return []
    return _engine(engine).modinv_batch(vals, n * n, **_fresh(randomizer, n, len(vals)))


def sum_groups(groups: Sequence[Sequence[Any]], n: Optional[int] = None, engine: Any = None, randomizer: Any = None) -> List[int]:
    """[prod(g) mod N^2] for every group — the sum of its plaintexts (an empty group gives 1, an encryption of 0)."""
    groups = [list(g) for g in groups]
    flat, n = _values([c for g in groups for c in g], n)
    out, pos = [], 0
    for g in groups:
        out.append(flat[pos : pos + len(g)])
        pos += len(g)
    return _engine(engine).ciphertext_sum_batch(out, n, **_fresh(randomizer, n, len(out)))


def linear_map(cts: Sequence[Any], weights: Sequence[Any], n: Optional[int] = None, bias: Optional[Sequence[int]] = None,
               engine: Any = None, randomizer: Any = None) -> List[int]:
    """The encrypted W x + b: [(1 + (b_j mod N) N) prod_i c_i^(W_ji) mod N^2 for every row j of W]."""
    vals, n = _values(cts, n)
    weights = list(weights)
    return _engine(engine).ciphertext_linear_map_batch(vals, weights, n, bias=bias, **_fresh(randomizer, n, len(weights)))


def matmul(x: Sequence[Sequence[Any]], weights: Sequence[Any], n: Optional[int] = None, bias: Optional[Sequence[int]] = None,
           engine: Any = None, randomizer: Any = None) -> List[List[int]]:
    """The encrypted W x_b + bias of every sample x_b of a batch: [[(1 + (bias_j mod N) N) prod_i x[b][i]^(W_ji) mod N^2
    for every row j of W] for every b].  All samples have the same length; W (dense rows or ``{column: weight}``) and the
    bias are public plaintexts."""
    samples = [list(smp) for smp in x]
    if not samples:
        return []
    for b, smp in enumerate(samples):
        if len(smp) != len(samples[0]):
            raise ValueError(f"sample {b} has {len(smp)} ciphertexts, sample 0 has {len(samples[0])}")
    flat, n = _values([c for smp in samples for c in smp], n)
    width = len(samples[0])
    vals = [flat[b * width : (b + 1) * width] for b in range(len(samples))]
    weights = weights if hasattr(weights, "shape") else list(weights)
    return _engine(engine).ciphertext_matmul_batch(vals, weights, n, bias=bias, **_fresh(randomizer, n, len(samples) * len(weights)))


def conv2d(x: Sequence[Any], weights: Any, n: Optional[int] = None, bias: Optional[Sequence[int]] = None, stride: Any = 1,
           padding: Any = 0, dilation: Any = 1, engine: Any = None, randomizer: Any = None) -> List[List[List[List[int]]]]:
    """The encrypted convolution of every grid x[b] ([C][H][W] ciphertexts) with the public kernel ``weights``
    ([O][C][kh][kw] signed ints) and the public ``bias`` ([O]):

        Y[b][o][y][x] = (1 + (bias_o mod N) N) prod_(c,i,j) X[b][c][y sh - ph + i dh][x sw - pw + j dw]^(w[o][c][i][j])  mod N^2

    as nested lists [B][O][H'][W'] with H' = (H + 2 ph - dh (kh - 1) - 1) // sh + 1.  ``stride``, ``padding`` (zeros: a tap
    outside the grid contributes 1) and ``dilation`` are ints or pairs (rows, columns).  Cross-correlation — the kernel
    is not flipped."""
    grids = [[[list(r) for r in ch] for ch in img] for img in x]
    flat, n = _values([c for img in grids for ch in img for r in ch for c in r], n)
    it = iter(flat)
    vals = [[[[next(it) for _ in r] for r in ch] for ch in img] for img in grids]
    fresh = {}
    if randomizer is not None:
        from . import conv_plan as cp

        rows = grids[0][0] if grids and grids[0] else [[None]]
        kernel = cp.kernel_array(weights)
        out_h, out_w = cp.output_hw(len(rows), len(rows[0]) if rows else 0, kernel.shape[2], kernel.shape[3], stride, padding, dilation)
        fresh = _fresh(randomizer, n, len(grids) * kernel.shape[0] * out_h * out_w)
    return _engine(engine).ciphertext_conv2d_batch(vals, weights, n, bias=bias, stride=stride, padding=padding,
                                                   dilation=dilation, **fresh)


def conv1d(x: Sequence[Any], weights: Any, n: Optional[int] = None, bias: Optional[Sequence[int]] = None, stride: int = 1,
           padding: int = 0, dilation: int = 1, engine: Any = None, randomizer: Any = None) -> List[List[List[int]]]:
    """conv2d for series: x[b] is [C][L] ciphertexts, ``weights`` [O][C][k]; the result is [B][O][L'].  The H = kh = 1
    case with scalar stride, padding and dilation."""
    y = conv2d([[[list(ch)] for ch in series] for series in x], [[[list(taps)] for taps in ker] for ker in weights], n=n,
               bias=bias, stride=(1, int(stride)), padding=(0, int(padding)), dilation=(1, int(dilation)), engine=engine,
               randomizer=randomizer)
    return [[ch[0] for ch in img] for img in y]


def histogram(cts: Sequence[Any], bins: Any, n_bins: int, n: Optional[int] = None, engine: Any = None,
              randomizer: Any = None) -> List[List[int]]:
    """[[prod(c_i for i with bins[f][i] == b) mod N^2 for b in range(n_bins)] for every feature f] — the sum of the
    plaintexts of every bin (an empty bin gives 1, an encryption of 0).  ``bins`` (nested lists, a numpy array or a
    torch tensor ``[F][len(cts)]``) is PUBLIC: values in [0, n_bins), or -1 for a sample that is not in this feature's
    histogram.  ValueError for anything else, before anything is launched; shape and dtype before a ciphertext is read
    (the values of ``bins`` are checked once, by the engine)."""
    from . import hist_plan as hp

    count = len(cts)
    bins_t = hp.as_bins(bins, count)
    hp.check_bins(bins_t, count, n_bins, values=False)
    vals, n = _values(cts, n)
    return _engine(engine).ciphertext_histogram_batch(vals, bins_t, int(n_bins), n, **_fresh(randomizer, n, bins_t.shape[0] * int(n_bins)))


def sparse_matmul(cts: Sequence[Any], matrix: Any, n: Optional[int] = None, bias: Optional[Sequence[int]] = None,
                  engine: Any = None, randomizer: Any = None) -> List[int]:
    """The encrypted A x + b for a PUBLIC sparse matrix A: [(1 + (b_r mod N) N) prod_t c_(col[t])^(val[t]) mod N^2 over
    the stored terms t of row r, for every row r].  ``matrix`` is a ``(crow, col, val)`` triple in CSR form (nested lists,
    numpy arrays or torch tensors; signed ``val`` with |val| <= 2^63 - 1) or a torch sparse CSR or COO tensor of an
    integer dtype with ``len(cts)`` columns (converted by torch's own ``to_sparse_csr``).  A negative weight uses the
    inverse of its ciphertext (ValueError, as ``neg``, if it has none), duplicate entries are terms of their own, a stored
    0 contributes nothing, an empty row gives 1 or its bias factor.  ValueError for anything else, before anything is
    launched; shape and dtype before a ciphertext is read (the values of the matrix are checked once, by the engine)."""
    from . import spmm_plan as sp

    crow, col, val = sp.as_matrix(matrix, len(cts))
    rows = crow.numel() - 1
    sp.check_bias(bias, rows)
    vals, n = _values(cts, n)
    return _engine(engine).ciphertext_spmm_batch(vals, crow, col, val, n, bias=bias, **_fresh(randomizer, n, rows))


def cumsum(series: Sequence[Any], n: Optional[int] = None, exclusive: bool = False, reverse: bool = False, engine: Any = None,
           randomizer: Any = None) -> List[Any]:
    """The running totals of a series of ciphertexts: ``out[j] = c_0 * ... * c_j mod N^2``, the sum of the plaintexts up
    to j.  ``series`` is a flat sequence of ciphertexts (a flat list comes back) or a sequence of sequences, every one a
    series of its own (lists of the same ragged shape come back; an empty series gives an empty list).
    ``exclusive=True`` leaves c_j out: ``out[0] = 1``, an encryption of 0.  ``reverse=True`` scans from the end:
    ``out[j] = c_j * ... * c_last``.  No input needs an inverse; a 0 makes every later prefix of its series 0."""
    series = list(series)
    nested = [isinstance(s, (list, tuple)) for s in series]
    if any(nested) and not all(nested):
        raise ValueError("series must be ciphertexts or sequences of ciphertexts, not both")
    is_nested = bool(series) and all(nested)
    lengths = [len(s) for s in series] if is_nested else [len(series)]
    flat = [c for s in series for c in s] if is_nested else series
    if not flat:
        return [[] for _ in series] if is_nested else []
    vals, n = _values(flat, n)
    out = _engine(engine).ciphertext_cumsum_batch(vals, lengths, n, exclusive=bool(exclusive), reverse=bool(reverse),
                                                  **_fresh(randomizer, n, len(vals)))
    if not is_nested:
        return out
    ends = [0]
    for k in lengths:
        ends.append(ends[-1] + k)
    return [out[a:b] for a, b in zip(ends, ends[1:])]
