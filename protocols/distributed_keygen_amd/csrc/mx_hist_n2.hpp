// Histogram modulo a SQUARE:  H[f][b] = prod_{i : bins[f][i] == b} c_i  mod N^2  — the sums of Paillier ciphertexts by
// a public bin index.  Weight-1 products only, on the pair arithmetic of mx_powmod_n2.hpp
// (PairArithT::mul, the conversion constants of mx_powmod_nsquare_prepare): no weights, no windows, no squarings, no
// inversions — a ciphertext without an inverse modulo N^2 is a legal input.
//
//   convert     (hist_n2_convert_kernel): one group of lanes per ciphertext; writes its pair-form ROW once (pair_convert).
//               One more group writes the domain's one (ONE0, ONE1) behind the last sample: row n_samples.  There is no
//               2^w table: nothing but the row itself is ever read.
//   accumulate  (hist_n2_kernel): one group of lanes per PIECE; acc = one, then `chunk` pair multiplications by
//               rows[index[piece][t]].  Every group of a launch runs the same trip count: control flow depends on the
//               launch shape only (the property DESIGN §3 and the cross-lane carries of mx_lanes.hpp rely on); only the
//               row ADDRESS depends on the index.  Ragged bins are the index array's business: the host cuts every
//               (feature, bin) segment into ceil(len / chunk) pieces and pads the last one with the index of the one row.
//   combine     the same kernel over the previous level's piece rows: with pair_out it writes its products in pair form
//               (and the one row behind them: row `pieces`), so a level's output is the next level's input as it stands.
//               The last level runs the shared epilogue (pair_store): canonical residues in [0, N^2).
//
// Row layout: the table entry of mx_multiexp_n2.hpp — 2 * L * K contiguous words, word ((half * L + j) * K + p) for limb
// j of lane p: a group reads one contiguous, lane-consecutive span per product.  Every row address is 64-bit and the
// index is clamped into the row set (a wrong index array gives wrong values, never an access outside the rows).
#pragma once
#include "mx_powmod_n2.hpp"

namespace mx {

struct HistN2Args {
  const u32* inputs;    // convert: [n_samples][limbs2] residues < N^2
  u32* rows_out;        // convert: [n_samples + 1][2][L][K], the last row the domain's one
  const u32* rows;      // accumulate: [n_rows + 1][2][L][K] pair-form rows, row n_rows the domain's one
  const u32* consts;    // [8][limbsn] the plan's constant rows of this geometry: N, ONE0, ONE1, K1_0, K1_1, K2_0, K2_1, C'
  const int* index;     // [pieces][chunk] row of every term (n_rows: the one row)
  u32* out;             // pair_out: [pieces + 1][2][L][K], the last row the domain's one; otherwise [pieces][limbs2]
  i64 n_samples, n_rows, pieces;
  int chunk, pair_out;
  int limbsn, limbs2, nblk;
  int ksplit;           // x = x_lo + 2^ksplit * x_hi, ksplit = bits(N) - 1
};

template <int K, int L>
constexpr size_t hist_n2_lds_bytes() { return powmod_n2_lds_bytes<K, L>(false); }

// (a0, a1) to the pair-form row `dst` (already offset by the lane)
template <int K, int L>
__device__ __forceinline__ void hist_put_row(u32* dst, const u32 (&a0)[L], const u32 (&a1)[L], bool valid) {
  if (!valid) return;
#pragma unroll
  for (int j = 0; j < L; ++j) { dst[j * K] = a0[j]; dst[(L + j) * K] = a1[j]; }
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) hist_n2_convert_kernel(HistN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  constexpr int WIDE = M_t::LDS_WORDS;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const bool valid = raw <= A.n_samples;            // group n_samples writes the one row
  const bool is_one = raw >= A.n_samples;
  const i64 e = raw < A.n_samples ? raw : A.n_samples - 1;      // surplus groups redo the last sample and store nothing
  M_t M;
  u32* cp_lds = pair_setup<K, L>(M, smem, gw, A.consts, A.limbsn, A.nblk);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  u32* wide = smem + gw * M_t::LDS_WORDS;
  const u32* src = A.inputs + e * A.limbs2;
  __syncthreads();
  for (int k = p; k < WIDE; k += K) wide[k] = (k < A.limbs2) ? src[k] : 0u;
  __syncthreads();
  u32 x0[L], x1[L];
  pair_convert<W>(M, P, wide, A.consts, A.limbsn, A.ksplit, x0, x1);
  {
    u32 t0[L], t1[L];
    M.load(t0, A.consts + 1 * A.limbsn, A.limbsn);          // the domain's one
    M.load(t1, A.consts + 2 * A.limbsn, A.limbsn);
#pragma unroll
    for (int j = 0; j < L; ++j) { x0[j] = is_one ? t0[j] : x0[j]; x1[j] = is_one ? t1[j] : x1[j]; }
  }
  const i64 row = raw < A.n_samples ? raw : A.n_samples;
  hist_put_row<K, L>(A.rows_out + row * ((i64)2 * L * K) + p, x0, x1, valid);
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) hist_n2_kernel(HistN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const i64 r = raw < A.pieces ? raw : A.pieces - 1;    // surplus groups redo the last piece
  M_t M;
  u32* cp_lds = pair_setup<K, L>(M, smem, gw, A.consts, A.limbsn, A.nblk);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  u32 acc0[L], acc1[L];
  M.load(acc0, A.consts + 1 * A.limbsn, A.limbsn);   // the domain's one
  M.load(acc1, A.consts + 2 * A.limbsn, A.limbsn);
  const i64 row_words = (i64)2 * L * K;
  const u32* rows = A.rows + p;
  const int* idx_row = A.index + r * A.chunk;
  const int last = (int)A.n_rows;                    // the one row
  // the index of term t + 1 is loaded before the product of term t, so that only the row load waits for it
  int i = idx_row[0];
  for (int t = 0; t < A.chunk; ++t) {
    i = i < 0 ? 0 : (i > last ? last : i);
    const u32* f = rows + (i64)i * row_words;
    u32 f0[L], f1[L];
#pragma unroll
    for (int j = 0; j < L; ++j) { f0[j] = f[j * K]; f1[j] = f[(L + j) * K]; }
    i = idx_row[t + 1 < A.chunk ? t + 1 : t];
    P.mul(acc0, acc1, acc0, acc1, f0, f1);
  }
  if (A.pair_out) {
    // piece rows of the next level; group `pieces` (one always exists: the host launches pieces + 1 groups) writes the one
    const bool is_one = raw >= A.pieces;
    u32 t0[L], t1[L];
    M.load(t0, A.consts + 1 * A.limbsn, A.limbsn);
    M.load(t1, A.consts + 2 * A.limbsn, A.limbsn);
#pragma unroll
    for (int j = 0; j < L; ++j) { acc0[j] = is_one ? t0[j] : acc0[j]; acc1[j] = is_one ? t1[j] : acc1[j]; }
    const i64 row = raw < A.pieces ? raw : A.pieces;
    hist_put_row<K, L>(A.out + row * row_words + p, acc0, acc1, raw <= A.pieces);
  } else {
    pair_store<K, W>(M, P, acc0, acc1, smem + gw * M_t::LDS_WORDS, A.nblk, A.out + r * A.limbs2, A.limbs2, raw < A.pieces);
  }
}

}  // namespace mx
