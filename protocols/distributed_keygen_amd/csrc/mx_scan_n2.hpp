// Prefix products modulo a SQUARE:  out[j] = c_0 * c_1 * ... * c_j  mod N^2  over the terms of a piece — the running
// totals of Paillier ciphertexts.  The accumulate kernel of mx_hist_n2.hpp with every intermediate
// product stored: the same pair-form rows (hist_n2_convert_kernel writes them), the same [pieces][chunk] index array,
// the same arithmetic (PairArithT::mul), no weights, windows, squarings or inversions.
//
//   scan   (scan_n2_kernel): one group of lanes per PIECE; acc = the piece's carry — row carry_index[piece] of a second
//          row set, the product of everything before the piece in its segment; the domain's one without a carry set —
//          then `chunk` pair multiplications by rows[index[piece][t]].  Inclusive: multiply, then store; exclusive:
//          store, then multiply.  The product of term t goes to the OUTPUT row index[piece][t], the input row's own
//          number: there is no destination array, and a reverse scan is a reversed index array.  A term that names the
//          one row (the padding of a piece) stores nothing.  Products are stored in pair form (hist_put_row); the
//          launch's surplus group writes the one row behind the last row, so the output is a row set again: the carries
//          of the level below, or the input of the store pass.
//   store  (scan_n2_store_kernel): one group of lanes per row; the shared epilogue (pair_store) over a row set:
//          canonical residues in [0, N^2).  A pass of its own: inside the scan loop pair_store has to sit beside the
//          accumulator and the loop's addresses, which at three wavefronts per SIMD spilled 8 to 43 registers in
//          every form tried, and a private segment is not accepted in this library.
//
// Every group of a launch runs the same trip count: control flow depends on the launch shape only; stores are
// predicated per group and term.  Row addresses are 64-bit; the index and the carry index are clamped into their row
// sets (a wrong array gives wrong values, never an access outside the rows).
#pragma once
#include "mx_hist_n2.hpp"

namespace mx {

struct ScanN2Args {
  const u32* rows;         // [n_rows + 1][2][L][K] pair-form rows, row n_rows the domain's one
  const u32* carry_rows;   // scan: [n_carry_rows + 1] pair-form rows, or null: every piece starts from the one
  const u32* consts;       // [8][limbsn] the plan's constant rows of this geometry (mx_hist_n2.hpp)
  const int* index;        // scan: [pieces][chunk] row of every term (n_rows: the one row, nothing stored)
  const int* carry_index;  // scan: [pieces] row of carry_rows the piece starts from (n_carry_rows: the one row)
  u32* out;                // scan: [n_rows + 1][2][L][K], the last row the domain's one;  store: [n_rows][limbs2]
  i64 n_rows, n_carry_rows, pieces;
  int chunk, exclusive;
  int limbsn, limbs2, nblk;
};

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) scan_n2_kernel(ScanN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const bool live = raw < A.pieces;
  const i64 r = live ? raw : A.pieces - 1;              // surplus groups redo the last piece and store nothing
  M_t M;
  u32* cp_lds = pair_setup<K, L>(M, smem, gw, A.consts, A.limbsn, A.nblk);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  const i64 row_words = (i64)2 * L * K;
  u32 acc0[L], acc1[L];
  if (A.carry_rows) {
    int ci = A.carry_index[r];
    const int clast = (int)A.n_carry_rows;
    ci = ci < 0 ? 0 : (ci > clast ? clast : ci);
    const u32* c = A.carry_rows + p + (i64)ci * row_words;
#pragma unroll
    for (int j = 0; j < L; ++j) { acc0[j] = c[j * K]; acc1[j] = c[(L + j) * K]; }
  } else {
    M.load(acc0, A.consts + 1 * A.limbsn, A.limbsn);    // the domain's one
    M.load(acc1, A.consts + 2 * A.limbsn, A.limbsn);
  }
  const u32* rows = A.rows + p;
  u32* out = A.out + p;
  const int* idx_row = A.index + r * A.chunk;
  const int last = (int)A.n_rows;                       // the one row
  // One loop body for both forms: trip t stores acc at row `at`, then multiplies by term t.  Exclusive: `at` is the row
  // of term t itself.  Inclusive: `at` is the row of term t - 1 (none at t == 0), and one more trip stores the last
  // product and multiplies by nothing.  The trip count depends on the launch alone.  The index of term t + 1 is loaded
  // before the product of term t, so that only the row load waits for it.
  const int trips = A.chunk + (A.exclusive ? 0 : 1);
  int i = idx_row[0];
  int at = last;
  for (int t = 0; t < trips; ++t) {
    i = i < 0 ? 0 : (i > last ? last : i);
    if (A.exclusive) at = i;
    hist_put_row<K, L>(out + (i64)at * row_words, acc0, acc1, live && at != last);
    if (t < A.chunk) {
      const u32* f = rows + (i64)i * row_words;
      u32 f0[L], f1[L];
#pragma unroll
      for (int j = 0; j < L; ++j) { f0[j] = f[j * K]; f1[j] = f[(L + j) * K]; }
      at = i;
      i = idx_row[t + 1 < A.chunk ? t + 1 : t];
      P.mul(acc0, acc1, acc0, acc1, f0, f1);
    }
  }
  if (raw == A.pieces) {
    // the one row behind the last row (one surplus group always exists: the host launches pieces + 1 groups)
    M.load(acc0, A.consts + 1 * A.limbsn, A.limbsn);
    M.load(acc1, A.consts + 2 * A.limbsn, A.limbsn);
    hist_put_row<K, L>(out + A.n_rows * row_words, acc0, acc1, true);
  }
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) scan_n2_store_kernel(ScanN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const i64 r = raw < A.n_rows ? raw : A.n_rows - 1;    // surplus groups redo the last row and store nothing
  M_t M;
  u32* cp_lds = pair_setup<K, L>(M, smem, gw, A.consts, A.limbsn, A.nblk);
  PairArith<K, L, W> P(M, cp_lds);
  const u32* f = A.rows + M.p + r * ((i64)2 * L * K);
  u32 acc0[L], acc1[L];
#pragma unroll
  for (int j = 0; j < L; ++j) { acc0[j] = f[j * K]; acc1[j] = f[(L + j) * K]; }
  pair_store<K, W>(M, P, acc0, acc1, smem + gw * M_t::LDS_WORDS, A.nblk, A.out + r * A.limbs2, A.limbs2, raw < A.n_rows);
}

}  // namespace mx
