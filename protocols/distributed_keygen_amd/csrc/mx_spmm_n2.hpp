// Sparse matrix products modulo a SQUARE:  y_r = prod_t x_{col[t]} ^ val[t]  mod N^2  over the stored terms of row r of
// a public CSR matrix — weighted sums of Paillier ciphertexts by a sparse public matrix.  The weights
// are cut into w-bit digits; every non-zero digit is a weight-1 term of the (row, digit position) segment it belongs
// to, so the products of the segments are a histogram (mx_hist_n2.hpp) over a table of small powers, and the
// positions of a row are folded by Horner's rule.  The two kernels on either side of mx_histogram_nsquare_run:
//
//   tables  (spmm_n2_table_kernel): one group of lanes per input; converts the row into pair form (pair_convert) and
//           writes x^1 .. x^(2^w - 1) as ROWS OF A HISTOGRAM ROW SET: entry (input i, digit d) is row
//           i * (2^w - 1) + d - 1, and one more group writes the domain's one behind the last row.  The accumulate
//           kernel reads the table as it stands.  With w = 1 this is the conversion alone.  There is no entry for the
//           digit 0: a zero digit is no term.
//   horner  (spmm_n2_horner_kernel): one group of lanes per output row over the row set S of the segment products, row
//           r * D + p the product of row r at digit position p:  acc = S[r][D - 1]; for p = D - 2 .. 0: w pair
//           squarings and one pair multiplication by S[r][p]; then one multiplication by the row's converted bias
//           factor, if the launch has any; then the shared epilogue (pair_store): a canonical residue in [0, N^2).
//
// Every group of a launch runs the same trip counts — (2^w - 2) products, (D - 1) (w + 1) products — which depend on
// the launch's (D, w) alone: control flow is wave-uniform (the property DESIGN §3 and the cross-lane carries of
// mx_lanes.hpp rely on).  Row layout and addressing are those of mx_hist_n2.hpp; every row address is 64-bit.
#pragma once
#include "mx_hist_n2.hpp"

namespace mx {

struct SpmmN2Args {
  const u32* inputs;     // tables: [n_inputs][limbs2] residues < N^2
  u32* rows_out;         // tables: [n_inputs * entries + 1][2][L][K], the last row the domain's one
  const u32* rows;       // horner: [n_rows * positions + 1][2][L][K] pair-form segment products
  const u32* bias_rows;  // horner: [n_rows][2][L][K] pair-form bias factors, or null
  const u32* consts;     // [8][limbsn] the plan's constant rows of this geometry (mx_hist_n2.hpp)
  u32* out;              // horner: [n_rows][limbs2]
  i64 n_inputs, n_rows;
  int entries;           // 2^window - 1 rows per input
  int positions, window;
  int limbsn, limbs2, nblk;
  int ksplit;            // x = x_lo + 2^ksplit * x_hi, ksplit = bits(N) - 1
};

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) spmm_n2_table_kernel(SpmmN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  constexpr int WIDE = M_t::LDS_WORDS;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const bool live = raw < A.n_inputs;
  const i64 e = live ? raw : A.n_inputs - 1;        // surplus groups redo the last input and store none of its powers
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
  const i64 row_words = (i64)2 * L * K;
  u32* dst = A.rows_out + p + e * A.entries * row_words;
  hist_put_row<K, L>(dst, x0, x1, live);
  u32 t0[L], t1[L];
#pragma unroll
  for (int j = 0; j < L; ++j) { t0[j] = x0[j]; t1[j] = x1[j]; }
  // x^d = x^(d-1) * x
  for (int d = 2; d <= A.entries; ++d) {
    P.mul(t0, t1, t0, t1, x0, x1);
    dst += row_words;
    hist_put_row<K, L>(dst, t0, t1, live);
  }
  // group n_inputs (one always exists: the host launches n_inputs + 1 groups) writes the one row behind the table
  M.load(t0, A.consts + 1 * A.limbsn, A.limbsn);
  M.load(t1, A.consts + 2 * A.limbsn, A.limbsn);
  hist_put_row<K, L>(A.rows_out + p + A.n_inputs * A.entries * row_words, t0, t1, raw == A.n_inputs);
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) spmm_n2_horner_kernel(SpmmN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const i64 r = raw < A.n_rows ? raw : A.n_rows - 1;    // surplus groups redo the last row and store nothing
  M_t M;
  u32* cp_lds = pair_setup<K, L>(M, smem, gw, A.consts, A.limbsn, A.nblk);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  const i64 row_words = (i64)2 * L * K;
  const u32* seg = A.rows + p + r * A.positions * row_words;
  u32 acc0[L], acc1[L];
  {
    const u32* f = seg + (i64)(A.positions - 1) * row_words;
#pragma unroll
    for (int j = 0; j < L; ++j) { acc0[j] = f[j * K]; acc1[j] = f[(L + j) * K]; }
  }
  for (int pos = A.positions - 2; pos >= 0; --pos) {
    for (int s = 0; s < A.window; ++s) P.sqr(acc0, acc1, acc0, acc1);
    const u32* f = seg + (i64)pos * row_words;
    u32 f0[L], f1[L];
#pragma unroll
    for (int j = 0; j < L; ++j) { f0[j] = f[j * K]; f1[j] = f[(L + j) * K]; }
    P.mul(acc0, acc1, acc0, acc1, f0, f1);
  }
  if (A.bias_rows) {                                     // the same for every group of the launch
    const u32* f = A.bias_rows + p + r * row_words;
    u32 f0[L], f1[L];
#pragma unroll
    for (int j = 0; j < L; ++j) { f0[j] = f[j * K]; f1[j] = f[(L + j) * K]; }
    P.mul(acc0, acc1, acc0, acc1, f0, f1);
  }
  pair_store<K, W>(M, P, acc0, acc1, smem + gw * M_t::LDS_WORDS, A.nblk, A.out + r * A.limbs2, A.limbs2, raw < A.n_rows);
}

}  // namespace mx
