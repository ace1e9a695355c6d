// Multi-exponentiation modulo a SQUARE:  out[r] = prod_t inputs[index[r][t]] ^ weights[r][t]  mod N^2  (weights >= 0),
// the homomorphic linear map of Paillier ciphertexts.  Interleaved fixed-window (Straus) form on the
// pair arithmetic of mx_powmod_n2.hpp (PairArithT::mul / sqr, the conversion constants of mx_powmod_nsquare_prepare):
//
//   table pass  (multiexp_n2_table_kernel): one group of lanes per input; converts the row into pair form and writes
//               its 2^w powers, entry 0 being the domain's one (ONE0, ONE1), into the caller's workspace;
//   main pass   (multiexp_n2_kernel): one group of lanes per output row; acc = one, then for every w-bit window from
//               the top: w pair squarings (none in the top window), and one pair multiplication per term by
//               table[index][digit].  Digit 0 multiplies by one, padding terms carry weight 0: every group of a
//               wavefront executes the same number of windows and terms, so control flow stays wave-uniform (the
//               property DESIGN §3 relies on); only the table ADDRESS depends on the weights.  The last product is by
//               E = (1, 0) and the epilogue is the one of powmod_n2_kernel: a canonical residue in [0, N^2).
//
// Table layout: entry (input i, digit d) is 2 * L * K contiguous words, word ((half * L + j) * K + p) for limb j of
// lane p: one group reads one contiguous span of 2 K L words, lane-consecutive.  The host lays the terms of rows that
// share a wavefront out in the same input order, so the groups of a wavefront read the same input's table at the same
// step and share its L2 lines.
#pragma once
#include "mx_powmod_n2.hpp"

namespace mx {

struct MultiexpN2Args {
  const u32* inputs;    // [n_inputs][limbs2] (table pass): residues < N^2
  u32* tables;          // [n_inputs][1 << window][2][L][K] (workspace)
  const u32* consts;    // [8][limbsn] the plan's constant rows of this geometry: N, ONE0, ONE1, K1_0, K1_1, K2_0, K2_1, C'
  const int* index;     // [rows][terms] input of every term
  const u32* weights;   // [rows][terms][wwords] little-endian words of the non-negative weight
  u32* out;             // [rows][limbs2]
  i64 n_inputs, rows;
  int terms, wwords, nwin, window;
  int limbsn, limbs2, nblk;
  int ksplit;           // x = x_lo + 2^ksplit * x_hi, ksplit = bits(N) - 1
};

template <int K, int L>
constexpr size_t multiexp_n2_lds_bytes() { return powmod_n2_lds_bytes<K, L>(false); }

// The two kernels below keep their own set-up, conversion and epilogue, the code that pair_setup, pair_convert and
// pair_store (mx_powmod_n2.hpp) hold for the other homomorphic kernels: built on the shared functions — and again with
// only the epilogue their own — a map of 1000 outputs with 2048-bit weights measured 2 % slower (20.55 -> 21.0 ms, all four
// runs, profiles/r12_fold_probes_ab.txt) although the instruction streams differed by a handful of scalar instructions.
// A correction to one of the three pieces has to be made here as well.
//
// Set-up of both passes: the group's Montgomery state and C' in LDS (one copy per workgroup).
template <int K, int L, class M_t>
__device__ __forceinline__ u32* multiexp_n2_setup(M_t& M, u32* smem, int gw, const MultiexpN2Args& A) {
  constexpr int GPW = 64 / K;
  M.init(smem + gw * M_t::LDS_WORDS, A.nblk);
  M.load(M.n, A.consts, A.limbsn);
  M.setup_modulus();
  u32* cp_lds = smem + GPW * M_t::LDS_WORDS;
  u32 v[L];
  M.load(v, A.consts + 7 * A.limbsn, A.limbsn);
  if (gw == 0) {
#pragma unroll
    for (int j = 0; j < L; ++j) cp_lds[M.p * L + j] = v[j];
  }
  __syncthreads();
  return cp_lds;
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) multiexp_n2_table_kernel(MultiexpN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  constexpr int WIDE = M_t::LDS_WORDS;
  extern __shared__ u32 smem[];
  const int lane = threadIdx.x;
  const int gw = lane / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const bool valid = raw < A.n_inputs;
  const i64 e = valid ? raw : A.n_inputs - 1;       // surplus groups redo the last input and store nothing
  M_t M;
  u32* cp_lds = multiexp_n2_setup<K, L>(M, smem, gw, A);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  // the two halves of x = x_lo + 2^k x_hi, as powmod_n2_kernel's prologue splits them
  u32* wide = smem + gw * M_t::LDS_WORDS;
  const u32* src = A.inputs + e * A.limbs2;
  __syncthreads();
  for (int k = p; k < WIDE; k += K) wide[k] = (k < A.limbs2) ? src[k] : 0u;
  __syncthreads();
  u32 lo[L], hi[L], zero[L];
#pragma unroll
  for (int j = 0; j < L; ++j) {
    const int bit = W * (p * L + j);
    const int room = A.ksplit - bit;
    lo[j] = room <= 0 ? 0u : extract_field(wide, bit, room < W ? room : W);
    const int hbit = A.ksplit + bit;
    hi[j] = (hbit + W + 32 <= 32 * WIDE) ? extract_field(wide, hbit, W) : 0u;
    zero[j] = 0u;
  }
  // x = (x_lo, 0) * K1 + (x_hi, 0) * K2; constant pairs are loaded where they are used (keeping them all in registers
  // spilled)
  u32 x0[L], x1[L], t0[L], t1[L];
  M.load(t0, A.consts + 3 * A.limbsn, A.limbsn);
  M.load(t1, A.consts + 4 * A.limbsn, A.limbsn);
  P.mul(x0, x1, lo, zero, t0, t1);
  M.load(t0, A.consts + 5 * A.limbsn, A.limbsn);
  M.load(t1, A.consts + 6 * A.limbsn, A.limbsn);
  P.mul(t0, t1, hi, zero, t0, t1);
  M.add(x0, x0, t0);
  M.add(x1, x1, t1);
  const int entries = 1 << A.window;
  const i64 entry_words = (i64)2 * L * K;
  u32* tab = A.tables + e * entries * entry_words + p;
  auto put = [&](int d, const u32 (&a)[L], const u32 (&b)[L]) {
    if (!valid) return;
    u32* dst = tab + d * entry_words;
#pragma unroll
    for (int j = 0; j < L; ++j) { dst[j * K] = a[j]; dst[(L + j) * K] = b[j]; }
  };
  M.load(t0, A.consts + 1 * A.limbsn, A.limbsn);          // the domain's one
  M.load(t1, A.consts + 2 * A.limbsn, A.limbsn);
  put(0, t0, t1);
  put(1, x0, x1);
  // x^d = x^(d-1) * x
  for (int j = 0; j < L; ++j) { t0[j] = x0[j]; t1[j] = x1[j]; }
  for (int d = 2; d < entries; ++d) {
    P.mul(t0, t1, t0, t1, x0, x1);
    put(d, t0, t1);
  }
}

// digit `win` (bits [win * window, (win + 1) * window)) of a little-endian weight of `wwords` words
__device__ __forceinline__ u32 multiexp_digit(const u32* w, int wwords, int win, int window) {
  const int bit = win * window, wi = bit >> 5, off = bit & 31;
  const u64 lo = wi < wwords ? w[wi] : 0u;
  const u64 hi = wi + 1 < wwords ? w[wi + 1] : 0u;
  return (u32)((lo | (hi << 32)) >> off) & ((1u << window) - 1u);
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) multiexp_n2_kernel(MultiexpN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int S = M_t::S;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int lane = threadIdx.x;
  const int gw = lane / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const i64 r = raw < A.rows ? raw : A.rows - 1;    // surplus groups redo the last row and store nothing
  M_t M;
  u32* cp_lds = multiexp_n2_setup<K, L>(M, smem, gw, A);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  u32 acc0[L], acc1[L];
  M.load(acc0, A.consts + 1 * A.limbsn, A.limbsn);   // the domain's one
  M.load(acc1, A.consts + 2 * A.limbsn, A.limbsn);
  const i64 entry_words = (i64)2 * L * K;
  const i64 input_words = entry_words << A.window;
  const u32* tab = A.tables + p;
  const int* idx_row = A.index + r * A.terms;
  const u32* w_row = A.weights + r * A.terms * A.wwords;
  for (int win = A.nwin - 1; win >= 0; --win) {
    if (win != A.nwin - 1)
      for (int s = 0; s < A.window; ++s) P.sqr(acc0, acc1, acc0, acc1);
    for (int t = 0; t < A.terms; ++t) {
      int i = idx_row[t];
      i = i < 0 ? 0 : (i >= A.n_inputs ? (int)A.n_inputs - 1 : i);
      const u32 d = multiexp_digit(w_row + (i64)t * A.wwords, A.wwords, win, A.window);
      const u32* f = tab + (i64)i * input_words + (i64)d * entry_words;
      u32 f0[L], f1[L];
#pragma unroll
      for (int j = 0; j < L; ++j) { f0[j] = f[j * K]; f1[j] = f[(L + j) * K]; }
      P.mul(acc0, acc1, acc0, acc1, f0, f1);
    }
  }
  // the last product, by E = (1, 0): the N-adic digits of the residue (mx_powmod_n2.hpp)
  {
    u32 e0[L], e1[L];
    M.set_small(e0, 1u);
    M.set_small(e1, 0u);
    P.mul(acc0, acc1, acc0, acc1, e0, e1);
  }
  // ---- epilogue of powmod_n2_kernel: digits into [0, N), then z = Y0 + Y1 * N by a plain product
  {
    u64 t[L];
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = acc0[j];
    M.normalize_full(acc0, t);
    const u32 carry = M.cond_sub(acc0);
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = acc1[j];
    if (p == 0) t[0] += carry;
    M.normalize_full(acc1, t);
    M.cond_sub(acc1);
  }
  u32* wide = smem + gw * M_t::LDS_WORDS;
  u32 hi[L];
  __syncthreads();
  M.template mulx<M_t::F_INIT | M_t::F_PLAIN>(hi, acc1, M.n, acc1, M.n, acc0, nullptr, wide, A.nblk);
  {
    u64 t[L];
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = hi[j];
    M.normalize_full(hi, t);
  }
  const int it = A.nblk * L;
#pragma unroll
  for (int j = 0; j < L; ++j) wide[it + p * L + j] = hi[j];
  if (p == 0) { wide[it + S] = 0; wide[it + S + 1] = 0; wide[it + S + 2] = 0; wide[it + S + 3] = 0; }
  __syncthreads();
  const bool valid = raw < A.rows;
  u32* dst = A.out + r * A.limbs2;
  const int nl = it + S;
  for (int k = p; k < A.limbs2; k += K) {
    const int bit = 32 * k;
    const int g = bit / W, off = bit - g * W;
    u32 o = 0;
    if (g < nl) {
      u64 v = (u64)wide[g] >> off;
      v |= (u64)wide[g + 1] << (W - off);
      if (2 * W - off < 32) v |= (u64)wide[g + 2] << (2 * W - off);
      o = (u32)v;
    }
    if (valid) dst[k] = o;
  }
}

}  // namespace mx
