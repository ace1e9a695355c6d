// Encrypted matrix product modulo a SQUARE over a batch of ciphertext vectors:
//
//   out[b][j] = prod_t table(index[j][t], b) ^ weights[j][t]  mod N^2      for every weight row j and sample b < tile
//
// — the multi-exponentiation of mx_multiexp_n2.hpp with the weight rows SHARED by every sample.  The table pass is
// multiexp_n2_table_kernel, unchanged, over n_cols * tile + n_shared inputs; only the main pass is new.
//
// Tables.  A table column c < n_cols has one table per sample of the tile, table number c * tile + b: the tables of one
// column are contiguous in b.  The n_shared tables that do not depend on the sample (the bias inputs 1 + (b_j mod N) N)
// are stored ONCE, behind the per-sample ones, table number n_cols * tile + s.
//
// Index.  index[rows][terms] and weights[rows][terms][wwords] are per WEIGHT ROW, never per sample.  index >= 0 names a
// table column (read with the sample's offset), index < 0 names the shared table ~index = -1 - index (read without it).
// All table addresses are 64-bit and clamped into the table set, as multiexp_n2_kernel clamps its inputs.
//
// Groups.  One group of K lanes per output (row j, sample b); a block is one wavefront.  The samples of a row are padded
// to a multiple of 64 / K groups, so the groups of a wavefront are CONSECUTIVE SAMPLES OF ONE WEIGHT ROW: they read the
// same term's index and weight (scalar loads through the constant address space) and consecutive tables of one column.  Surplus groups
// redo the last sample and store nothing.
//
// Zero digits cost no multiplication.  Where the current digit is zero in every group of the wavefront, the multiplication by the
// domain's one is skipped.  The test is a wave-wide vote (__any over the 64 lanes), so all lanes take the same branch
// around P.mul's LDS staging and barriers whatever the arrangement of groups; with the arrangement above the digit is
// the same in every group of a wavefront, so the vote skips exactly the zero digits.  Skipping changes the pair-form
// representative of the accumulator, not its value: the epilogue gives the same canonical residue.
//
// THE WEIGHTS ARE PUBLIC PLAINTEXTS: here — unlike in the modexp kernels, whose exponents are secret shares — control
// flow may depend on them (§4.9 already lets the table address depend on them).  Nothing secret enters this kernel: its
// inputs are ciphertexts, public weights and public biases.
#pragma once
#include "mx_multiexp_n2.hpp"

namespace mx {

struct MatmulN2Args {
  const u32* tables;    // [n_cols * tile + n_shared][1 << window][2][L][K] (workspace, written by the table pass)
  const u32* consts;    // [8][limbsn] the plan's constant rows of this geometry (MultiexpN2Args::consts)
  const int* index;     // [rows][terms]: >= 0 table column, < 0 shared table ~index
  const u32* weights;   // [rows][terms][wwords] little-endian words of the non-negative weight
  u32* out;             // [tile][rows][limbs2], sample-major
  i64 n_cols, n_shared, rows;
  int tile;             // samples of this launch
  int tile_blocks;      // wavefronts per weight row: ceil(tile / (64 / K))
  int terms, wwords, nwin, window;
  int limbsn, limbs2, nblk;
};

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) matmul_n2_kernel(MatmulN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int S = M_t::S;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int lane = threadIdx.x;
  const int gw = lane / K;
  const i64 row = (i64)(blockIdx.x / (unsigned)A.tile_blocks);                 // wave-uniform: the weight row
  const int raw = (int)(blockIdx.x % (unsigned)A.tile_blocks) * GPW + gw;
  const bool valid = raw < A.tile;
  const int b = valid ? raw : A.tile - 1;           // surplus groups redo the last sample and store nothing
  M_t M;
  u32* cp_lds;
  {
    MultiexpN2Args sa{};                              // the set-up reads the constants, limbsn and nblk only
    sa.consts = A.consts;
    sa.limbsn = A.limbsn;
    sa.nblk = A.nblk;
    cp_lds = multiexp_n2_setup<K, L>(M, smem, gw, sa);
  }
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  u32 acc0[L], acc1[L];
  M.load(acc0, A.consts + 1 * A.limbsn, A.limbsn);   // the domain's one
  M.load(acc1, A.consts + 2 * A.limbsn, A.limbsn);
  const i64 entry_words = (i64)2 * L * K;
  const i64 table_words = entry_words << A.window;
  const i64 n_tables = A.n_cols * A.tile + A.n_shared;
  const u32* tab = A.tables + p;
  // index and weights are written by the host before the launch and only read here, at wave-uniform addresses: read
  // through the constant address space (scalar loads through the scalar cache, as the tape of mx_powmod_n2.hpp)
  typedef const __attribute__((address_space(4))) int* const_int_ptr_t;
  const const_int_ptr_t idx_row = (const_int_ptr_t)A.index + row * A.terms;
  const tape_ptr_t w_row = (tape_ptr_t)A.weights + row * A.terms * A.wwords;
  const u32 dmask = (1u << A.window) - 1u;
  for (int win = A.nwin - 1; win >= 0; --win) {
    if (win != A.nwin - 1)
      for (int s = 0; s < A.window; ++s) P.sqr(acc0, acc1, acc0, acc1);
    const int bit = win * A.window, wi = bit >> 5, off = bit & 31;
    for (int t = 0; t < A.terms; ++t) {
      // the term's index and its digit (multiexp_digit's arithmetic) are loaded together, before the vote
      const int i = idx_row[t];
      const tape_ptr_t w = w_row + (i64)t * A.wwords;
      const u64 lo = wi < A.wwords ? w[wi] : 0u;
      const u64 hi = wi + 1 < A.wwords ? w[wi + 1] : 0u;
      const u32 d = (u32)((lo | (hi << 32)) >> off) & dmask;
      if (!__any(d != 0u)) continue;                 // a zero digit in every group of the wavefront: acc * one = acc
      i64 tn = i >= 0 ? (i64)i * A.tile + b : A.n_cols * A.tile + (i64)~i;
      tn = tn < 0 ? 0 : (tn >= n_tables ? n_tables - 1 : tn);
      const u32* f = tab + tn * table_words + (i64)d * entry_words;
      u32 f0[L], f1[L];
#pragma unroll
      for (int j = 0; j < L; ++j) { f0[j] = f[j * K]; f1[j] = f[(L + j) * K]; }
      P.mul(acc0, acc1, acc0, acc1, f0, f1);
    }
  }
  // the last product, by E = (1, 0), and the epilogue of multiexp_n2_kernel: a canonical residue in [0, N^2)
  {
    u32 e0[L], e1[L];
    M.set_small(e0, 1u);
    M.set_small(e1, 0u);
    P.mul(acc0, acc1, acc0, acc1, e0, e1);
  }
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
  u32* dst = A.out + ((i64)b * A.rows + row) * A.limbs2;
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
