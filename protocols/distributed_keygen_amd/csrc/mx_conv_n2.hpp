// Encrypted convolution modulo a SQUARE: a grid of ciphertexts under a public kernel:
//
//   out[j][b] = prod_t table(index[j][t], b) ^ weights[j][t]  mod N^2      for every weight row j and position b
//
// — the shared-weight product of mx_matmul_n2.hpp with another ADDRESS RULE.  There a table column holds one table per
// sample (index * tile + b); here the tables are the pixels of the padded input grids, and a tap reads the pixel that
// lies at a fixed offset from the position's own corner:
//
//   table(i, b) = i + origin[b]          i >= 0: the table of the tap at output position 0
//               = n_local + ~i           i <  0: shared table ~i = -1 - i (the bias inputs), read without the origin
//
// so every pixel has ONE table however many windows cover it.  The table pass is multiexp_n2_table_kernel, unchanged,
// over n_local + n_shared inputs; only the main pass is new.  Stride, dilation, channels and padding are in the two
// integer arrays alone: index[rows][terms] (per weight row) and origin[positions] (per position, the image's offset
// included).  The host checks max(index) + max(origin) < n_local before a launch; the 64-bit clamp into the table set
// below is the second line of defence, as in multiexp_n2_kernel.
//
// Groups.  One group of K lanes per output (row j, position b); a block is one wavefront.  The positions of a row are
// padded to a multiple of 64 / K groups, so the groups of a wavefront are CONSECUTIVE POSITIONS OF ONE WEIGHT ROW: they
// read the same term's index and weight (scalar loads through the constant address space) and tables one stride apart.
// Every group loads its origin once, before the window loop.  Surplus groups redo the last position and store nothing.
//
// Output.  The positions of a launch are `images` runs of image_positions each; out is [image][row][position of the
// image]: with the kernels as rows and whole images per launch this is the public layout [b][o][y][x] as it stands.
//
// Zero digits cost no multiplication (the wave-wide vote of mx_matmul_n2.hpp).  THE WEIGHTS ARE PUBLIC PLAINTEXTS:
// control flow depends on them.  Nothing secret enters this kernel.
#pragma once
#include "mx_multiexp_n2.hpp"

namespace mx {

struct ConvN2Args {
  const u32* tables;    // [n_local + n_shared][1 << window][2][L][K] (workspace, written by the table pass)
  const u32* consts;    // [8][limbsn] the plan's constant rows of this geometry (MultiexpN2Args::consts)
  const int* index;     // [rows][terms]: >= 0 table of the tap at position 0, < 0 shared table ~index
  const u32* weights;   // [rows][terms][wwords] little-endian words of the non-negative weight
  const i64* origin;    // [positions] table offset of every position
  u32* out;             // [positions / image_positions][rows][image_positions][limbs2]
  i64 n_local, n_shared, rows;
  i64 image_positions;  // positions of one image of this launch (divides positions)
  int positions;        // output positions of this launch
  int pos_blocks;       // wavefronts per weight row: ceil(positions / (64 / K))
  int terms, wwords, nwin, window;
  int limbsn, limbs2, nblk;
};

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) conv_n2_kernel(ConvN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int S = M_t::S;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int lane = threadIdx.x;
  const int gw = lane / K;
  const i64 row = (i64)(blockIdx.x / (unsigned)A.pos_blocks);                  // wave-uniform: the weight row
  const int raw = (int)(blockIdx.x % (unsigned)A.pos_blocks) * GPW + gw;
  const bool valid = raw < A.positions;
  const int b = valid ? raw : A.positions - 1;      // surplus groups redo the last position and store nothing
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
  const i64 n_tables = A.n_local + A.n_shared;
  const u32* tab = A.tables + p;
  const i64 org = A.origin[b];                       // the position's offset: once per group
  // index and weights are written by the host before the launch and only read here, at wave-uniform addresses: read
  // through the constant address space (scalar loads through the scalar cache, as in matmul_n2_kernel)
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
      i64 tn = i >= 0 ? (i64)i + org : A.n_local + (i64)~i;
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
  const i64 image = (i64)b / A.image_positions, within = (i64)b - image * A.image_positions;
  u32* dst = A.out + ((image * A.rows + row) * A.image_positions + within) * A.limbs2;
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
