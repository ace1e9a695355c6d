// Shared-weight product modulo a SQUARE: one set of public weight rows applied at many positions.
//
//   out[j][b] = prod_t table(index[j][t], b) ^ weights[j][t]  mod N^2      for every weight row j and position b
//
// — the multi-exponentiation of mx_multiexp_n2.hpp with the weight rows SHARED by every position.  The table pass is
// multiexp_n2_table_kernel, unchanged, over n_local + n_shared inputs; only the main pass, shared_n2_kernel, is here.
// Two operators run it, and differ in the launch arguments alone:
//
//   table(i, b) = i * stride + origin[b]     i >= 0      (origin == nullptr: origin[b] = b)
//               = n_local + ~i               i <  0      shared table ~i = -1 - i (the bias inputs 1 + (b_j mod N) N),
//                                                        stored ONCE behind the others and read without the origin
//   out         = ((image * rows + row) * image_positions + within) * limbs2,
//                 image = b / image_positions, within = b % image_positions
//
// Encrypted matrix product over a batch of ciphertext vectors: the positions are the samples of a
// tile.  A table column c < n_cols has one table per sample, table number c * tile + b — the tables of one column are
// contiguous in b: stride = tile, no origin array, n_local = n_cols * tile, and image_positions = 1 makes out
// [tile][rows][limbs2], sample-major.
//
// Encrypted convolution of ciphertext grids with a public kernel: the tables are the pixels of the
// padded input grids, and a tap reads the pixel that lies at a fixed offset from the position's own corner: stride = 1,
// index is the table of the tap at output position 0 and origin[b] the position's offset (the image's included), so
// every pixel has ONE table however many windows cover it.  Stride, dilation, channels and padding are in the two
// integer arrays alone.  The positions of a launch are `images` runs of image_positions each; out is
// [image][row][position of the image]: with the kernels as rows and whole images per launch this is the public layout
// [b][o][y][x] as it stands.  The host checks max(index) + max(origin) < n_local before a launch.
//
// Index.  index[rows][terms] and weights[rows][terms][wwords] are per WEIGHT ROW, never per position.  All table
// addresses are 64-bit and clamped into the table set, as multiexp_n2_kernel clamps its inputs (for the convolution
// the second line of defence behind the host's check).
//
// Groups.  One group of K lanes per output (row j, position b); a block is one wavefront.  The positions of a row are
// padded to a multiple of 64 / K groups, so the groups of a wavefront are CONSECUTIVE POSITIONS OF ONE WEIGHT ROW: they
// read the same term's index and weight (scalar loads through the constant address space) and tables one stride
// apart — consecutive tables of one column for the matrix product.  Every group loads its origin once, before the
// window loop.  Surplus groups redo the last position and store nothing.
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

struct SharedN2Args {
  const u32* tables;    // [n_local + n_shared][1 << window][2][L][K] (workspace, written by the table pass)
  const u32* consts;    // [8][limbsn] the plan's constant rows of this geometry (MultiexpN2Args::consts)
  const int* index;     // [rows][terms]: >= 0 table of the term at origin 0, in strides; < 0 shared table ~index
  const u32* weights;   // [rows][terms][wwords] little-endian words of the non-negative weight
  const i64* origin;    // [positions] table offset of every position; nullptr: the position itself
  u32* out;             // [positions / image_positions][rows][image_positions][limbs2]
  i64 n_local, n_shared, rows;
  int stride;           // tables per unit of index
  int image_positions;  // positions of one image of this launch (divides positions)
  int positions;        // output positions of this launch
  int pos_blocks;       // wavefronts per weight row: ceil(positions / (64 / K))
  int terms, wwords, nwin, window;
  int limbsn, limbs2, nblk;
};

template <int K, int L, int W>
__global__ void __launch_bounds__(64, 3) shared_n2_kernel(SharedN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int lane = threadIdx.x;
  const int gw = lane / K;
  const i64 row = (i64)(blockIdx.x / (unsigned)A.pos_blocks);                  // wave-uniform: the weight row
  const int raw = (int)(blockIdx.x % (unsigned)A.pos_blocks) * GPW + gw;
  const bool valid = raw < A.positions;
  const int b = valid ? raw : A.positions - 1;      // surplus groups redo the last position and store nothing
  M_t M;
  u32* cp_lds = pair_setup<K, L>(M, smem, gw, A.consts, A.limbsn, A.nblk);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  u32 acc0[L], acc1[L];
  M.load(acc0, A.consts + 1 * A.limbsn, A.limbsn);   // the domain's one
  M.load(acc1, A.consts + 2 * A.limbsn, A.limbsn);
  const i64 entry_words = (i64)2 * L * K;
  const i64 table_words = entry_words << A.window;
  const i64 n_tables = A.n_local + A.n_shared;
  const u32* tab = A.tables + p;
  const i64 org = A.origin ? A.origin[b] : (i64)b;   // the position's offset: once per group
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
      i64 tn = i >= 0 ? (i64)i * A.stride + org : A.n_local + (i64)~i;
      tn = tn < 0 ? 0 : (tn >= n_tables ? n_tables - 1 : tn);
      const u32* f = tab + tn * table_words + (i64)d * entry_words;
      u32 f0[L], f1[L];
#pragma unroll
      for (int j = 0; j < L; ++j) { f0[j] = f[j * K]; f1[j] = f[(L + j) * K]; }
      P.mul(acc0, acc1, acc0, acc1, f0, f1);
    }
  }
  // image_positions divides positions <= 2^30: a 32-bit division, once per group
  const u32 image = (u32)b / (u32)A.image_positions, within = (u32)b - image * (u32)A.image_positions;
  u32* dst = A.out + (((i64)image * A.rows + row) * A.image_positions + within) * A.limbs2;
  pair_store<K, W>(M, P, acc0, acc1, smem + gw * M_t::LDS_WORDS, A.nblk, dst, A.limbs2, valid);
}

}  // namespace mx
