// Fixed-base exponentiation modulo a SQUARE:  out[r] = f_r * g^(e_r)  mod N^2  for ONE base g and many exponents e_r,
// the randomiser of a Paillier encryption or re-randomisation when g = h_s is fixed per key.
//
//   table pass, two launches:
//     fixedbase_n2_chain_kernel  one group of lanes: converts g into pair form and walks the chain g^(2^(w i)),
//                                i < windows = ceil(exp_bits / w), by w pair squarings per step; writes entry 0 (the
//                                domain's one) and entry 1 of every window;
//     fixedbase_n2_fill_kernel   one group per (window i, digit d >= 2): T[i][d] = T[i][1]^d by a left-to-right binary
//                                ladder of w - 1 steps that every group runs in full (square, then multiply by T[i][1] or
//                                by one): 2 (w - 1) pair products whatever d is, so control flow is wave-uniform;
//   run pass (fixedbase_n2_run_kernel): one group of lanes per output.  acc = T[0][d_0], then one pair product by
//     T[i][d_i] for every further window — NO squaring — with d_i read from the exponent's words (bits at exp_bits and
//     above are masked, not trusted).  The entry of window i + 1 is requested before the product of window i runs.  Then
//     the factor of the mode, the product by E = (1, 0) and the epilogue (pair_store): canonical residues.
//       POWER      f_r = 1
//       ENCRYPT    f_r = 1 + m_r N, m_r < N.  In pair form value(X0, X1) = rho (X0 + X1 N), so (0, m) has the value
//                  rho m N and ONE PAIR PRODUCT by K1 (the value R) gives m N; adding the domain's one gives 1 + m N.
//                  A general residue needs the split at bits(N) - 1 and two products.
//       RANDOMIZE  f_r = c_r < N^2, any residue: the conversion of the multiexp and pack kernels, (x_lo, 0) K1 + (x_hi, 0) K2.
//     Control flow depends on (exp_bits, w, mode) only: every group of a wavefront runs the same windows, a digit 0
//     multiplies by the domain's one like any other digit; only the table ADDRESS depends on the exponent.
//
// Table layout (the entry layout of mx_multiexp_n2.hpp with one "input" per window): entry (i, d) is 2 K L contiguous
// words at ((i << w) + d) * 2 K L, word ((half * L + j) * K + p) for limb j of lane p — a group reads one contiguous,
// lane-consecutive span per product.
#pragma once
#include "mx_multiexp_n2.hpp"

namespace mx {

enum : int { FIXEDBASE_POWER = 0, FIXEDBASE_ENCRYPT = 1, FIXEDBASE_RANDOMIZE = 2 };

struct FixedBaseN2Args {
  const u32* base;      // [limbs2] (chain pass): any residue < N^2
  u32* table;           // [windows][1 << window][2][L][K]
  const u32* consts;    // [8][limbsn] the plan's constant rows of this geometry: N, ONE0, ONE1, K1_0, K1_1, K2_0, K2_1, C'
  const u32* exps;      // [count][ewords] little-endian words; bits at exp_bits and above are ignored
  const u32* operand;   // ENCRYPT: [count][oplimbs] messages < N; RANDOMIZE: [count][oplimbs] residues < N^2; POWER: unused
  u32* out;             // [count][limbs2]
  i64 count;
  int exp_bits, ewords, window, windows, mode, oplimbs;
  int limbsn, limbs2, nblk;
  int ksplit;           // x = x_lo + 2^ksplit * x_hi, ksplit = bits(N) - 1
};

template <int K, int L>
constexpr size_t fixedbase_n2_lds_bytes() { return powmod_n2_lds_bytes<K, L>(false); }

// One workgroup; every group of the wavefront walks the same chain and the first one stores.
template <int K, int L, int W>
__global__ void __launch_bounds__(64, 2) fixedbase_n2_chain_kernel(FixedBaseN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int WIDE = M_t::LDS_WORDS;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  M_t M;
  u32* cp_lds = pair_setup<K, L>(M, smem, gw, A.consts, A.limbsn, A.nblk);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  u32* wide = smem + gw * M_t::LDS_WORDS;
  __syncthreads();
  for (int k = p; k < WIDE; k += K) wide[k] = (k < A.limbs2) ? A.base[k] : 0u;
  __syncthreads();
  u32 x0[L], x1[L], t0[L], t1[L];
  pair_convert<W>(M, P, wide, A.consts, A.limbsn, A.ksplit, x0, x1);
  M.load(t0, A.consts + 1 * A.limbsn, A.limbsn);          // the domain's one
  M.load(t1, A.consts + 2 * A.limbsn, A.limbsn);
  const i64 entry_words = (i64)2 * L * K;
  const bool store = gw == 0;
  auto put = [&](int i, int d, const u32 (&a)[L], const u32 (&b)[L]) {
    if (!store) return;
    u32* dst = A.table + (((i64)i << A.window) + d) * entry_words + p;
#pragma unroll
    for (int j = 0; j < L; ++j) { dst[j * K] = a[j]; dst[(L + j) * K] = b[j]; }
  };
  for (int i = 0; i < A.windows; ++i) {
    if (i != 0)
      for (int s = 0; s < A.window; ++s) P.sqr(x0, x1, x0, x1);
    put(i, 0, t0, t1);
    put(i, 1, x0, x1);
  }
}

// One group per (window, digit >= 2); reads entry 1 of its window (written by the chain launch before it on the stream).
template <int K, int L, int W>
__global__ void __launch_bounds__(64, 2) fixedbase_n2_fill_kernel(FixedBaseN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  const int per = (1 << A.window) - 2;                    // digits 2 .. 2^w - 1 of every window (the host launches none for w = 1)
  const i64 total = (i64)A.windows * per;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const bool valid = raw < total;
  const i64 e = valid ? raw : total - 1;                  // surplus groups redo the last entry and store nothing
  const int i = (int)(e / per);
  const u32 d = 2u + (u32)(e - (i64)i * per);
  M_t M;
  u32* cp_lds = pair_setup<K, L>(M, smem, gw, A.consts, A.limbsn, A.nblk);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  const i64 entry_words = (i64)2 * L * K;
  u32* win = A.table + ((i64)i << A.window) * entry_words + p;
  u32 x0[L], x1[L], o0[L], o1[L], acc0[L], acc1[L];
#pragma unroll
  for (int j = 0; j < L; ++j) { x0[j] = win[entry_words + j * K]; x1[j] = win[entry_words + (L + j) * K]; }
  M.load(o0, A.consts + 1 * A.limbsn, A.limbsn);
  M.load(o1, A.consts + 2 * A.limbsn, A.limbsn);
  {
    const bool top = (d >> (A.window - 1)) & 1u;
#pragma unroll
    for (int j = 0; j < L; ++j) { acc0[j] = top ? x0[j] : o0[j]; acc1[j] = top ? x1[j] : o1[j]; }
  }
  for (int b = A.window - 2; b >= 0; --b) {
    P.sqr(acc0, acc1, acc0, acc1);
    const bool bit = (d >> b) & 1u;
    u32 f0[L], f1[L];
#pragma unroll
    for (int j = 0; j < L; ++j) { f0[j] = bit ? x0[j] : o0[j]; f1[j] = bit ? x1[j] : o1[j]; }
    P.mul(acc0, acc1, acc0, acc1, f0, f1);
  }
  if (valid) {
    u32* dst = win + (i64)d * entry_words;
#pragma unroll
    for (int j = 0; j < L; ++j) { dst[j * K] = acc0[j]; dst[(L + j) * K] = acc1[j]; }
  }
}

// digit `win` of an exponent row: bits [win * window, (win + 1) * window) below exp_bits
__device__ __forceinline__ u32 fixedbase_digit(const u32* e, int ewords, int exp_bits, int win, int window) {
  const int bit = win * window, wi = bit >> 5, off = bit & 31;
  const u64 lo = wi < ewords ? e[wi] : 0u;
  const u64 hi = wi + 1 < ewords ? e[wi + 1] : 0u;
  const int room = exp_bits - bit;                        // >= 1 for every window the kernels run
  const int nb = room < window ? room : window;
  return (u32)((lo | (hi << 32)) >> off) & ((1u << nb) - 1u);
}

// Two wavefronts per SIMD, as the pack kernel: the accumulator pair, the current entry and the requested one are live
// across a product.
template <int K, int L, int W>
__global__ void __launch_bounds__(64, 2) fixedbase_n2_run_kernel(FixedBaseN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  constexpr int WIDE = M_t::LDS_WORDS;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const i64 r = raw < A.count ? raw : A.count - 1;        // surplus groups redo the last output and store nothing
  M_t M;
  u32* cp_lds = pair_setup<K, L>(M, smem, gw, A.consts, A.limbsn, A.nblk);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  u32* wide = smem + gw * M_t::LDS_WORDS;
  const i64 entry_words = (i64)2 * L * K;
  const u32* tab = A.table + p;
  const u32* e_row = A.exps + r * A.ewords;
  auto entry = [&](int i) {
    return tab + (((i64)i << A.window) + fixedbase_digit(e_row, A.ewords, A.exp_bits, i, A.window)) * entry_words;
  };
  u32 acc0[L], acc1[L], f0[L], f1[L];
  {
    const u32* f = entry(0);
#pragma unroll
    for (int j = 0; j < L; ++j) { acc0[j] = f[j * K]; acc1[j] = f[(L + j) * K]; }
  }
  if (A.windows > 1) {
    const u32* f = entry(1);
#pragma unroll
    for (int j = 0; j < L; ++j) { f0[j] = f[j * K]; f1[j] = f[(L + j) * K]; }
  }
  for (int i = 1; i < A.windows; ++i) {
    u32 n0[L], n1[L];
    const u32* f = entry(i + 1 < A.windows ? i + 1 : i);  // the next entry travels while this product runs
#pragma unroll
    for (int j = 0; j < L; ++j) { n0[j] = f[j * K]; n1[j] = f[(L + j) * K]; }
    P.mul(acc0, acc1, acc0, acc1, f0, f1);
#pragma unroll
    for (int j = 0; j < L; ++j) { f0[j] = n0[j]; f1[j] = n1[j]; }
  }
  // ---- the factor of the mode
  if (A.mode != FIXEDBASE_POWER) {
    const bool enc = A.mode == FIXEDBASE_ENCRYPT;
    const u32* src = A.operand + r * A.oplimbs;
    __syncthreads();
    for (int k = p; k < WIDE; k += K) wide[k] = (k < A.oplimbs) ? src[k] : 0u;
    __syncthreads();
    // RANDOMIZE: the two halves of c = c_lo + 2^k c_hi; ENCRYPT: the whole message as one digit (no split) — the split
    // point, the digit that carries lo and the second term all depend on the mode, so this is not pair_convert
    const int ks = enc ? 32 * WIDE : A.ksplit;
    u32 lo[L], hi[L], zero[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const int bit = W * (p * L + j);
      const int room = ks - bit;
      lo[j] = room <= 0 ? 0u : extract_field(wide, bit, room < W ? room : W);
      const int hbit = ks + bit;
      hi[j] = (hbit + W + 32 <= 32 * WIDE) ? extract_field(wide, hbit, W) : 0u;
      zero[j] = 0u;
    }
    u32 u0[L], u1[L];
#pragma unroll
    for (int j = 0; j < L; ++j) { u0[j] = enc ? 0u : lo[j]; u1[j] = enc ? lo[j] : 0u; }
    // (c_lo, 0) * K1, or (0, m) * K1 = m N
    u32 x0[L], x1[L], t0[L], t1[L];
    M.load(t0, A.consts + 3 * A.limbsn, A.limbsn);
    M.load(t1, A.consts + 4 * A.limbsn, A.limbsn);
    P.mul(x0, x1, u0, u1, t0, t1);
    if (enc) {
      M.load(t0, A.consts + 1 * A.limbsn, A.limbsn);      // + the domain's one
      M.load(t1, A.consts + 2 * A.limbsn, A.limbsn);
    } else {
      M.load(t0, A.consts + 5 * A.limbsn, A.limbsn);      // + (c_hi, 0) * K2
      M.load(t1, A.consts + 6 * A.limbsn, A.limbsn);
      P.mul(t0, t1, hi, zero, t0, t1);
    }
    M.add(x0, x0, t0);
    M.add(x1, x1, t1);
    P.mul(acc0, acc1, acc0, acc1, x0, x1);
  }
  pair_store<K, W>(M, P, acc0, acc1, wide, A.nblk, A.out + r * A.limbs2, A.limbs2, raw < A.count);
}

}  // namespace mx
