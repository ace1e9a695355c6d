// Private-key (CRT) Paillier decryption around the two half-size modexps, batched over ciphertexts (Paillier 1999, §7):
//
//   crt_split_kernel       c  ->  c mod p^2, c mod q^2          (what the pair kernel raises to p - 1 and q - 1)
//   crt_recombine_kernel   x_p, x_q  ->  m_p = L_p(x_p) h_p mod p,  m_q = L_q(x_q) h_q mod q,  L_r(x) = (x - 1) / r
//                                        m = m_p + p ((m_q - m_p) p^-1 mod q),  status bit 0: x_p != 1 mod p, bit 1: x_q != 1 mod q
//
// tools/crt_model.py is the model of both at the level of these products, with every operand bound asserted.
//
// The split reduces a row of limbs2 words — ANY value below 2^(32 limbs2) — the way mx_generators.hpp reduces a wide
// draw: the row is cut at s = 16 limbs2 into lo and hi, both below Rs / 16 for the radix Rs >= 2^(s + 4) of the launch, and
//   h = mont(hi, 2^s Rs mod P) = hi 2^s, < 2 P;   t = lo + h < Rs;   c mod P = mont(mont(t, Rs^2 mod P), 1), one subtraction
// — mont(a, b) < 2 P for ANY a < Rs when b < P.  Three products per prime square, no division.  One radix, from the longer
// prime, serves both squares.
//
// The recombination divides x - 1 by the prime exactly through a quotient-recording Montgomery reduction, as mx_combine.hpp
// divides by N: REDC gives r = (y + Q p) / R1 with r in {0, p} iff p | y, and then y / p = (R1 - Q) mod R1.  R1 >= 16 max(p, q)
// is one radix again: m_p < p is then a Montgomery operand modulo q whatever the order and the lengths of the primes.  The
// last step m_p + p t is a plain product (F_PLAIN) started from m_p, written out through the group's wide LDS row like the
// epilogue of mx_powmod_n2.hpp; it is below N because m_p < p and t <= q - 1.
//
// Everything that depends on the key comes from the host with the plan (mx_crt_prepare).  One group of K lanes per
// ciphertext; control flow and every address depend on the sizes only; no private segment; plain vector stores.
#pragma once
#include "mx_mont.hpp"
#include "mx_prio.hpp"
#include "mx_split.hpp"

namespace mx {

// rows of the plan, each `rw` words (the width of a half)
constexpr int CRT_ROW_SPLIT = 0;      // per prime square P: P | 2^s Rs mod P | Rs^2 mod P
constexpr int CRT_ROW_P = 6;          // p | h_p R1 mod p
constexpr int CRT_ROW_Q = 8;          // q | h_q R1 mod q | R1 mod q | p^-1 R1 mod q
constexpr int CRT_ROWS = 12;

struct CrtSplitArgs {
  const u32* cts;      // [batch][limbs2]
  u32* out;            // [2][batch][rw]
  const u32* plan;     // [CRT_ROWS][rw]
  long long batch;
  int limbs2, rw, nblk, split_bit;
};

struct CrtRecombineArgs {
  const u32* xp;       // [batch][rw]: x_p below p^2
  const u32* xq;       // [batch][rw]: x_q below q^2
  u32* out;            // [batch][out_stride]: limbs words of m, then (if the row is wider) one status word and zeros
  unsigned char* status;   // [batch], or null
  const u32* plan;
  long long batch;
  int limbs, rw, out_stride, nblk1;
};

// lazy x (< 2 N) -> the canonical residue, exact limbs
template <int K, int L, int W>
__device__ __forceinline__ void crt_canonical(Mont<K, L, W, true>& M, u32 (&x)[L]) {
  u64 t[L];
#pragma unroll
  for (int j = 0; j < L; ++j) t[j] = x[j];
  M.normalize_full(x, t);
  M.cond_sub(x);
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64) crt_split_kernel(CrtSplitArgs A) {
  aux_wave_priority();
  using M_t = Mont<K, L, W, true>;
  extern __shared__ u32 smem[];
  constexpr int GPW = 64 / K;
  const int gw = threadIdx.x / K;
  const long long elem_raw = (long long)blockIdx.x * GPW + gw;
  const bool valid = elem_raw < A.batch;
  const long long elem = valid ? elem_raw : A.batch - 1;
  M_t M;
  M.init(smem + gw * M_t::LDS_WORDS, A.nblk);
  M.stage_words(A.cts + elem * A.limbs2, A.limbs2);
  u32 lo[L], hi[L];
  limbs_of_bits(M, lo, 0, A.split_bit);
  limbs_of_bits(M, hi, A.split_bit, 32 * M_t::LDS_WORDS);      // up to the end of the row: the scratch is zero beyond it
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const u32* rows = A.plan + (size_t)(CRT_ROW_SPLIT + 3 * half) * A.rw;
    M.load(M.n, rows, A.rw);                     // (its first barrier is behind every lane's reads of the row)
    M.setup_modulus();
    u32 k[L], t[L];
    M.load(k, rows + A.rw, A.rw);
    M.mul(t, hi, k);                             // hi 2^s, < 2 P
    M.add(t, lo, t);                             // = c modulo P, < Rs
    M.load(k, rows + 2 * A.rw, A.rw);
    M.mul(t, t, k);                              // c Rs, < 2 P
    M.set_small(k, 1);
    M.mul(t, t, k);
    crt_canonical(M, t);
    M.store(A.out + ((long long)half * A.batch + elem) * A.rw, A.rw, t, valid);
  }
}

// L_r(x) h_r modulo the prime r that M holds, lazy (< 2 r); false when r does not divide x - 1
template <int K, int L, int W>
__device__ __forceinline__ bool crt_l_times_h(Mont<K, L, W, true>& M, u32 (&m)[L], const u32* x_row, const u32* h_row, int rw) {
  using M_t = Mont<K, L, W, true>;
  u32 x[L], y[L];
  M.load(x, x_row, rw);
  const bool x_zero = M.is_zero(x);
  {
    // y = x - 1 (for x >= 1): add 2^(W*S) - 1, drop the carry
    u64 t[L];
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = (u64)x[j] + M_t::MASK;
    M.normalize_full(y, t);
  }
  u32 one[L], q[L], r[L];
  M.set_small(one, 1);
  M.template mul<true>(r, y, one, q);            // r = (y + Q r) / R1, lazy
  {
    u64 t[L];
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = r[j];
    M.normalize_full(r, t);
  }
  const bool r_zero = M.is_zero(r);
  const bool r_is_n = M.equal(r, M.n);
  // u = (R1 - Q) mod R1 (limbs below nblk * L), or 0 when r == 0
  u32 u[L];
  {
    u64 t[L];
    const bool in_range = M.p < M.nblk;
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = (in_range && r_is_n) ? (u64)(M_t::MASK - q[j]) : 0;
    if (M.p == 0 && r_is_n) t[0] += 1;
    M.normalize_full(u, t);
    if (!in_range) {
#pragma unroll
      for (int j = 0; j < L; ++j) u[j] = 0;
    }
  }
  u32 h[L];
  M.load(h, h_row, rw);
  M.mul(m, u, h);
  return (r_zero || r_is_n) && !x_zero;
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64) crt_recombine_kernel(CrtRecombineArgs A) {
  aux_wave_priority();
  using M_t = Mont<K, L, W, true>;
  constexpr int S = K * L;
  constexpr int WIDE_WORDS = 2 * S + 8;          // nblk1 * L low limbs, S high limbs, 4 words of zeros
  extern __shared__ u32 smem[];
  constexpr int GPW = 64 / K;
  const int gw = threadIdx.x / K;
  const long long elem_raw = (long long)blockIdx.x * GPW + gw;
  const bool valid = elem_raw < A.batch;
  const long long elem = valid ? elem_raw : A.batch - 1;
  u32* wide = smem + GPW * M_t::LDS_WORDS + gw * WIDE_WORDS;
  M_t M;
  M.init(smem + gw * M_t::LDS_WORDS, A.nblk1);

  // ---- modulo p: m_p canonical, it is a summand of the result
  const u32* rows_p = A.plan + (size_t)CRT_ROW_P * A.rw;
  M.load(M.n, rows_p, A.rw);
  M.setup_modulus();
  u32 mp[L];
  const bool ok_p = crt_l_times_h(M, mp, A.xp + elem * A.rw, rows_p + A.rw, A.rw);
  crt_canonical(M, mp);

  // ---- modulo q: m_q stays lazy, then Garner's t = (m_q - m_p) p^-1 mod q
  const u32* rows_q = A.plan + (size_t)CRT_ROW_Q * A.rw;
  M.load(M.n, rows_q, A.rw);
  M.setup_modulus();
  u32 t[L];
  const bool ok_q = crt_l_times_h(M, t, A.xq + elem * A.rw, rows_q + A.rw, A.rw);
  {
    u32 k[L], a[L];
    M.load(k, rows_q + 2 * A.rw, A.rw);
    M.mul(a, mp, k);                             // m_p modulo q, < 2 q (m_p < p <= R1 / 16)
    u64 c[L];
#pragma unroll
    for (int j = 0; j < L; ++j) c[j] = a[j];
    M.normalize_full(a, c);
    // d = m_q + 2 q - a in (0, 4 q): the complement of a's exact limbs plus one, the carry out of the top dropped
#pragma unroll
    for (int j = 0; j < L; ++j) c[j] = (u64)t[j] + 2 * (u64)M.n[j] + (u64)(M_t::MASK - a[j]);
    if (M.p == 0) c[0] += 1;
    M.normalize_full(t, c);
    M.load(k, rows_q + 3 * A.rw, A.rw);
    M.mul(t, t, k);
    crt_canonical(M, t);
  }

  // ---- m = m_p + p t by a plain product: the low limbs leave through `wide`, the high part stays in the lanes
  const bool ok = ok_p && ok_q;
  u32 pl[L], hi[L];
  M.load(pl, rows_p, A.rw);
  M.template mulx<M_t::F_INIT | M_t::F_PLAIN>(hi, t, pl, t, pl, mp, nullptr, wide, A.nblk1);
  {
    u64 c[L];
#pragma unroll
    for (int j = 0; j < L; ++j) c[j] = hi[j];
    M.normalize_full(hi, c);
  }
  const int it = A.nblk1 * L;
#pragma unroll
  for (int j = 0; j < L; ++j) wide[it + M.p * L + j] = hi[j];
  if (M.p == 0) { wide[it + S] = 0; wide[it + S + 1] = 0; wide[it + S + 2] = 0; wide[it + S + 3] = 0; }
  __syncthreads();
  u32* dst = A.out + elem * A.out_stride;
  const int nl = it + S;
  for (int k = M.p; k < A.limbs; k += K) {
    const int bit = 32 * k;
    const int g = bit / W, off = bit - g * W;
    u32 o = 0;
    if (g < nl) {
      u64 v = (u64)wide[g] >> off;
      v |= (u64)wide[g + 1] << (W - off);
      if (2 * W - off < 32) v |= (u64)wide[g + 2] << (2 * W - off);
      o = (u32)v;
    }
    if (valid) dst[k] = ok ? o : 0u;
  }
  if (valid && M.p == 0) {
    const u32 st = (ok_p ? 0u : 1u) | (ok_q ? 0u : 2u);
    if (A.status) A.status[elem] = (unsigned char)st;
    for (int k = A.limbs; k < A.out_stride; ++k) dst[k] = (k == A.limbs) ? st : 0u;
  }
}

}  // namespace mx
