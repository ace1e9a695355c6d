// The strong-pseudoprime (Miller-Rabin) test, batched over S odd candidates n_c >= 3 — one MODULUS PER GROUP of G rows, as
// in mx_generators.hpp; candidates of different bit lengths share a launch.  With n_c - 1 = 2^s d, d odd:
//
//   mr_split_kernel   d as rows, s as int32: the trailing zero bits of n_c - 1 counted, the rest shifted down across the
//                     32-bit words (no arithmetic modulo anything)
//   mr_tail_kernel    the witness loop of a round to ANY base b: from x0 = b^d mod n_c (the generic modexp's output) the
//                     round passes iff b == 0 (vacuous), x0 == 1, x0 == n_c - 1, or x0^(2^i) == n_c - 1 for an i in [1, s)
//   mr_base2_kernel   the whole round to the base 2 from the candidate alone: left to right over the bits of n_c - 1, one
//                     squaring per bit and a doubling selected by the bit; the trailing s zero bits ARE the witness loop
//
// Everything is compared in the Montgomery domain: R mod n_c (the form of 1, by doubling as in mx_setup.hpp) and
// n_c - R mod n_c (the form of -1) are canonical, and a lazy value is made canonical by one carry sweep and one
// conditional subtraction before it is compared.
//
// Uniformity.  The loops run over wave-wide ranges: mr_tail_kernel squares max(s) - 1 times, the largest s among the
// elements of its wavefront, and an element past its own s keeps squaring without touching its flag; mr_base2_kernel runs
// one step per bit of the WIDEST candidate the launch was sized for, a shorter candidate squares the form of 1 until its
// top bit arrives, and the comparisons run in the last max(s) steps of the wavefront only.  The doubling is a select, not
// a branch; the bit of a step is read from an LDS copy of the candidate at an address the step number alone decides.  No
// table, no tape, no private segment; plain vector stores through Mont::store.
#pragma once
#include "mx_mont.hpp"
#include "mx_split.hpp"

namespace mx {

struct MrSplitArgs {
  const u32* cands;   // [groups][limbs]
  u32* d;             // [groups][limbs] (out)
  int* s;             // [groups] (out)
  long long groups;
  int limbs, nblk;
};

struct MrArgs {
  const u32* cands;      // [groups][limbs]
  const u32* x0;         // [batch][limbs]: b^d mod n_c, canonical (tail)
  const u32* bases;      // [batch][limbs]: b, canonical (tail)
  const int* s;          // [groups] (tail)
  unsigned char* pass;   // [batch] (out)
  long long batch;       // groups * group_size
  long long group_size;
  int limbs, nblk, mod_bits;
};

// the largest v among the 64 lanes, as a scalar
__device__ __forceinline__ int mr_wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return __builtin_amdgcn_readfirstlane(v);
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64) mr_split_kernel(MrSplitArgs A) {
  using M_t = Mont<K, L, W, true>;
  extern __shared__ u32 smem[];
  constexpr int GPW = 64 / K;
  const int gw = threadIdx.x / K;
  const long long g_raw = (long long)blockIdx.x * GPW + gw;
  const bool valid = g_raw < A.groups;
  const long long g = valid ? g_raw : A.groups - 1;
  M_t M;
  M.init(smem + gw * M_t::LDS_WORDS, A.nblk);
  M.stage_words(A.cands + g * A.limbs, A.limbs);
  if (M.p == 0) M.lds[0] &= ~1u;                       // n - 1 of an odd n
  M_t::sync();
  const int staged = A.limbs < M_t::LDS_WORDS ? A.limbs : M_t::LDS_WORDS;
  int tz = 32 * staged;                                // the lowest set bit of n - 1 (none: n == 1, refused by the host)
  for (int k = M.p; k < staged; k += K) {
    const u32 w = M.lds[k];
    const int here = w ? 32 * k + __builtin_ctz(w) : 32 * staged;
    tz = min(tz, here);
  }
#pragma unroll
  for (int off = K / 2; off > 0; off >>= 1) tz = min(tz, __shfl_xor(tz, off));      // stays inside the group
  tz = tz < 32 * staged ? tz : 0;
  u32 d[L];
  limbs_of_bits(M, d, tz, 32 * M_t::LDS_WORDS);        // up to the end of the scratch: zero beyond the candidate
  M.store(A.d + g * A.limbs, A.limbs, d, valid);
  if (valid && M.p == 0) A.s[g] = tz;
}

// What the two test kernels share: the row's candidate as the modulus, the forms of 1 and -1, the comparison.
template <int K, int L, int W>
struct MrRow {
  using M_t = Mont<K, L, W, true>;
  M_t M;
  u32 one_m[L], minus_m[L];      // R mod n and n - R mod n, canonical
  long long elem, cand;
  bool valid;
  __device__ __forceinline__ void init(const MrArgs& A, u32* smem) {
    constexpr int GPW = 64 / K;
    const int gw = threadIdx.x / K;
    const long long elem_raw = (long long)blockIdx.x * GPW + gw;
    valid = elem_raw < A.batch;
    elem = valid ? elem_raw : A.batch - 1;
    cand = elem / A.group_size;
    M.init(smem + gw * M_t::LDS_WORDS, A.nblk);
    M.load(M.n, A.cands + cand * A.limbs, A.limbs);
    M.setup_modulus();
    M.rmodn_by_doubling(one_m);
    u64 t[L];
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = (u64)M.n[j] + (u64)(M_t::MASK - one_m[j]);
    if (M.p == 0) t[0] += 1;
    M.normalize_full(minus_m, t);                      // n + (2^(W S) - R mod n); the carry out of the top limb is dropped
  }
  // lazy x < (NSUB + 1) n in the domain -> its canonical residue
  template <int NSUB>
  __device__ __forceinline__ void canonical(u32 (&c)[L], const u32 (&x)[L]) {
    u64 t[L];
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = x[j];
    M.normalize_full(c, t);
#pragma unroll
    for (int k = 0; k < NSUB; ++k) M.cond_sub(c);
  }
};

template <int K, int L, int W>
__global__ void __launch_bounds__(64) mr_tail_kernel(MrArgs A) {
  extern __shared__ u32 smem[];
  MrRow<K, L, W> Row;
  Row.init(A, smem);
  auto& M = Row.M;
  int s = A.s[Row.cand];
  s = s < 1 ? 1 : (s > A.mod_bits ? A.mod_bits : s);   // whatever the rows hold, the loop is as long as the shapes allow
  const int smax = mr_wave_max(s);
  u32 x[L], b[L], c[L];
  M.load(b, A.bases + Row.elem * A.limbs, A.limbs);
  bool pass = M.is_zero(b) || M.equal(b, M.n);         // a base that is 0 modulo n tests nothing
  M.load(x, A.x0 + Row.elem * A.limbs, A.limbs);
  M.set_small(c, 1);
  pass = pass || M.equal(x, c);
#pragma unroll
  for (int j = 0; j < L; ++j) c[j] = M.n[j];
  if (M.p == 0) c[0] &= ~1u;
  pass = pass || M.equal(x, c);
  u32 r2[L];
  M.compute_r2(r2, Row.one_m);
  M.mul(x, x, r2);                                     // into the domain
  for (int i = 1; i < smax; ++i) {
    M.sqr(x, x);
    Row.template canonical<1>(c, x);                   // a product is below 2 n
    const bool hit = M.equal(c, Row.minus_m);
    pass = pass || (hit && i < s);
  }
  if (Row.valid && M.p == 0) A.pass[Row.elem] = pass ? 1 : 0;
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64) mr_base2_kernel(MrArgs A) {
  using M_t = Mont<K, L, W, true>;
  extern __shared__ u32 smem[];
  MrRow<K, L, W> Row;
  Row.init(A, smem);                                   // group_size is 1: one row per candidate
  auto& M = Row.M;
  // the candidate's radix-2^32 words where every lane of the group reads the bit of a step: the scratch of the SECOND
  // multiplier, which one-row products never touch (mx_mont.hpp: LDS_D)
  constexpr int ROOM = M_t::LDS_WORDS - M_t::LDS_D;
  const int nw = A.limbs < ROOM ? A.limbs : ROOM;
  const u32* src = A.cands + Row.cand * A.limbs;
  M_t::sync();
  for (int k = M.p; k < ROOM; k += K) M.lds[M_t::LDS_D + k] = k < nw ? src[k] : 0u;
  M_t::sync();
  int tz = 32 * nw;                                    // s: the lowest set bit of n - 1
  for (int k = M.p; k < nw; k += K) {
    const u32 w = M.lds[M_t::LDS_D + k] & (k == 0 ? ~1u : ~0u);
    const int here = w ? 32 * k + __builtin_ctz(w) : 32 * nw;
    tz = min(tz, here);
  }
#pragma unroll
  for (int off = K / 2; off > 0; off >>= 1) tz = min(tz, __shfl_xor(tz, off));
  const int s = tz < A.mod_bits ? tz : A.mod_bits;
  const int smax = mr_wave_max(s);
  u32 x[L], c[L];
#pragma unroll
  for (int j = 0; j < L; ++j) x[j] = Row.one_m[j];
  bool pass = false;
  for (int i = A.mod_bits - 1; i >= 1; --i) {          // bit 0 of n - 1 is 0 and 2^(n-1) itself is never looked at
    const u32 bit = (M.lds[M_t::LDS_D + (i >> 5)] >> (i & 31)) & 1u;
    const u32 mask = 0u - bit;
    M.sqr(x, x);
    u32 y[L];
#pragma unroll
    for (int j = 0; j < L; ++j) y[j] = x[j] & mask;
    M.add(x, x, y);                                    // x or 2 x: below 4 n, which the next squaring takes
    if (i <= smax) {                                   // the same for the whole wavefront
      Row.template canonical<3>(c, x);
      const bool minus = M.equal(c, Row.minus_m), plus = M.equal(c, Row.one_m);
      pass = pass || (minus && i <= s) || (plus && i == s);
    }
  }
  if (Row.valid && M.p == 0) A.pass[Row.elem] = pass ? 1 : 0;
}

}  // namespace mx
