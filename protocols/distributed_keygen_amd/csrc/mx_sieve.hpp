// Small-prime sieve: out[e] = 1 iff some prime of the list divides candidate e.
// Replaces __small_prime_divisors_test (distributed_keygen.py:1197-1209) applied to every
// candidate modulus of a batch (distributed_keygen.py:1288-1292).
//
// N mod l is evaluated as  sum_j N_j * (2^(32j) mod l)  — one v_mad_u64_u32 per (limb, prime),
// no division in the loop — and divisibility of that 64-bit sum by the odd prime l is decided
// by the exact-division test  (x * l^-1 mod 2^64) <= floor((2^64-1)/l).
// The 64-bit column holds `chunk` products (each < 2^32 l) on top of a folded value: after every `chunk` limbs
// the column is folded with the table's own 2^32 mod l:  x <- lo32(x) + hi32(x) * (2^32 mod l)  < 2^32 (l + 1),
// which leaves the residue unchanged.  The host sets chunk = floor((2^32 - 2) / max prime) - 1, so that
// 2^32 ((chunk + 1) l + 1) < 2^64: no fold at all for lists below 2^21 (the reference's default threshold is 2000),
// one every 63 limbs at 2^26, one per limb only above 2^30.  Primes < 2^31.
// One wavefront handles SIEVE_C candidates: lanes run over primes (coalesced table reads), the
// candidates' limbs are staged transposed in LDS so that one ds_read_b128 feeds four MACs.
//
// JOINT, the sieve of the safe-prime search (p = 2h + 1 with h and p prime) over rows h: out[e] = 1 iff some prime l of
// the list has h ≡ 0 (l divides h) or h ≡ (l - 1) / 2 (l divides 2h + 1) modulo l.  Limbs, table rows and MACs are read
// and issued once for the two conditions.  What is added per (candidate, block of 64 primes) comes after the loop: the
// column acc ≡ h is folded once more with the table's own w1 = 2^32 mod l,
//     x = lo32(acc) + hi32(acc) * w1  <=  (2^32 - 1) + (2^32 - 1)(l - 1)  <  2^32 l  <  2^63      for l < 2^31,
// so 2x + 1 < 2^64 is exact in a register, and the exact-division test decides both v = x and v = 2x + 1; the second
// product is 2 (x l^-1) + l^-1, one shift and one add.  Rows of one word have no table row 1 and need none: their
// column is the word itself, below 2^32.  The plain form reads row 1 inside its fold only, which one-word rows never reach.
#pragma once
#include "mx_sieve_setup.hpp"

namespace mx {

template <bool JOINT>
__global__ void __launch_bounds__(64) sieve_kernel(SieveArgs A) {
  extern __shared__ u32 smem[];   // [limbs][SIEVE_C]
  const int lane = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * SIEVE_C;
  // stage candidates transposed; rows beyond the batch are zero (zero is reported divisible,
  // but such rows are never stored)
  for (int idx = lane; idx < A.limbs * SIEVE_C; idx += 64) {
    int c = idx / A.limbs, j = idx - c * A.limbs;   // consecutive lanes read consecutive words
    long long e = e0 + c;
    smem[j * SIEVE_C + c] = (e < A.batch) ? A.cands[e * A.limbs + j] : 0u;
  }
  __syncthreads();
  unsigned hit[SIEVE_C];
#pragma unroll
  for (int c = 0; c < SIEVE_C; ++c) hit[c] = 0;
  for (int k0 = 0; k0 < A.np_pad; k0 += 64) {
    const int k = k0 + lane;
    u32 w1 = 0u;          // 2^32 mod l
    if constexpr (JOINT) w1 = A.limbs > 1 ? A.pw[(long long)A.np_pad + k] : 0u;
    u64 acc[SIEVE_C];
#pragma unroll
    for (int c = 0; c < SIEVE_C; ++c) acc[c] = 0;
    for (int j0 = 0; j0 < A.limbs; j0 += A.chunk) {
      const int j1 = j0 + A.chunk < A.limbs ? j0 + A.chunk : A.limbs;
      for (int j = j0; j < j1; ++j) {
        u32 w = A.pw[(long long)j * A.np_pad + k];
        const uint4 lo = *reinterpret_cast<const uint4*>(&smem[j * SIEVE_C]);
        const uint4 hi = *reinterpret_cast<const uint4*>(&smem[j * SIEVE_C + 4]);
        acc[0] += (u64)lo.x * w; acc[1] += (u64)lo.y * w; acc[2] += (u64)lo.z * w; acc[3] += (u64)lo.w * w;
        acc[4] += (u64)hi.x * w; acc[5] += (u64)hi.y * w; acc[6] += (u64)hi.z * w; acc[7] += (u64)hi.w * w;
      }
      if (j1 < A.limbs) {          // more limbs to come: fold the columns (limbs >= 2 here, so row 1 of the table exists)
        if constexpr (!JOINT) w1 = A.pw[(long long)A.np_pad + k];
#pragma unroll
        for (int c = 0; c < SIEVE_C; ++c) acc[c] = (acc[c] & 0xFFFFFFFFull) + (acc[c] >> 32) * w1;
      }
    }
    const u64 inv = A.inv[k], lim = A.lim[k];
#pragma unroll
    for (int c = 0; c < SIEVE_C; ++c) {
      if constexpr (JOINT) {
        const u64 x = (acc[c] & 0xFFFFFFFFull) + (acc[c] >> 32) * w1;          // < 2^63: 2x + 1 does not wrap
        const u64 t = x * inv;                                                   // l | x      iff t <= lim
        const u64 t2 = (t << 1) + inv;                                           // l | 2x + 1 iff (2x + 1) l^-1 <= lim
        hit[c] |= (k < A.np && (t <= lim || t2 <= lim)) ? 1u : 0u;
      } else {
        hit[c] |= (k < A.np && acc[c] * inv <= lim) ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < SIEVE_C; ++c) {
    bool any = __any(hit[c] != 0);
    if (lane == 0 && e0 + c < A.batch) A.out[e0 + c] = any ? 1 : 0;
  }
}

// What mx_sieve (JOINT = false) and mx_safe_sieve (true) run once their own checks have passed: the primes into the
// workspace, the argument block, the tables of the list (sieve_setup_kernel) and the sieve.
template <bool JOINT>
int run_sieve(const u32* d_rows, unsigned char* d_out, const u32* h_primes, int n_primes, u32 top, int limbs,
              int64_t batch, const SievePlan& p, void* d_ws, hipStream_t s) {
  char* ws = (char*)d_ws;
  MX_TRY(upload_words(ws + p.off_primes, h_primes, (size_t)n_primes, s));
  SieveArgs a;
  a.cands = d_rows; a.out = d_out;
  a.primes = (const u32*)(ws + p.off_primes);
  a.pw = (u32*)(ws + p.off_pw);
  a.inv = (u64*)(ws + p.off_inv);
  a.lim = (u64*)(ws + p.off_lim);
  a.batch = batch; a.limbs = limbs; a.np = n_primes; a.np_pad = p.np_pad;
  // limbs a 64-bit column takes between two folds: 2^32 ((chunk + 1) top + 1) < 2^64
  const int64_t chunk = (int64_t)(0xFFFFFFFEull / top) - 1;          // >= 1 for top < 2^31
  a.chunk = (int)std::min<int64_t>(chunk, limbs);
  MX_TRY(mx_launch(sieve_setup_kernel, p.np_pad / 64, 64, 0, s, a));
  return mx_launch(sieve_kernel<JOINT>, sieve_blocks(batch), 64, (size_t)limbs * SIEVE_C * 4, s, a);
}

}  // namespace mx
