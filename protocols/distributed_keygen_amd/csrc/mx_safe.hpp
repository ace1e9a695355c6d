// Safe-prime search, p = 2h + 1 with h and p prime: the joint sieve of h and 2h + 1, and the rows 2h + 1.
//
// safe_sieve_kernel: out[e] = 1 iff some prime l of the list has h ≡ 0 (l divides h) or h ≡ (l - 1) / 2 (l divides
// 2h + 1) modulo l.  The geometry, the tables and the 64-bit columns are those of sieve_kernel (mx_sieve_setup.hpp: SieveArgs,
// sieve_setup_kernel, SIEVE_C candidates per wavefront, lanes over primes, limbs transposed in LDS, a fold every `chunk`
// limbs), so limbs, table rows and MACs are read and issued once for the two conditions.  What is added per (candidate,
// block of 64 primes) comes after the loop: the column acc ≡ h is folded once more with the table's own w1 = 2^32 mod l,
//     x = lo32(acc) + hi32(acc) * w1  <=  (2^32 - 1) + (2^32 - 1)(l - 1)  <  2^32 l  <  2^63      for l < 2^31,
// so 2x + 1 < 2^64 is exact in a register, and the exact-division test of mx_sieve.hpp, v * l^-1 mod 2^64 <= floor((2^64
// - 1) / l), decides both v = x and v = 2x + 1; the second product is 2 (x l^-1) + l^-1, one shift and one add.
// Rows of one word have no table row 1 and need none: their column is the word itself, below 2^32.
//
// safe_double_kernel: out = 2 in + 1 over rows of 32-bit words, one thread per word; the bit that crosses a word
// boundary is the top bit of the word below.  A row whose top bit is set does not fit: the caller refuses it.
#pragma once
#include "mx_sieve_setup.hpp"

namespace mx {

__global__ void __launch_bounds__(64) safe_sieve_kernel(SieveArgs A) {
  extern __shared__ u32 smem[];   // [limbs][SIEVE_C]
  const int lane = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * SIEVE_C;
  // rows beyond the batch are zero (reported as hit, never stored)
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
    const u32 w1 = A.limbs > 1 ? A.pw[(long long)A.np_pad + k] : 0u;          // 2^32 mod l
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
      if (j1 < A.limbs) {          // more limbs to come: fold the columns
#pragma unroll
        for (int c = 0; c < SIEVE_C; ++c) acc[c] = (acc[c] & 0xFFFFFFFFull) + (acc[c] >> 32) * w1;
      }
    }
    const u64 inv = A.inv[k], lim = A.lim[k];
#pragma unroll
    for (int c = 0; c < SIEVE_C; ++c) {
      const u64 x = (acc[c] & 0xFFFFFFFFull) + (acc[c] >> 32) * w1;          // < 2^63: 2x + 1 does not wrap
      const u64 t = x * inv;                                                   // l | x      iff t <= lim
      const u64 t2 = (t << 1) + inv;                                           // l | 2x + 1 iff (2x + 1) l^-1 <= lim
      hit[c] |= (k < A.np && (t <= lim || t2 <= lim)) ? 1u : 0u;
    }
  }
#pragma unroll
  for (int c = 0; c < SIEVE_C; ++c) {
    bool any = __any(hit[c] != 0);
    if (lane == 0 && e0 + c < A.batch) A.out[e0 + c] = any ? 1 : 0;
  }
}

struct SafeDoubleArgs {
  const u32* in;       // [rows][limbs] device
  u32* out;            // [rows][limbs] device, not the rows of `in`
  long long words;     // rows * limbs
  int limbs;
};

__global__ void __launch_bounds__(256) safe_double_kernel(SafeDoubleArgs A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.words) return;
  const int j = (int)(i % A.limbs);
  const u32 w = A.in[i];
  const u32 below = j ? A.in[i - 1] >> 31 : 1u;      // the carry out of the word below; the + 1 at the bottom
  A.out[i] = (w << 1) | below;
}

}  // namespace mx
