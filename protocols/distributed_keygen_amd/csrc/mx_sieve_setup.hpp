// What the sieves share (mx_sieve.hpp: sieve_kernel; mx_safe.hpp: safe_sieve_kernel): the argument block, the number of
// candidates per wavefront and the kernel that fills the per-prime tables of the workspace.
#pragma once
#include "mx_lanes.hpp"

namespace mx {

constexpr int SIEVE_C = 8;   // candidates per wavefront

struct SieveArgs {
  const u32* cands;    // [batch][limbs] device
  unsigned char* out;  // [batch] device
  const u32* primes;   // [np] device
  u32* pw;             // [limbs][np_pad] device: 2^(32 j) mod prime_k
  u64* inv;            // [np_pad] device: prime^-1 mod 2^64
  u64* lim;            // [np_pad] device: floor((2^64-1)/prime)
  long long batch;
  int limbs;
  int np;
  int np_pad;          // multiple of 64
  int chunk;           // limbs between two folds of the 64-bit columns (>= limbs: never)
};

namespace {      // a copy per translation unit (mx_capi.hip, mx_capi_safe.hip), as upload_kernel
// one thread per prime: powers of 2^32, inverse and limit
__global__ void sieve_setup_kernel(SieveArgs A) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= A.np_pad) return;
  if (k >= A.np) {   // padding lanes (masked out in the main kernel)
    for (int j = 0; j < A.limbs; ++j) A.pw[(long long)j * A.np_pad + k] = 0;
    A.inv[k] = 1; A.lim[k] = 0;
    return;
  }
  u64 l = A.primes[k];
  u64 r = 1 % l;
  for (int j = 0; j < A.limbs; ++j) {
    A.pw[(long long)j * A.np_pad + k] = (u32)r;
    r = (r << 32) % l;
  }
  u64 x = l;                       // Newton inverse mod 2^64 (l odd): 3 -> 6 -> ... -> 96 bits
  for (int i = 0; i < 5; ++i) x *= 2 - l * x;
  A.inv[k] = x;
  A.lim[k] = ~0ull / l;
}
}  // namespace

}  // namespace mx
