// What the two forms of the sieve share beside the kernel itself (mx_sieve.hpp: sieve_kernel<JOINT>, run_sieve<JOINT>): the
// argument block, the number of candidates per wavefront, the kernel that fills the per-prime tables of the workspace,
// and on the host the layout of that workspace and the check of the list of primes.
#pragma once
#include "mx_lanes.hpp"
#include "mx_upload.hpp"

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

// the workspace, region for region: primes | 2^(32 j) mod l | l^-1 mod 2^64 | floor((2^64 - 1) / l)
struct SievePlan { int np_pad; int64_t off_primes, off_pw, off_inv, off_lim, total; };
SievePlan plan_sieve(int limbs, int np) {
  SievePlan p;
  p.np_pad = (np + 63) / 64 * 64;
  int64_t o = 0;
  p.off_primes = o; o += align256((int64_t)np * 4);
  p.off_pw = o;     o += align256((int64_t)limbs * p.np_pad * 4);
  p.off_inv = o;    o += align256((int64_t)p.np_pad * 8);
  p.off_lim = o;    o += align256((int64_t)p.np_pad * 8);
  p.total = o;
  return p;
}

// every listed prime odd and in [3, 2^31); top = the largest of them
bool sieve_primes_ok(const u32* h_primes, int n_primes, u32& top) {
  top = 3;
  for (int k = 0; k < n_primes; ++k) {
    if (!(h_primes[k] & 1u) || h_primes[k] < 3 || h_primes[k] >= (1u << 31)) return false;
    if (h_primes[k] > top) top = h_primes[k];
  }
  return true;
}

int64_t sieve_blocks(int64_t batch) { return (batch + SIEVE_C - 1) / SIEVE_C; }
}  // namespace

}  // namespace mx
