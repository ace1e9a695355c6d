// Safe-prime search, p = 2h + 1 with h and p prime: the rows 2h + 1.  The joint sieve of h and 2h + 1 is the JOINT form of
// sieve_kernel (mx_sieve.hpp).
//
// safe_double_kernel: out = 2 in + 1 over rows of 32-bit words, one thread per word; the bit that crosses a word
// boundary is the top bit of the word below.  A row whose top bit is set does not fit: the caller refuses it.
#pragma once
#include "mx_lanes.hpp"

namespace mx {

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
