// The response of the decryption proofs (threshold.py; tools/proof_model.py is the model):
//
//   z[r] = rho[r] + e[r] * x   over the integers,   r < count
//
// rho rows [count][wz], challenge rows e [count][ew], ONE secret row x [wx] resident on the device, z rows [count][wz];
// status[r] = 1 iff the sum does not fit wz words (z[r] then holds its low wz words), else 0.  The host sizes wz so that
// it never happens.
//
// One row per lane.  Column k of the result is rho_k + sum_j e_j x_(k-j) + the carry of column k - 1: plain 32 x 32 -> 64
// multiply-adds into a 96-bit accumulator (64 + 32 bits: up to 2^31 products of a column fit).  The columns at wz and above
// (they exist when wx + ew > wz) and the last carry are ORed into the status instead of being stored.  Every loop bound
// and every branch is a function of (wz, ew, wx, count); the words of x are read at wave-uniform addresses, those of
// rho and e at addresses that depend on the row number only: control flow and addresses are independent of x, rho and e.
// The carries are add-with-compare arithmetic, no branch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mx {

constexpr int DLEQ_THREADS = 256;

struct DleqResponseArgs {
  const uint32_t* rho;      // [count][wz]
  const uint32_t* e;        // [count][ew]
  const uint32_t* x;        // [wx]
  uint32_t* z;              // [count][wz]
  uint8_t* status;          // [count]
  int64_t count;
  int32_t wz, ew, wx;
};

__global__ __launch_bounds__(DLEQ_THREADS) void dleq_response_kernel(const DleqResponseArgs a) {
  const int64_t r = (int64_t)blockIdx.x * DLEQ_THREADS + threadIdx.x;
  if (r >= a.count) return;
  const uint32_t* rho = a.rho + r * a.wz;
  const uint32_t* e = a.e + r * a.ew;
  uint32_t* z = a.z + r * a.wz;
  const int cols = a.wx + a.ew > a.wz ? a.wx + a.ew : a.wz;      // the columns of rho + e x
  uint64_t lo = 0;          // the accumulator: lo + 2^64 hi
  uint32_t hi = 0;
  uint32_t over = 0;
  for (int k = 0; k < cols; ++k) {
    if (k < a.wz) {
      const uint64_t v = rho[k];
      lo += v;
      hi += lo < v;
    }
    const int j0 = k - (a.wx - 1) > 0 ? k - (a.wx - 1) : 0;      // 0 <= k - j < wx
    const int j1 = k < a.ew - 1 ? k : a.ew - 1;                  // j < ew
    for (int j = j0; j <= j1; ++j) {
      const uint64_t prod = (uint64_t)e[j] * a.x[k - j];
      lo += prod;
      hi += lo < prod;
    }
    if (k < a.wz) z[k] = (uint32_t)lo;
    else over |= (uint32_t)lo;
    lo = (lo >> 32) | ((uint64_t)hi << 32);
    hi = 0;
  }
  over |= (uint32_t)lo | (uint32_t)(lo >> 32);
  a.status[r] = over ? 1 : 0;
}

}  // namespace mx
