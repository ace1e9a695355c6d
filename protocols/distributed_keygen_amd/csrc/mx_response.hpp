// The responses of the range proofs (range_proof.py; tools/range_model.py is the model):
//
//   z[r] = rho[r] + e[r] * x[r]   over the integers,   r < count
//
// rho rows [count][wz], challenge rows e [count][ew], secret rows x [count][wx] — ONE PER PROOF, where the response of
// the decryption proofs (mx_proof.hpp: dleq_response_kernel, which stays as it is) has one secret for the whole batch —
// z rows [count][wz]; status[r] = 1 iff the sum does not fit wz words (z[r] then holds its low wz words), else 0.
//
// One row per lane, the column accumulator of dleq_response_kernel: column k of the result is rho_k + sum_j e_j x_(k-j)
// + the carry of column k - 1, plain 32 x 32 -> 64 multiply-adds into a 96-bit accumulator.  The columns at wz and
// above and the last carry are ORed into the status instead of being stored.  Every loop bound and every branch is a
// function of (wz, ew, wx, count); the words of rho, e and x are read at addresses that depend on the row number only:
// control flow and addresses are independent of x, rho and e.  The carries are add-with-compare arithmetic, no branch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mx {

constexpr int RESPONSE_THREADS = 256;

struct ResponseRowsArgs {
  const uint32_t* rho;      // [count][wz]
  const uint32_t* e;        // [count][ew]
  const uint32_t* x;        // [count][wx]
  uint32_t* z;              // [count][wz]
  uint8_t* status;          // [count]
  int64_t count;
  int32_t wz, ew, wx;
};

__global__ __launch_bounds__(RESPONSE_THREADS) void response_rows_kernel(const ResponseRowsArgs a) {
  const int64_t r = (int64_t)blockIdx.x * RESPONSE_THREADS + threadIdx.x;
  if (r >= a.count) return;
  const uint32_t* rho = a.rho + r * a.wz;
  const uint32_t* e = a.e + r * a.ew;
  const uint32_t* x = a.x + r * a.wx;
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
      const uint64_t prod = (uint64_t)e[j] * x[k - j];
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
