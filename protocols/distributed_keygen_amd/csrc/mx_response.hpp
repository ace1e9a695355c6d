// The responses of the proofs, in their two forms:
//
//   z[r] = rho[r] + e[r] * x      over the integers,   r < count      response_kernel<false>, mx_dleq_response
//   z[r] = rho[r] + e[r] * x[r]                                        response_kernel<true>,  mx_response_rows
//
// rho rows [count][wz], challenge rows e [count][ew], z rows [count][wz]; status[r] = 1 iff the sum does not fit wz words
// (z[r] then holds its low wz words), else 0.  The decryption proofs (threshold.py; tools/proof_model.py is the model;
// DESIGN.md §4.25) have ONE secret row x [wx] resident on the device for the whole batch, and the host sizes wz so that
// the status stays 0; the range proofs (range_proof.py; tools/range_model.py) have secret rows
// x [count][wx], ONE PER PROOF.
//
// One row per lane.  Column k of the result is rho_k + sum_j e_j x_(k-j) + the carry of column k - 1: plain 32 x 32 -> 64
// multiply-adds into a 96-bit accumulator (64 + 32 bits: up to 2^31 products of a column fit).  The columns at wz and above
// (they exist when wx + ew > wz) and the last carry are ORed into the status instead of being stored.  Every loop bound
// and every branch is a function of (wz, ew, wx, count); the words of rho and e are read at addresses that depend on the
// row number only, and so are those of a per-row x, while the words of the shared x are read at wave-uniform addresses
// (PER_ROW is a compile-time flag, not a stride, so that they stay there): control flow and addresses are independent of
// x, rho and e.  The carries are add-with-compare arithmetic, no branch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mx_launch.hpp"

namespace mx {

constexpr int RESPONSE_THREADS = 256;

struct ResponseArgs {
  const uint32_t* rho;      // [count][wz]
  const uint32_t* e;        // [count][ew]
  const uint32_t* x;        // PER_ROW ? [count][wx] : [wx]
  uint32_t* z;              // [count][wz]
  uint8_t* status;          // [count]
  int64_t count;
  int32_t wz, ew, wx;
};

template <bool PER_ROW>
__global__ __launch_bounds__(RESPONSE_THREADS) void response_kernel(const ResponseArgs a) {
  const int64_t r = (int64_t)blockIdx.x * RESPONSE_THREADS + threadIdx.x;
  if (r >= a.count) return;
  const uint32_t* rho = a.rho + r * a.wz;
  const uint32_t* e = a.e + r * a.ew;
  const uint32_t* x = PER_ROW ? a.x + r * a.wx : a.x;
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

// what mx_dleq_response (PER_ROW = false) and mx_response_rows (true) are
template <bool PER_ROW>
int run_response(const uint32_t* d_rho, const uint32_t* d_e, const uint32_t* d_x, uint32_t* d_z, uint8_t* d_status,
                 int wz, int ew, int wx, int64_t count, void* stream) {
  if (!d_rho || !d_e || !d_x || !d_z || !d_status || wz < 1 || ew < 1 || wx < 1 || count < 0) return MX_ERR_ARG;
  if (wz > MX_DLEQ_MAX_WORDS || ew > MX_DLEQ_MAX_WORDS || wx > MX_DLEQ_MAX_WORDS) return MX_ERR_SIZE;
  const int64_t nblocks = (count + RESPONSE_THREADS - 1) / RESPONSE_THREADS;
  if (nblocks > 0x7FFFFFFF) return MX_ERR_SIZE;
  if (count == 0) return MX_OK;
  ResponseArgs a;
  a.rho = d_rho; a.e = d_e; a.x = d_x; a.z = d_z; a.status = d_status;
  a.count = count;
  a.wz = wz; a.ew = ew; a.wx = wx;
  return mx_launch(response_kernel<PER_ROW>, nblocks, RESPONSE_THREADS, 0, (hipStream_t)stream, a);
}

}  // namespace mx
