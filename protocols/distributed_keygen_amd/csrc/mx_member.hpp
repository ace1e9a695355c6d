// The challenge arithmetic of the one-of-k membership proofs (membership.py; tools/member_model.py is the model;
// DESIGN.md §4.27): the Cramer-Damgard-Schoenmakers OR-composition splits one 128-bit challenge e over k branches, of
// which ONE — the real one, index[r] — is the prover's secret.  Rows of four little-endian words, sim and out
// [count][k][4], e [count][4], index [count], status [count]:
//
//   MEMBER_MASK   out[r][j] = (j == index[r]) ? 0 : sim[r][j]                                member_challenge_kernel<0>
//   MEMBER_SPLIT  out[r][index[r]] = e[r] - sum_(j != index[r]) sim[r][j]  mod 2^128,
//                 out[r][j] = sim[r][j] elsewhere                                            member_challenge_kernel<1>
//   MEMBER_SUM    status[r] = (sum_j sim[r][j] mod 2^128 != e[r])   (the verifier: no index is read)   <2>
//
// One row per lane.  Every loop bound, every branch and every address is a function of (k, count, r, j): the real slot
// is picked by an all-ones / all-zeros word made from the comparison j != index[r] and applied with AND / OR, every slot
// of every row is read and every slot is written, whichever is the real one.  The 128-bit sums and the difference are
// two 64-bit halves whose carry and borrow are add-with-compare arithmetic, no branch.  A lane reads slot j before it
// writes slot j and touches no other row, so out may be sim.  Plain C++, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mx_launch.hpp"

namespace mx {

constexpr int MEMBER_THREADS = 256;
constexpr int MEMBER_MASK = 0, MEMBER_SPLIT = 1, MEMBER_SUM = 2;
constexpr int MEMBER_MIN_K = 2, MEMBER_MAX_K = 16;

struct MemberArgs {
  const uint32_t* e;        // [count][4]            (split, sum)
  const uint32_t* sim;      // [count][k][4]
  const int32_t* index;     // [count]               (mask, split)
  uint32_t* out;            // [count][k][4]         (mask, split; it may be sim)
  uint8_t* status;          // [count]               (sum)
  int64_t count;
  int32_t k;
};

struct U128 {
  uint64_t lo, hi;
};

__device__ __forceinline__ U128 member_load(const uint32_t* p) {
  U128 v;
  v.lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);
  v.hi = (uint64_t)p[2] | ((uint64_t)p[3] << 32);
  return v;
}

__device__ __forceinline__ void member_store(uint32_t* p, const U128 v) {
  p[0] = (uint32_t)v.lo;
  p[1] = (uint32_t)(v.lo >> 32);
  p[2] = (uint32_t)v.hi;
  p[3] = (uint32_t)(v.hi >> 32);
}

template <int MODE>
__global__ __launch_bounds__(MEMBER_THREADS) void member_challenge_kernel(const MemberArgs a) {
  const int64_t r = (int64_t)blockIdx.x * MEMBER_THREADS + threadIdx.x;
  if (r >= a.count) return;
  const uint32_t* sim = a.sim + r * a.k * 4;
  if (MODE == MEMBER_SUM) {
    U128 sum = {0, 0};
    for (int j = 0; j < a.k; ++j) {
      const U128 v = member_load(sim + j * 4);
      sum.lo += v.lo;
      sum.hi += v.hi + (uint64_t)(sum.lo < v.lo);
    }
    const U128 e = member_load(a.e + r * 4);
    a.status[r] = (uint8_t)(((sum.lo ^ e.lo) | (sum.hi ^ e.hi)) != 0);
    return;
  }
  uint32_t* out = a.out + r * a.k * 4;
  const int32_t real = a.index[r];
  U128 own = {0, 0};          // what the real slot receives: 0 (mask), e - the sum of the others (split)
  if (MODE == MEMBER_SPLIT) {
    U128 sum = {0, 0};
    for (int j = 0; j < a.k; ++j) {
      const uint64_t keep = 0 - (uint64_t)(j != real);
      U128 v = member_load(sim + j * 4);
      v.lo &= keep;
      v.hi &= keep;
      sum.lo += v.lo;
      sum.hi += v.hi + (uint64_t)(sum.lo < v.lo);
    }
    const U128 e = member_load(a.e + r * 4);
    own.lo = e.lo - sum.lo;
    own.hi = e.hi - sum.hi - (uint64_t)(e.lo < sum.lo);
  }
  for (int j = 0; j < a.k; ++j) {
    const uint64_t keep = 0 - (uint64_t)(j != real);
    U128 v = member_load(sim + j * 4);
    v.lo = (v.lo & keep) | (own.lo & ~keep);
    v.hi = (v.hi & keep) | (own.hi & ~keep);
    member_store(out + j * 4, v);
  }
}

// what mx_member_challenges is: the refusals, then one launch
inline int run_member_challenges(const uint32_t* d_e, const uint32_t* d_sim, const int32_t* d_index, uint32_t* d_out,
                                 uint8_t* d_status, int k, int64_t count, int mode, void* stream) {
  if (mode != MEMBER_MASK && mode != MEMBER_SPLIT && mode != MEMBER_SUM) return MX_ERR_ARG;
  if (!d_sim || k < MEMBER_MIN_K || k > MEMBER_MAX_K || count < 0) return MX_ERR_ARG;
  if (mode != MEMBER_MASK && !d_e) return MX_ERR_ARG;
  if (mode == MEMBER_SUM ? !d_status : (!d_index || !d_out)) return MX_ERR_ARG;
  const int64_t nblocks = (count + MEMBER_THREADS - 1) / MEMBER_THREADS;
  if (nblocks > 0x7FFFFFFF) return MX_ERR_SIZE;
  if (count == 0) return MX_OK;
  MemberArgs a;
  a.e = d_e; a.sim = d_sim; a.index = d_index; a.out = d_out; a.status = d_status;
  a.count = count;
  a.k = k;
  hipStream_t s = (hipStream_t)stream;
  if (mode == MEMBER_MASK) return mx_launch(member_challenge_kernel<MEMBER_MASK>, nblocks, MEMBER_THREADS, 0, s, a);
  if (mode == MEMBER_SPLIT) return mx_launch(member_challenge_kernel<MEMBER_SPLIT>, nblocks, MEMBER_THREADS, 0, s, a);
  return mx_launch(member_challenge_kernel<MEMBER_SUM>, nblocks, MEMBER_THREADS, 0, s, a);
}

}  // namespace mx
