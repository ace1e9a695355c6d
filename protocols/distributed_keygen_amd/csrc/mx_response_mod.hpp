// The response of a Sigma-protocol whose exponent lives MODULO M, with the quotient the prover needs to correct its
// second response (multiplication.py; tools/mul_model.py is the model):
//
//   s = rho[r] + e[r] * x[r]   over the integers,   w[r] = s mod M,   t[r] = floor(s / M),   r < count      response_mod_kernel
//
// rho and x rows [count][wn], challenge rows e [count][ew], ONE modulus M of wn words whose top word is non-zero, w rows
// [count][wn] (canonical, below M), t rows [count][ew]; status[r] = 1 iff the quotient does not fit ew words — only when
// rho or x is not below M —, t[r] then holds its low ew words and w[r] is the correct residue all the same.
//
// One row per lane.  s < 2^(32 (wn + ew)) always, and its wn + ew words live in the row's OWN OUTPUT: word k in w[k] for
// k < wn and in t[k - wn] above.  Pass 1 forms them by columns as response_kernel does.  Then schoolbook division, digit
// i = ew .. 0: the window is the wn words s[i .. i + wn - 1] and the word above them (hi: s[i + wn], 0 for i = ew), below
// M 2^32 because what the digit before left is below M.  The digit's estimate
//
//   qh = floor(Uh nu / 2^64),   Uh = the top 64 bits of (window << shift),   nu = floor(2^96 / (Md + 1)),
//   Md = the top 64 bits of (M << shift),   shift = the leading zeros of M's top word          (nu and shift from the host)
//
// satisfies q - 2 <= qh <= q (tools/mul_model.py checks it exhaustively at 4-bit words).  The window takes
// three passes of the same code, "window -= f M, is the result >= M ?", with f = qh and then twice the answer of the pass
// before (0 or 1), which is added to the digit: two masked corrections, no branch on data.  The word s[i + wn] is dead
// once digit i is known and is exactly where the digit goes (t[i]; digit ew goes into the status).  What remains in w is
// the residue.
//
// Every loop bound, every branch and every address is a function of (wn, ew, count, r) only; carries and borrows are
// add-with-compare arithmetic; the estimate is one 64 x 64 -> high 64 product.  A fixed number of words lives in
// registers (the accumulator, hi, the digit, the three top words), no private segment, no LDS.  Plain C++, vector loads
// and stores only.  No output may alias an input or the other output.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mx_launch.hpp"

namespace mx {

constexpr int RESPONSE_MOD_THREADS = 256;

struct ResponseModArgs {
  const uint32_t* rho;      // [count][wn]
  const uint32_t* e;        // [count][ew]
  const uint32_t* x;        // [count][wn]
  const uint32_t* mod;      // [wn], top word non-zero
  uint32_t* w;              // [count][wn]
  uint32_t* t;              // [count][ew]
  uint8_t* status;          // [count]
  uint64_t recip;           // floor(2^96 / (Md + 1)), in [2^32, 2^33)
  int64_t count;
  int32_t wn, ew, shift;
};

// word k of the row's s: the low wn words in w, the ew above them in t
__device__ __forceinline__ uint32_t* response_mod_word(uint32_t* w, uint32_t* t, int wn, int k) {
  return k < wn ? w + k : t + (k - wn);
}

// window -= f * M over the wn words s[i ..] and hi above them; returns 1 iff the result is >= M, else 0
__device__ __forceinline__ uint32_t response_mod_mulsub(uint32_t* w, uint32_t* t, const uint32_t* mod, int wn, int i,
                                                        uint32_t f, uint32_t& hi) {
  uint64_t carry = 0;       // of f * M
  uint32_t borrow = 0;      // of window - f * M
  uint32_t below = 0;       // the borrow of (window - f * M) - M
  for (int j = 0; j < wn; ++j) {
    uint32_t* p = response_mod_word(w, t, wn, i + j);
    const uint32_t m = mod[j];
    const uint64_t prod = (uint64_t)f * m + carry;
    carry = prod >> 32;
    const uint64_t d = (uint64_t)*p - (uint32_t)prod - borrow;
    borrow = (uint32_t)(d >> 32) & 1u;
    *p = (uint32_t)d;
    const uint64_t c = (uint64_t)(uint32_t)d - m - below;
    below = (uint32_t)(c >> 32) & 1u;
  }
  hi = hi - (uint32_t)carry - borrow;
  return (uint32_t)(hi >= below);
}

__global__ __launch_bounds__(RESPONSE_MOD_THREADS) void response_mod_kernel(const ResponseModArgs a) {
  const int64_t r = (int64_t)blockIdx.x * RESPONSE_MOD_THREADS + threadIdx.x;
  if (r >= a.count) return;
  const int wn = a.wn, ew = a.ew;
  const uint32_t* rho = a.rho + r * wn;
  const uint32_t* e = a.e + r * ew;
  const uint32_t* x = a.x + r * wn;
  uint32_t* w = a.w + r * wn;
  uint32_t* t = a.t + r * ew;
  // pass 1: the wn + ew words of s = rho + e x by columns (the last carry is 0: s <= 2^(32 ew) (2^(32 wn) - 1))
  uint64_t lo = 0;          // the accumulator: lo + 2^64 hi2
  uint32_t hi2 = 0;
  for (int k = 0; k < wn + ew; ++k) {
    if (k < wn) {
      const uint64_t v = rho[k];
      lo += v;
      hi2 += lo < v;
    }
    const int j0 = k - (wn - 1) > 0 ? k - (wn - 1) : 0;      // 0 <= k - j < wn
    const int j1 = k < ew - 1 ? k : ew - 1;                  // j < ew
    for (int j = j0; j <= j1; ++j) {
      const uint64_t prod = (uint64_t)e[j] * x[k - j];
      lo += prod;
      hi2 += lo < prod;
    }
    *response_mod_word(w, t, wn, k) = (uint32_t)lo;
    lo = (lo >> 32) | ((uint64_t)hi2 << 32);
    hi2 = 0;
  }
  // the digits of the quotient, from the top
  uint32_t over = 0;
  for (int i = ew; i >= 0; --i) {
    uint32_t hi = i < ew ? t[i] : 0u;                         // s[i + wn]
    const uint32_t u1 = *response_mod_word(w, t, wn, i + wn - 1);
    const uint32_t u0 = wn >= 2 ? *response_mod_word(w, t, wn, i + wn - 2) : 0u;
    const uint64_t uh = ((((uint64_t)hi << 32) | u1) << a.shift) | (((uint64_t)u0 << a.shift) >> 32);
    uint32_t q = (uint32_t)__umul64hi(uh, a.recip);           // q - 2 <= estimate <= q < 2^32
    uint32_t ge = response_mod_mulsub(w, t, a.mod, wn, i, q, hi);
    q += ge;
    ge = response_mod_mulsub(w, t, a.mod, wn, i, ge, hi);
    q += ge;
    response_mod_mulsub(w, t, a.mod, wn, i, ge, hi);
    if (i < ew) t[i] = q;
    else over |= q;
  }
  a.status[r] = over ? 1 : 0;
}

// what mx_response_mod_rows is: the refusals, then one launch
inline int run_response_mod(const uint32_t* d_rho, const uint32_t* d_e, const uint32_t* d_x, const uint32_t* d_mod,
                            uint64_t recip, int shift, uint32_t* d_w, uint32_t* d_t, uint8_t* d_status, int wn, int ew,
                            int64_t count, void* stream) {
  if (!d_rho || !d_e || !d_x || !d_mod || !d_w || !d_t || !d_status || wn < 1 || ew < 1 || count < 0) return MX_ERR_ARG;
  if (shift < 0 || shift > 31 || (recip >> 32) != 1) return MX_ERR_ARG;
  if (wn > MX_DLEQ_MAX_WORDS || ew > MX_DLEQ_MAX_WORDS) return MX_ERR_SIZE;
  const int64_t nblocks = (count + RESPONSE_MOD_THREADS - 1) / RESPONSE_MOD_THREADS;
  if (nblocks > 0x7FFFFFFF) return MX_ERR_SIZE;
  if (count == 0) return MX_OK;
  ResponseModArgs a;
  a.rho = d_rho; a.e = d_e; a.x = d_x; a.mod = d_mod; a.w = d_w; a.t = d_t; a.status = d_status;
  a.recip = recip;
  a.count = count;
  a.wn = wn; a.ew = ew; a.shift = shift;
  return mx_launch(response_mod_kernel, nblocks, RESPONSE_MOD_THREADS, 0, (hipStream_t)stream, a);
}

}  // namespace mx
