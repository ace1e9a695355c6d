// mx_safe_sieve / mx_safe_double: the joint sieve of h and 2h + 1 and the rows 2h + 1 of the safe-prime search
// (mx_sieve.hpp: sieve_kernel<true>; mx_safe.hpp), behind the C ABI (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_sieve.hpp"
#include "mx_safe.hpp"

extern "C" int64_t mx_safe_sieve_workspace_bytes(int limbs, int n_primes) {
  if (limbs < 1 || n_primes < 1) return MX_ERR_ARG;
  return mx::plan_sieve(limbs, n_primes).total;
}

extern "C" int mx_safe_sieve(const uint32_t* d_halves, uint8_t* d_out, const uint32_t* h_primes, int n_primes, int limbs,
                             int64_t batch, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!d_halves || !d_out || !h_primes || !d_ws || limbs < 1 || n_primes < 1 || batch < 0) return MX_ERR_ARG;
  uint32_t top;
  if (!mx::sieve_primes_ok(h_primes, n_primes, top)) return MX_ERR_ARG;
  if (limbs > 1024) return MX_ERR_SIZE;
  if (mx::sieve_blocks(batch) > 0x7FFFFFFF) return MX_ERR_SIZE;
  const mx::SievePlan p = mx::plan_sieve(limbs, n_primes);
  if (p.total > ws_bytes) return MX_ERR_WORKSPACE;
  if (batch == 0) return MX_OK;
  return mx::run_sieve<true>(d_halves, d_out, h_primes, n_primes, top, limbs, batch, p, d_ws, (hipStream_t)stream);
}

extern "C" int mx_safe_double(const uint32_t* d_in, uint32_t* d_out, int limbs, int64_t rows, void* stream) {
  if (!d_in || !d_out || d_in == d_out || limbs < 1 || rows < 0) return MX_ERR_ARG;
  if (rows > INT64_MAX / limbs || (rows * limbs + 255) / 256 > 0x7FFFFFFF) return MX_ERR_SIZE;
  if (rows == 0) return MX_OK;
  mx::SafeDoubleArgs a;
  a.in = d_in; a.out = d_out; a.words = rows * limbs; a.limbs = limbs;
  return mx_launch(mx::safe_double_kernel, (a.words + 255) / 256, 256, 0, (hipStream_t)stream, a);
}
