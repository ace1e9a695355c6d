// mx_safe_sieve / mx_safe_double: the joint sieve of h and 2h + 1 and the rows 2h + 1 of the safe-prime search
// (mx_safe.hpp), behind the C ABI (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_safe.hpp"

namespace {

// the workspace of mx_sieve, region for region: primes | 2^(32 j) mod l | l^-1 mod 2^64 | floor((2^64 - 1) / l)
struct SafeSievePlan { int np_pad; int64_t off_primes, off_pw, off_inv, off_lim, total; };
SafeSievePlan plan_safe_sieve(int limbs, int np) {
  SafeSievePlan p;
  p.np_pad = (np + 63) / 64 * 64;
  int64_t o = 0;
  p.off_primes = o; o += align256((int64_t)np * 4);
  p.off_pw = o;     o += align256((int64_t)limbs * p.np_pad * 4);
  p.off_inv = o;    o += align256((int64_t)p.np_pad * 8);
  p.off_lim = o;    o += align256((int64_t)p.np_pad * 8);
  p.total = o;
  return p;
}

}  // namespace

extern "C" int64_t mx_safe_sieve_workspace_bytes(int limbs, int n_primes) {
  if (limbs < 1 || n_primes < 1) return MX_ERR_ARG;
  return plan_safe_sieve(limbs, n_primes).total;
}

extern "C" int mx_safe_sieve(const uint32_t* d_halves, uint8_t* d_out, const uint32_t* h_primes, int n_primes, int limbs,
                             int64_t batch, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!d_halves || !d_out || !h_primes || !d_ws || limbs < 1 || n_primes < 1 || batch < 0) return MX_ERR_ARG;
  uint32_t top = 3;
  for (int k = 0; k < n_primes; ++k) {
    if (!(h_primes[k] & 1u) || h_primes[k] < 3 || h_primes[k] >= (1u << 31)) return MX_ERR_ARG;
    if (h_primes[k] > top) top = h_primes[k];
  }
  if (limbs > 1024) return MX_ERR_SIZE;
  const int64_t nblocks = (batch + mx::SIEVE_C - 1) / mx::SIEVE_C;
  if (nblocks > 0x7FFFFFFF) return MX_ERR_SIZE;
  SafeSievePlan p = plan_safe_sieve(limbs, n_primes);
  if (p.total > ws_bytes) return MX_ERR_WORKSPACE;
  if (batch == 0) return MX_OK;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)d_ws;
  MX_TRY(upload_words(ws + p.off_primes, h_primes, (size_t)n_primes, s));
  mx::SieveArgs a;
  a.cands = d_halves; a.out = d_out;
  a.primes = (const u32*)(ws + p.off_primes);
  a.pw = (u32*)(ws + p.off_pw);
  a.inv = (u64*)(ws + p.off_inv);
  a.lim = (u64*)(ws + p.off_lim);
  a.batch = batch; a.limbs = limbs; a.np = n_primes; a.np_pad = p.np_pad;
  // limbs a 64-bit column takes between two folds (mx_sieve.hpp): 2^32 ((chunk + 1) top + 1) < 2^64
  const int64_t chunk = (int64_t)(0xFFFFFFFEull / top) - 1;          // >= 1 for top < 2^31
  a.chunk = (int)std::min<int64_t>(chunk, limbs);
  MX_TRY(mx_launch(mx::sieve_setup_kernel, p.np_pad / 64, 64, 0, s, a));
  return mx_launch(mx::safe_sieve_kernel, nblocks, 64, (size_t)limbs * mx::SIEVE_C * 4, s, a);
}

extern "C" int mx_safe_double(const uint32_t* d_in, uint32_t* d_out, int limbs, int64_t rows, void* stream) {
  if (!d_in || !d_out || d_in == d_out || limbs < 1 || rows < 0) return MX_ERR_ARG;
  if (rows > INT64_MAX / limbs || (rows * limbs + 255) / 256 > 0x7FFFFFFF) return MX_ERR_SIZE;
  if (rows == 0) return MX_OK;
  mx::SafeDoubleArgs a;
  a.in = d_in; a.out = d_out; a.words = rows * limbs; a.limbs = limbs;
  return mx_launch(mx::safe_double_kernel, (a.words + 255) / 256, 256, 0, (hipStream_t)stream, a);
}
