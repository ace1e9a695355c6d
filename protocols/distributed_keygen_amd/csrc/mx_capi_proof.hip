// mx_sha256_rows / mx_dleq_response: the Fiat-Shamir challenge and the response of the decryption proofs (mx_sha256.hpp,
// mx_response.hpp) behind the C ABI (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_sha256.hpp"
#include "mx_response.hpp"

extern "C" int mx_sha256_rows(const uint8_t prefix[32], const uint32_t* const* d_rows, const int* limbs, int n_sets,
                              int64_t count, uint32_t* d_out, void* stream) {
  if (!prefix || !d_out || n_sets < 0 || n_sets > mx::SHA_MAX_SETS || count < 0) return MX_ERR_ARG;
  if (n_sets > 0 && (!d_rows || !limbs)) return MX_ERR_ARG;
  int64_t words = 8;
  for (int s = 0; s < n_sets; ++s) {
    if (!d_rows[s] || limbs[s] < 1) return MX_ERR_ARG;
    words += limbs[s];
  }
  if (words > MX_SHA256_MAX_WORDS) return MX_ERR_SIZE;
  const int64_t nblocks = (count + mx::SHA_THREADS - 1) / mx::SHA_THREADS;
  if (nblocks > 0x7FFFFFFF) return MX_ERR_SIZE;
  if (count == 0) return MX_OK;
  mx::ShaRowsArgs a{};
  for (int k = 0; k < 8; ++k)
    a.prefix[k] = (uint32_t)prefix[4 * k] << 24 | (uint32_t)prefix[4 * k + 1] << 16 | (uint32_t)prefix[4 * k + 2] << 8 | prefix[4 * k + 3];
  for (int s = 0; s < n_sets; ++s) { a.rows[s] = d_rows[s]; a.limbs[s] = limbs[s]; }
  a.out = d_out;
  a.count = count;
  a.n_sets = n_sets;
  a.words = (int32_t)words;
  return mx_launch(mx::sha256_rows_kernel, nblocks, mx::SHA_THREADS, 0, (hipStream_t)stream, a);
}

extern "C" int mx_dleq_response(const uint32_t* d_rho, const uint32_t* d_e, const uint32_t* d_x, uint32_t* d_z,
                                uint8_t* d_status, int wz, int ew, int wx, int64_t count, void* stream) {
  return mx::run_response<false>(d_rho, d_e, d_x, d_z, d_status, wz, ew, wx, count, stream);
}
