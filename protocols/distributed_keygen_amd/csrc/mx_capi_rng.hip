// mx_chacha20_rows: the device random-row generator (mx_chacha.hpp) behind the C ABI (translation unit of its own, built
// in parallel with the others).
#include "mx_launch.hpp"
#include "mx_chacha.hpp"

extern "C" int mx_chacha20_rows(const uint32_t key[8], const uint32_t nonce[3], uint32_t counter0, uint32_t* d_out,
                                int64_t count, int row_words, int bits, void* stream) {
  if (!key || !nonce || !d_out) return MX_ERR_ARG;
  if (count < 0 || bits < 1 || row_words < 1 || (int64_t)bits > 32 * (int64_t)row_words) return MX_ERR_ARG;
  const int64_t w = ((int64_t)bits + 31) / 32;
  if (count > (((int64_t)1 << 36) / w)) return MX_ERR_ARG;                  // more words than 2^32 blocks hold
  const int64_t blocks = (count * w + 15) / 16;
  if ((int64_t)counter0 + blocks > ((int64_t)1 << 32)) return MX_ERR_ARG;   // the 32-bit block counter would wrap
  if (count == 0) return MX_OK;
  mx::ChaChaArgs a;
  for (int k = 0; k < 8; ++k) a.key[k] = key[k];
  for (int k = 0; k < 3; ++k) a.nonce[k] = nonce[k];
  a.counter0 = counter0;
  a.out = d_out;
  a.count = count;
  a.row_words = row_words;
  a.bits = bits;
  const int64_t groups = (blocks + mx::CHACHA_THREADS - 1) / mx::CHACHA_THREADS;      // <= 2^24
  return mx_launch(mx::chacha20_rows_kernel, groups, mx::CHACHA_THREADS, 0, (hipStream_t)stream, a);
}
