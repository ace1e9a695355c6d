// Random rows on the device: the ChaCha20 keystream of RFC 8439 written as rows of little-endian 32-bit words — the
// exponent rows of the fixed-base kernels (mx_fixedbase_n2.hpp) and the bases r of r^N (mx_powmod_n2.hpp) without a
// host draw and an upload.  tools/chacha_model.py is the bit-exact model; DESIGN.md §4.12.
//
// State: four constants, eight key words, a 32-bit block counter in word 12, a 96-bit nonce in words 13-15; twenty
// rounds, then the feed-forward addition; output words in state order.
//
// Mapping (the contract, the same for every launch shape), w = ceil(bits / 32):
//   keystream word i = r * w + j  ->  d_out[r][j], j < w;  it is word i mod 16 of block counter0 + i div 16
//   the top word of a row is masked to bits mod 32 bits when that is not 0
//   words w .. row_words - 1 of a row are written as 0
//   the unused tail of the last block is discarded
//
// One lane per 64-byte block; the sixteen state words are named scalars, the rounds unrolled: registers only.  A lane's
// block is 64 contiguous bytes of the stream, so stores straight from the lanes would put the 64 lanes of one store
// instruction 64 bytes apart.  The workgroup's 256 blocks go through LDS instead (rows of 17 words: an odd stride,
// so a wavefront's writes fall into 64 different banks) and come back word-major: one store instruction of a wavefront then writes 64 consecutive keystream words,
// 256 contiguous bytes wherever a row does not end.  Control flow depends on (count, row_words, bits) only; key and
// nonce arrive by value in the kernel-argument block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mx {

struct ChaChaArgs {
  uint32_t key[8];
  uint32_t nonce[3];
  uint32_t counter0;
  uint32_t* out;        // [count][row_words]
  int64_t count;
  int row_words;
  int bits;
};

constexpr int CHACHA_THREADS = 256;                       // lanes = blocks of the keystream per workgroup
constexpr int CHACHA_GROUP_WORDS = 16 * CHACHA_THREADS;   // keystream words per workgroup
constexpr int CHACHA_LDS_ROW = 17;                        // words per lane in LDS (16 + 1: odd stride)

__device__ __forceinline__ uint32_t chacha_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

#define MX_CHACHA_QR(a, b, c, d)                 \
  a += b; d = chacha_rotl(d ^ a, 16);            \
  c += d; b = chacha_rotl(b ^ c, 12);            \
  a += b; d = chacha_rotl(d ^ a, 8);             \
  c += d; b = chacha_rotl(b ^ c, 7);

__global__ __launch_bounds__(CHACHA_THREADS) void chacha20_rows_kernel(const ChaChaArgs a) {
  __shared__ uint32_t lds[CHACHA_THREADS * CHACHA_LDS_ROW];
  const uint32_t t = threadIdx.x;
  const uint32_t w = (uint32_t)(a.bits + 31) >> 5;
  const uint64_t total = (uint64_t)a.count * w;           // keystream words of the call

  // ---- this lane's block (lanes past the last block compute one too: nothing of it is stored)
  const uint32_t s12 = a.counter0 + (uint32_t)((uint64_t)blockIdx.x * CHACHA_THREADS + t);
  uint32_t x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
  uint32_t x4 = a.key[0], x5 = a.key[1], x6 = a.key[2], x7 = a.key[3];
  uint32_t x8 = a.key[4], x9 = a.key[5], x10 = a.key[6], x11 = a.key[7];
  uint32_t x12 = s12, x13 = a.nonce[0], x14 = a.nonce[1], x15 = a.nonce[2];
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    MX_CHACHA_QR(x0, x4, x8, x12) MX_CHACHA_QR(x1, x5, x9, x13) MX_CHACHA_QR(x2, x6, x10, x14) MX_CHACHA_QR(x3, x7, x11, x15)
    MX_CHACHA_QR(x0, x5, x10, x15) MX_CHACHA_QR(x1, x6, x11, x12) MX_CHACHA_QR(x2, x7, x8, x13) MX_CHACHA_QR(x3, x4, x9, x14)
  }
  uint32_t* mine = lds + t * CHACHA_LDS_ROW;
  mine[0] = x0 + 0x61707865u; mine[1] = x1 + 0x3320646eu; mine[2] = x2 + 0x79622d32u; mine[3] = x3 + 0x6b206574u;
  mine[4] = x4 + a.key[0]; mine[5] = x5 + a.key[1]; mine[6] = x6 + a.key[2]; mine[7] = x7 + a.key[3];
  mine[8] = x8 + a.key[4]; mine[9] = x9 + a.key[5]; mine[10] = x10 + a.key[6]; mine[11] = x11 + a.key[7];
  mine[12] = x12 + s12; mine[13] = x13 + a.nonce[0]; mine[14] = x14 + a.nonce[1]; mine[15] = x15 + a.nonce[2];
  __syncthreads();

  // ---- word-major out of LDS: in step k this lane holds word k * 256 + t of the workgroup's 4096
  const uint32_t top = (a.bits & 31) ? ((1u << (a.bits & 31)) - 1u) : 0xFFFFFFFFu;
  const uint32_t step_rows = CHACHA_THREADS / w, step_words = CHACHA_THREADS % w;      // 256 words further on
  uint64_t i = (uint64_t)blockIdx.x * CHACHA_GROUP_WORDS + t;
  uint64_t r = i / w;
  uint32_t j = (uint32_t)(i - r * w);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t lw = (uint32_t)k * CHACHA_THREADS + t;
    uint32_t v = lds[(lw >> 4) * CHACHA_LDS_ROW + (lw & 15)];
    if (j == w - 1) v &= top;
    if (i < total) a.out[r * (uint64_t)a.row_words + j] = v;          // i < total  <=>  r < count; j < w <= row_words
    i += CHACHA_THREADS;
    r += step_rows;
    j += step_words;
    if (j >= w) { j -= w; r += 1; }
  }

  // ---- the zero words beyond w, all lanes of the grid together
  const uint32_t pad = (uint32_t)a.row_words - w;
  if (pad) {
    const uint64_t pad_total = (uint64_t)a.count * pad, stride = (uint64_t)gridDim.x * CHACHA_THREADS;
    for (uint64_t p = (uint64_t)blockIdx.x * CHACHA_THREADS + t; p < pad_total; p += stride) {
      const uint64_t pr = p / pad;                                     // pr < count, w + (p - pr * pad) < row_words
      a.out[pr * (uint64_t)a.row_words + w + (uint32_t)(p - pr * pad)] = 0u;
    }
  }
}

#undef MX_CHACHA_QR

}  // namespace mx
