// SHA-256 (FIPS 180-4) over limb rows on the device: the Fiat-Shamir challenge of the decryption proofs (mx_response.hpp,
// threshold.py) without fetching the rows.  tools/proof_model.py (sha256_rows) is the model; DESIGN.md §4.25.
//
//   digest[r] = SHA-256(prefix | BE(rows_0[r]) | .. | BE(rows_{k-1}[r])),   r < count,   k <= 8 row sets
//
// prefix: 32 bytes, by value in the kernel-argument block as eight big-endian message words.  BE(row): the row as a
// big-endian integer of 4 * limbs bytes — the row's little-endian words in reverse order, and those ARE the hash's
// big-endian message words: no byte is swapped.  The message has W = 8 + sum limbs words; padding is the word
// 0x80000000, zero words, and the 64-bit bit length 32 W in the last two words of the last block, ceil((W + 3) / 16)
// blocks in all.  out[r][j] = H[7 - j]: eight little-endian words whose integer is int.from_bytes(digest, "big").
//
// Mapping: one row per lane, 256 lanes per workgroup.  A lane walks its own row from the top word down; the words of
// one load instruction of a wavefront lie 4 * limbs bytes apart, so a load touches 64 cache lines, and the 31 loads that
// follow hit the same lines (a wavefront's live lines: 8 KiB).  A staged form (the workgroup loads 16-word segments
// side by side into LDS, every lane reads its segment back) would coalesce those loads; it was not built, because the
// hash reads four rows per proof that cost some ten thousand modular products to make: DESIGN.md §4.25 has the measured share.
// The message schedule is a rolling window of sixteen words in registers (every index below is a compile-time constant
// once the rounds are unrolled); the walk over the sets keeps three wave-uniform scalars.  Control flow and addresses
// depend on (count, the widths) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mx {

constexpr int SHA_MAX_SETS = 8;
constexpr int SHA_THREADS = 256;

struct ShaRowsArgs {
  uint32_t prefix[8];                     // big-endian message words 0 .. 7
  const uint32_t* rows[SHA_MAX_SETS];     // set s: [count][limbs[s]]
  int32_t limbs[SHA_MAX_SETS];
  uint32_t* out;                          // [count][8]
  int64_t count;
  int32_t n_sets;
  int32_t words;                          // W = 8 + sum limbs
};

__constant__ const uint32_t SHA256_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

__device__ __forceinline__ uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

__global__ __launch_bounds__(SHA_THREADS) void sha256_rows_kernel(const ShaRowsArgs a) {
  const int64_t lane_row = (int64_t)blockIdx.x * SHA_THREADS + threadIdx.x;
  const int64_t r = lane_row < a.count ? lane_row : a.count - 1;      // lanes past the end hash the last row and store nothing
  const int W = a.words;
  const int nblocks = (W + 3 + 15) >> 4;
  const int last = nblocks * 16 - 1;                                  // the word that holds the low half of the length

  uint32_t h0 = 0x6a09e667u, h1 = 0xbb67ae85u, h2 = 0x3c6ef372u, h3 = 0xa54ff53au;
  uint32_t h4 = 0x510e527fu, h5 = 0x9b05688cu, h6 = 0x1f83d9abu, h7 = 0x5be0cd19u;

  // the walk over the sets: `left` words of set `set` remain, the next one is p[left - 1]
  int set = -1, left = 0;
  const uint32_t* p = nullptr;

  for (int blk = 0; blk < nblocks; ++blk) {
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int g = blk * 16 + k;
      uint32_t v;
      if (k < 8 && blk == 0) {
        v = a.prefix[k];
      } else if (g < W) {
        if (left == 0) {                                              // (every set has at least one word: g < W finds one)
          ++set;
          left = a.limbs[set];
          p = a.rows[set] + r * (int64_t)left;
        }
        --left;
        v = p[left];
      } else {
        v = g == W ? 0x80000000u : (g == last ? (uint32_t)W << 5 : (g == last - 1 ? (uint32_t)W >> 27 : 0u));
      }
      w[k] = v;
    }
    uint32_t A = h0, B = h1, C = h2, D = h3, E = h4, F = h5, G = h6, H = h7;
#pragma unroll
    for (int t = 0; t < 64; ++t) {
      if (t >= 16) {
        const uint32_t x15 = w[(t + 1) & 15], x2 = w[(t + 14) & 15];
        w[t & 15] += (sha_rotr(x15, 7) ^ sha_rotr(x15, 18) ^ (x15 >> 3)) + w[(t + 9) & 15] +
                     (sha_rotr(x2, 17) ^ sha_rotr(x2, 19) ^ (x2 >> 10));
      }
      const uint32_t t1 = H + (sha_rotr(E, 6) ^ sha_rotr(E, 11) ^ sha_rotr(E, 25)) + ((E & F) ^ (~E & G)) + SHA256_K[t] + w[t & 15];
      const uint32_t t2 = (sha_rotr(A, 2) ^ sha_rotr(A, 13) ^ sha_rotr(A, 22)) + ((A & B) ^ (A & C) ^ (B & C));
      H = G; G = F; F = E; E = D + t1; D = C; C = B; B = A; A = t1 + t2;
    }
    h0 += A; h1 += B; h2 += C; h3 += D; h4 += E; h5 += F; h6 += G; h7 += H;
  }
  if (lane_row < a.count) {
    uint32_t* o = a.out + lane_row * 8;
    o[0] = h7; o[1] = h6; o[2] = h5; o[3] = h4; o[4] = h3; o[5] = h2; o[6] = h1; o[7] = h0;
  }
}

}  // namespace mx
