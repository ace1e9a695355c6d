// Slot-packed plaintexts: the codec between int64 values and the plaintext rows of the C ABI (radix-2^32 words, element-major)
// in the layout packing.py fixes — value j k + i in bits [b i, b (i + 1)) of plaintext j, signed plaintexts reduced modulo N.
// DESIGN.md §4.14.
//
//   encode   T = sum_i ((m_i + 2^(b-1)) mod 2^b) 2^(b i)   (signed: every field made non-negative),   S = T - off,
//            off = 2^(b-1) sum_{i<k} 2^(b i);   row = S < 0 ? S + N : S.     Unsigned: row = sum_i m_i 2^(b i).
//   decode   U = ((v > N div 2 ? v - N : v) + off) mod 2^(b k);   m_i = field i of U - 2^(b-1).   Unsigned: U = v mod 2^(b k).
//
// Mapping, the same for both kernels: a workgroup of 256 lanes owns R consecutive plaintexts, whose rows stand in LDS
// (row stride odd, so the lanes of a wavefront that each walk their own row fall into different banks).  Three phases:
//   A  word-major over the R rows: lane <-> (row, word), consecutive lanes consecutive words.  encode gathers the fields
//      that overlap its word straight from the values (neighbouring lanes read neighbouring values) and checks their range;
//      decode copies the plaintext words in.  No two lanes write the same LDS word.
//   B  one lane per row: the multi-word borrow / carry chain over the row in LDS — T - off then + N, or v (- N) + off.  The
//      chain is serial by nature and short (a word per step); N and off are read at a wave-uniform index from the
//      kernel-argument block.  Skipped for unsigned slots.
//   C  word-major again (encode: the rows, zero beyond N's words) or value-major (decode: lane <-> value, every field read
//      from up to three LDS words): a store instruction of a wavefront writes 64 consecutive words / int64 values.
// Lanes past the last row or value read nothing from global memory and store nothing.  Registers and LDS only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mx {

constexpr int SLOTS_THREADS = 256;
constexpr int SLOTS_MAX_WORDS = 258;            // words of N a launch takes (N up to 8224 bits and a spare word)
constexpr int SLOTS_LDS_BUDGET = 48 * 1024;     // bytes of row storage per workgroup

struct SlotsArgs {
  uint32_t n[SLOTS_MAX_WORDS];       // N, zero padded
  uint32_t off[SLOTS_MAX_WORDS];     // 2^(b-1) sum_{i<k} 2^(b i) for signed slots, else zero
  const int64_t* values;             // encode: [count]
  int64_t* values_out;               // decode: [count]
  const uint32_t* rows_in;           // decode: [outputs][stride]
  uint32_t* rows_out;                // encode: [outputs][stride]
  unsigned char* status;             // encode: [outputs]
  int64_t count, outputs;
  int limbs, stride, slot_bits, slots, is_signed;
  int rows_per_group, lds_stride;    // R and the odd row stride in LDS (>= limbs + 2: two zero words behind every row)
};

__device__ __forceinline__ int slots_rows_here(const SlotsArgs& a, int64_t row0) {
  const int64_t left = a.outputs - row0;
  return left < a.rows_per_group ? (int)left : a.rows_per_group;
}

__global__ __launch_bounds__(SLOTS_THREADS) void slots_encode_kernel(const SlotsArgs a) {
  extern __shared__ uint32_t slots_lds[];
  __shared__ uint32_t bad[SLOTS_THREADS];
  const int t = threadIdx.x, R = a.rows_per_group, L = a.limbs, b = a.slot_bits, k = a.slots;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int rows = slots_rows_here(a, row0);
  const uint64_t bias = a.is_signed ? (uint64_t)1 << (b - 1) : 0;
  const uint64_t fmask = b == 64 ? ~(uint64_t)0 : ((uint64_t)1 << b) - 1;
  const int used_bits = b * k;
  bad[t] = 0;
  __syncthreads();

  // ---- A: the words of T
  for (int idx = t; idx < R * L; idx += SLOTS_THREADS) {
    const int r = idx / L, w = idx - r * L;
    const int lo_bit = 32 * w;
    uint32_t word = 0;
    if (r < rows && lo_bit < used_bits) {
      const int64_t e0 = (row0 + r) * k;
      for (int i = lo_bit / b; i < k && b * i < lo_bit + 32; ++i) {
        const int64_t e = e0 + i;
        const uint64_t u = (e < a.count ? (uint64_t)a.values[e] : 0) + bias;      // a missing slot holds 0
        if (u & ~fmask) bad[r] = 1;                                                // (lanes that race store the same 1)
        const uint64_t f = u & fmask;
        const int d = b * i - lo_bit;                                              // -63 .. 31
        word |= d >= 0 ? (uint32_t)f << d : (uint32_t)(f >> -d);
      }
    }
    slots_lds[r * a.lds_stride + w] = word;
  }
  __syncthreads();

  // ---- B: S = T - off, + N when negative; one lane per row, every lane the same word in the same step
  if (a.is_signed && t < rows) {
    uint32_t* row = slots_lds + t * a.lds_stride;
    int64_t c = 0;
    for (int w = 0; w < L; ++w) {
      const int64_t v = (int64_t)row[w] - (int64_t)a.off[w] + c;
      row[w] = (uint32_t)v;
      c = v >> 32;
    }
    const bool neg = c < 0;
    uint64_t cc = 0;
    for (int w = 0; w < L; ++w) {
      const uint64_t v = (uint64_t)row[w] + (neg ? a.n[w] : 0u) + cc;
      row[w] = (uint32_t)v;
      cc = v >> 32;
    }
  }
  __syncthreads();

  // ---- C: rows and status bytes out
  const int S = a.stride;
  uint32_t* out = a.rows_out + row0 * S;                    // rows < R rows of this group: idx < rows * S is in bounds
  for (int idx = t; idx < rows * S; idx += SLOTS_THREADS) {
    const int r = idx / S, w = idx - r * S;
    out[idx] = w < L ? slots_lds[r * a.lds_stride + w] : 0u;
  }
  if (t < rows) a.status[row0 + t] = bad[t] ? 1 : 0;
}

__global__ __launch_bounds__(SLOTS_THREADS) void slots_decode_kernel(const SlotsArgs a) {
  extern __shared__ uint32_t slots_lds[];
  const int t = threadIdx.x, R = a.rows_per_group, L = a.limbs, b = a.slot_bits, k = a.slots;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int rows = slots_rows_here(a, row0);

  // ---- A: the plaintext words in (words beyond N's are not read), two zero words behind every row
  const int LZ = L + 2;
  for (int idx = t; idx < R * LZ; idx += SLOTS_THREADS) {
    const int r = idx / LZ, w = idx - r * LZ;
    slots_lds[r * a.lds_stride + w] = (r < rows && w < L) ? a.rows_in[(row0 + r) * a.stride + w] : 0u;
  }
  __syncthreads();

  // ---- B: U = (v > N div 2 ? v - N : v) + off modulo 2^(32 L); one lane per row
  if (a.is_signed && t < rows) {
    uint32_t* row = slots_lds + t * a.lds_stride;
    bool above = false, decided = false;                    // v > N div 2, from the top word down
    for (int w = L - 1; w >= 0; --w) {
      const uint32_t h = (a.n[w] >> 1) | (w + 1 < L ? a.n[w + 1] << 31 : 0u);
      const uint32_t v = row[w];
      if (!decided && v != h) { decided = true; above = v > h; }
    }
    int64_t c = 0;
    for (int w = 0; w < L; ++w) {
      const int64_t v = (int64_t)row[w] + (int64_t)a.off[w] - (above ? (int64_t)a.n[w] : 0) + c;
      row[w] = (uint32_t)v;
      c = v >> 32;
    }
  }
  __syncthreads();

  // ---- C: one lane per value; field i of its row's U (bits at b k and above are never part of a field)
  const int64_t e0 = row0 * k;
  const int64_t left = a.count - e0;
  const int here = left < (int64_t)rows * k ? (int)left : rows * k;
  const uint64_t fmask = b == 64 ? ~(uint64_t)0 : ((uint64_t)1 << b) - 1;
  const uint64_t bias = a.is_signed ? (uint64_t)1 << (b - 1) : 0;
  for (int idx = t; idx < here; idx += SLOTS_THREADS) {
    const int r = idx / k, i = idx - r * k;
    const int bit = b * i, w = bit >> 5, sh = bit & 31;    // w + 2 <= L + 1: inside the row and its two zero words
    const uint32_t* row = slots_lds + r * a.lds_stride;
    uint64_t f = ((uint64_t)row[w] | ((uint64_t)row[w + 1] << 32)) >> sh;
    if (sh) f |= (uint64_t)row[w + 2] << (64 - sh);
    a.values_out[e0 + idx] = (int64_t)((f & fmask) - bias);
  }
}

}  // namespace mx
