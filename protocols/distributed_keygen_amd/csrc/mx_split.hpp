// A bit field of a radix-2^32 row as lane-distributed radix-2^W limbs: how the kernels that reduce a number WIDER than
// the Montgomery radix R (draws of bits(N) + 64 bits: mx_share.hpp, mx_generators.hpp) cut it into pieces below R.
#pragma once
#include "mx_mont.hpp"

namespace mx {

// This lane's limbs of the bits [bit0, bit0 + nbits) of the number staged in the group's LDS scratch (radix-2^32 words,
// zero padded to Mont::LDS_WORDS by stage_words).
template <int K, int L, int W>
__device__ __forceinline__ void limbs_of_bits(const Mont<K, L, W, true>& M, u32 (&dst)[L], int bit0, int nbits) {
  using M_t = Mont<K, L, W, true>;
  constexpr int LAST = 32 * (M_t::LDS_WORDS - 2);           // the last bit position whose two words lie in the scratch
#pragma unroll
  for (int j = 0; j < L; ++j) {
    const int rel = W * (M.p * L + j);
    const int width = nbits - rel < W ? nbits - rel : W;    // <= 0: the limb lies above the field
    int bit = bit0 + rel;
    bit = bit < LAST ? bit : LAST;
    const int w = bit >> 5, off = bit & 31;
    const u64 v = (u64)M.lds[w] | ((u64)M.lds[w + 1] << 32);
    dst[j] = width > 0 ? ((u32)(v >> off) & (u32)((1u << width) - 1u)) : 0u;
  }
}

}  // namespace mx
