// Packing of ciphertexts modulo a SQUARE:
//   out[j] = prod_{i < slots} cts[j * slots + i] ^ (2^(slot_bits * i))  mod N^2,   j < ceil(count / slots)
// which, with g = N + 1, encrypts sum_i m_i * 2^(slot_bits * i): one threshold decryption returns `slots` small plaintexts
// (DESIGN.md §4.10).  Rows at index `count` or above count as 1, so the last output may hold fewer slots.
//
// Horner on the pair arithmetic of mx_powmod_n2.hpp, one group of lanes per output: acc = one; for every slot from the
// top, slot_bits pair squarings (none before the top slot) and one pair multiplication by conv(c_i); then the product by
// E = (1, 0) and the epilogue of multiexp_n2_kernel, so outputs are canonical residues in [0, N^2).  conv is the one of
// multiexp_n2_table_kernel, (x_lo, 0) * K1 + (x_hi, 0) * K2 with the plan's constant rows.  A missing row converts the
// last present row like any other and then selects the domain's one (ONE0, ONE1) in its place: every group of a
// wavefront executes the same slots and squarings (`slots` and `slot_bits` are launch arguments), so control flow stays
// wave-uniform (the property DESIGN §3 relies on).  The Straus kernel would run every window for every slot; here each
// weight has one nonzero bit and the chain is (slots - 1) * slot_bits <= bits(N) squarings long.
#pragma once
#include "mx_multiexp_n2.hpp"

namespace mx {

struct PackN2Args {
  const u32* cts;       // [count][limbs2] residues < N^2
  const u32* consts;    // [8][limbsn] the plan's constant rows of this geometry: N, ONE0, ONE1, K1_0, K1_1, K2_0, K2_1, C'
  u32* out;             // [outputs][limbs2]
  i64 count, outputs;   // outputs = ceil(count / slots)
  int slots, slot_bits;
  int limbsn, limbs2, nblk;
  int ksplit;           // x = x_lo + 2^ksplit * x_hi, ksplit = bits(N) - 1
};

template <int K, int L>
constexpr size_t pack_n2_lds_bytes() { return powmod_n2_lds_bytes<K, L>(false); }

// Two wavefronts per SIMD: the accumulator pair stays live across the conversion's two products, and bounded to three
// (168 VGPRs) the compiler spilled 288-312 B per lane.  A launch of 10^5 values at key_length 2048 is ~200 wavefronts.
// The conversion and the epilogue below are this kernel's own copies of pair_convert and pair_store (mx_powmod_n2.hpp):
// built on the shared functions the kernel kept its registers but measured 5.5 % slower (18.2 -> 19.2 ms for the chain of
// 64 slots of 32 bits at key_length 2048, profiles/r12_fold_probes_ab.txt), so only the set-up is shared here.
template <int K, int L, int W>
__global__ void __launch_bounds__(64, 2) pack_n2_kernel(PackN2Args A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int S = M_t::S;
  constexpr int GPW = 64 / K;
  constexpr int WIDE = M_t::LDS_WORDS;
  extern __shared__ u32 smem[];
  const int lane = threadIdx.x;
  const int gw = lane / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const i64 r = raw < A.outputs ? raw : A.outputs - 1;   // surplus groups redo the last output and store nothing
  M_t M;
  u32* cp_lds = pair_setup<K, L>(M, smem, gw, A.consts, A.limbsn, A.nblk);
  PairArith<K, L, W> P(M, cp_lds);
  const int p = M.p;
  u32* wide = smem + gw * M_t::LDS_WORDS;
  // (x0, x1) = conv(row `e`), or the domain's one where the row is missing
  auto conv = [&](i64 e, u32 (&x0)[L], u32 (&x1)[L]) {
    const bool present = e < A.count;
    const u32* src = A.cts + (present ? e : A.count - 1) * A.limbs2;
    // the two halves of x = x_lo + 2^k x_hi, as powmod_n2_kernel's prologue splits them
    __syncthreads();
    for (int k = p; k < WIDE; k += K) wide[k] = (k < A.limbs2) ? src[k] : 0u;
    __syncthreads();
    u32 lo[L], hi[L], zero[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const int bit = W * (p * L + j);
      const int room = A.ksplit - bit;
      lo[j] = room <= 0 ? 0u : extract_field(wide, bit, room < W ? room : W);
      const int hbit = A.ksplit + bit;
      hi[j] = (hbit + W + 32 <= 32 * WIDE) ? extract_field(wide, hbit, W) : 0u;
      zero[j] = 0u;
    }
    // x = (x_lo, 0) * K1 + (x_hi, 0) * K2; constant pairs are loaded where they are used
    u32 t0[L], t1[L];
    M.load(t0, A.consts + 3 * A.limbsn, A.limbsn);
    M.load(t1, A.consts + 4 * A.limbsn, A.limbsn);
    P.mul(x0, x1, lo, zero, t0, t1);
    M.load(t0, A.consts + 5 * A.limbsn, A.limbsn);
    M.load(t1, A.consts + 6 * A.limbsn, A.limbsn);
    P.mul(t0, t1, hi, zero, t0, t1);
    M.add(x0, x0, t0);
    M.add(x1, x1, t1);
    M.load(t0, A.consts + 1 * A.limbsn, A.limbsn);        // the domain's one
    M.load(t1, A.consts + 2 * A.limbsn, A.limbsn);
#pragma unroll
    for (int j = 0; j < L; ++j) {
      x0[j] = present ? x0[j] : t0[j];
      x1[j] = present ? x1[j] : t1[j];
    }
  };
  // acc = one, then from the top slot: slot_bits squarings (none before the top slot) and the product by conv(c_i) — one
  // pair product more than starting from acc = conv(c_top), for a single call site of the conversion
  const i64 base = r * A.slots;
  u32 acc0[L], acc1[L];
  M.load(acc0, A.consts + 1 * A.limbsn, A.limbsn);
  M.load(acc1, A.consts + 2 * A.limbsn, A.limbsn);
  for (int i = A.slots - 1; i >= 0; --i) {
    if (i != A.slots - 1)
      for (int s = 0; s < A.slot_bits; ++s) P.sqr(acc0, acc1, acc0, acc1);
    u32 x0[L], x1[L];
    conv(base + i, x0, x1);
    P.mul(acc0, acc1, acc0, acc1, x0, x1);
  }
  // the last product, by E = (1, 0): the N-adic digits of the residue (mx_powmod_n2.hpp)
  {
    u32 e0[L], e1[L];
    M.set_small(e0, 1u);
    M.set_small(e1, 0u);
    P.mul(acc0, acc1, acc0, acc1, e0, e1);
  }
  // ---- epilogue of powmod_n2_kernel: digits into [0, N), then z = Y0 + Y1 * N by a plain product
  {
    u64 t[L];
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = acc0[j];
    M.normalize_full(acc0, t);
    const u32 carry = M.cond_sub(acc0);
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = acc1[j];
    if (p == 0) t[0] += carry;
    M.normalize_full(acc1, t);
    M.cond_sub(acc1);
  }
  u32 hi[L];
  __syncthreads();
  M.template mulx<M_t::F_INIT | M_t::F_PLAIN>(hi, acc1, M.n, acc1, M.n, acc0, nullptr, wide, A.nblk);
  {
    u64 t[L];
#pragma unroll
    for (int j = 0; j < L; ++j) t[j] = hi[j];
    M.normalize_full(hi, t);
  }
  const int it = A.nblk * L;
#pragma unroll
  for (int j = 0; j < L; ++j) wide[it + p * L + j] = hi[j];
  if (p == 0) { wide[it + S] = 0; wide[it + S + 1] = 0; wide[it + S + 2] = 0; wide[it + S + 3] = 0; }
  __syncthreads();
  const bool valid = raw < A.outputs;
  u32* dst = A.out + r * A.limbs2;
  const int nl = it + S;
  for (int k = p; k < A.limbs2; k += K) {
    const int bit = 32 * k;
    const int g = bit / W, off = bit - g * W;
    u32 o = 0;
    if (g < nl) {
      u64 v = (u64)wide[g] >> off;
      v |= (u64)wide[g + 1] << (W - off);
      if (2 * W - off < 32) v |= (u64)wide[g + 2] << (2 * W - off);
      o = (u32)v;
    }
    if (valid) dst[k] = o;
  }
}

}  // namespace mx
