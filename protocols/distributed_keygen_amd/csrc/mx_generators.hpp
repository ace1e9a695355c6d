// The generator step of a key-generation round (`__biprime_test_g_generation`, distributed_keygen.py:1001-1054), batched
// over the survivors of the sieve — S candidate moduli N_c, G generators each, one MODULUS PER GROUP of G rows:
//
//   generator_setup_kernel   r2[c] = R^2 mod N_c, canonical, for every candidate (R mod N_c by doubling as in mx_setup.hpp,
//                            then Mont::compute_r2): the one per-modulus constant of the two kernels below
//   generator_share_kernel   s[c G + k] = D[c G + k] mod N_c      D: a draw of B + 64 bits, B = the widest modulus
//   generator_sum_kernel     g[c G + k] = sum_j share_j[c G + k] mod N_c      any share below 2^(32 limbs)
//
// Both reduce a number X that may be wider than R, and far wider than a short N_c (moduli of different lengths share a
// launch).  X is cut at s = B - 1 into lo < 2^s and hi; with the integer 2^s as a plain Montgomery operand
//   h  = mont(mont(hi, r2), 2^s)      = hi 2^s mod N_c, lazy (< 2 N_c)
//   t  = lo + h                       < R (see below), = X modulo N_c
//   X mod N_c = mont(mont(t, r2), 1)  one conditional subtraction behind it
// — mont(a, b) = a b / R mod N is below 2 N for ANY a < R when b < N (a b / R < N), which is what lets t be reduced
// without being below a small multiple of N_c.  Four products per row, no division, nothing converted into the domain.
//
// The sum: the lo and the hi pieces of the parties' shares are added limb-wise in 64-bit columns (limbs below 2^29, at
// most MX_GEN_MAX_PARTIES of them) and carried once; then the same four products, once.
//   t < parties * 2^(B-1) + 2^(B+1) = (parties + 4) 2^(B-1)  must stay below R >= 2^(B+4):  parties <= 28.
//
// One group of K lanes per row (the geometry of the 9-limb kernels).  Control flow and every address depend on (S, G,
// parties, limbs, B) only; no private segment; plain vector stores through Mont::store.
#pragma once
#include "mx_mont.hpp"
#include "mx_split.hpp"

namespace mx {

struct GeneratorSetupArgs {
  const u32* mods;   // [groups][limbs]
  u32* r2;           // [groups][limbs] (out)
  long long groups;
  int limbs, nblk;
};

struct GeneratorArgs {
  const u32* rows;   // [parties][batch][words]: the draws (parties = 1, words = cw) or the parties' shares (words = limbs)
  u32* out;          // [batch][limbs]
  const u32* mods;   // [groups][limbs]
  const u32* r2;     // [groups][limbs]: R^2 mod N_c, canonical
  long long batch;   // groups * group_size
  long long group_size;
  int limbs, nblk, words, split_bit, parties;
};

// lazy x < 4 N (Montgomery domain or not) times the canonical b -> the canonical residue of x b / R
template <int K, int L, int W>
__device__ __forceinline__ void generator_canonical(Mont<K, L, W, true>& M, u32 (&x)[L], const u32 (&b)[L]) {
  M.mul(x, x, b);
  u64 t[L];
#pragma unroll
  for (int j = 0; j < L; ++j) t[j] = x[j];
  M.normalize_full(x, t);
  M.cond_sub(x);
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64) generator_setup_kernel(GeneratorSetupArgs A) {
  using M_t = Mont<K, L, W, true>;
  extern __shared__ u32 smem[];
  constexpr int GPW = 64 / K;
  const int gw = threadIdx.x / K;
  const long long g_raw = (long long)blockIdx.x * GPW + gw;
  const bool valid = g_raw < A.groups;
  const long long g = valid ? g_raw : A.groups - 1;
  M_t M;
  M.init(smem + gw * M_t::LDS_WORDS, A.nblk);
  M.load(M.n, A.mods + g * A.limbs, A.limbs);
  M.setup_modulus();
  u32 one_m[L], r2[L];
  M.rmodn_by_doubling(one_m);
  M.compute_r2(r2, one_m);                      // lazy, < 4 N, = R^2 as a residue
  generator_canonical(M, r2, one_m);            // r2 R / R
  M.store(A.r2 + g * A.limbs, A.limbs, r2, valid);
}

// lo (lazy limbs, value < R together with 2 N) + hi 2^s, reduced: the canonical residue in lo
template <int K, int L, int W>
__device__ __forceinline__ void generator_fold(Mont<K, L, W, true>& M, u32 (&lo)[L], u32 (&hi)[L], const u32 (&r2)[L], int split_bit) {
  u32 c[L];
  const int limb = split_bit / W;
#pragma unroll
  for (int j = 0; j < L; ++j) c[j] = (M.p * L + j == limb) ? (1u << (split_bit - limb * W)) : 0u;      // the integer 2^s
  M.mul(hi, hi, r2);            // hi R
  M.mul(hi, hi, c);             // hi 2^s, < 2 N
  M.add(lo, lo, hi);            // = X modulo N, < R
  M.mul(lo, lo, r2);            // X R, < 2 N
  M.set_small(c, 1);
  generator_canonical(M, lo, c);
}

// What both kernels share: the row's modulus and its constant, the geometry of the launch.
template <int K, int L, int W>
struct GeneratorRow {
  using M_t = Mont<K, L, W, true>;
  M_t M;
  u32 r2[L];
  long long elem;
  bool valid;
  __device__ __forceinline__ void init(const GeneratorArgs& A, u32* smem) {
    constexpr int GPW = 64 / K;
    const int gw = threadIdx.x / K;
    const long long elem_raw = (long long)blockIdx.x * GPW + gw;
    valid = elem_raw < A.batch;
    elem = valid ? elem_raw : A.batch - 1;
    const long long c = elem / A.group_size;
    M.init(smem + gw * M_t::LDS_WORDS, A.nblk);
    M.load(M.n, A.mods + c * A.limbs, A.limbs);
    M.setup_modulus();
    M.load(r2, A.r2 + c * A.limbs, A.limbs);
  }
};

template <int K, int L, int W>
__global__ void __launch_bounds__(64) generator_share_kernel(GeneratorArgs A) {
  using M_t = Mont<K, L, W, true>;
  extern __shared__ u32 smem[];
  GeneratorRow<K, L, W> G;
  G.init(A, smem);
  G.M.stage_words(A.rows + G.elem * A.words, A.words);
  u32 lo[L], hi[L];
  limbs_of_bits(G.M, lo, 0, A.split_bit);
  limbs_of_bits(G.M, hi, A.split_bit, 32 * M_t::LDS_WORDS);      // up to the end of the draw: the scratch is zero beyond it
  generator_fold(G.M, lo, hi, G.r2, A.split_bit);                 // (its first barrier is behind every lane's reads of the draw)
  G.M.store(A.out + G.elem * A.limbs, A.limbs, lo, G.valid);
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64) generator_sum_kernel(GeneratorArgs A) {
  using M_t = Mont<K, L, W, true>;
  extern __shared__ u32 smem[];
  GeneratorRow<K, L, W> G;
  G.init(A, smem);
  u64 slo[L], shi[L];
#pragma unroll
  for (int j = 0; j < L; ++j) { slo[j] = 0; shi[j] = 0; }
  for (int party = 0; party < A.parties; ++party) {
    G.M.stage_words(A.rows + ((long long)party * A.batch + G.elem) * A.words, A.words);
    u32 lo[L], hi[L];
    limbs_of_bits(G.M, lo, 0, A.split_bit);
    limbs_of_bits(G.M, hi, A.split_bit, 32 * M_t::LDS_WORDS);
#pragma unroll
    for (int j = 0; j < L; ++j) { slo[j] += lo[j]; shi[j] += hi[j]; }
  }
  u32 lo[L], hi[L];
  G.M.normalize_weak(lo, slo);
  G.M.normalize_weak(hi, shi);
  generator_fold(G.M, lo, hi, G.r2, A.split_bit);
  G.M.store(A.out + G.elem * A.limbs, A.limbs, lo, G.valid);
}

}  // namespace mx
