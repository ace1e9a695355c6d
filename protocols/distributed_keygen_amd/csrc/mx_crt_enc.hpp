// Private-key (CRT) Paillier encryption around the half-size modexps, batched over ciphertexts.  Modulo p^2 the reference's
// randomiser r^N is ((r mod p)^(q mod (p-1)) mod p)^p — x -> x^p mod p^2 depends on x mod p only — and a key holder's own
// draw D needs (D mod p^2)^p alone; likewise modulo q^2.  What stands around those modexps:
//
//   crt_split_kernel (mx_crt.hpp) over the plan rows of the PRIMES     r  ->  r mod p, r mod q
//   crt_lift_kernel    rho_p, rho_q [, v]  ->  c_p = v rho_p mod p^2,  c_q = v rho_q mod q^2,
//                                              c = c_p + p^2 ((c_q - c_p) (p^2)^-1 mod q^2),  canonical in [0, N^2)
//                      v = 1 + m N for a message row m below N, a ciphertext's halves (c mod p^2, c mod q^2), or 1;
//                      status bit 0: rho_p = 0, bit 1: rho_q = 0 (p or q divides the randomness), the row is zero then
//
// tools/crt_model.py (CrtEncPlan) is the model at the level of these products, with every operand bound asserted.
//
// The lift folds v in BEFORE Garner's step, so every Montgomery product lives in a lane group that holds a half: with the
// radix R >= 16 max(p^2, q^2) of the launch, per square P
//   a = mont(m, N R^2 mod P) + (R mod P) = (1 + m N) R, < 3 P      or      a = mont(v, R^2 mod P) = v R, < 2 P
//   c_P = mont(a, rho_P) = v rho_P, < 2 P                                   (rho_P < P, a < R)
// c_p is made canonical — it is a summand of the result — and Garner's step modulo q^2 is the recombination's with the
// squares in place of the primes: c_p < p^2 <= R / 16 is a Montgomery operand modulo q^2 whatever the order of the primes,
// and the difference c_q - c_p is taken by complement and carry on the lazy c_p mod q^2.  The only full-width step is the
// plain product c_p + p^2 t (F_PLAIN | F_INIT), written out through the group's wide LDS row.
//
// One group of K lanes per ciphertext; control flow and every address depend on the sizes and the mode only; no private
// segment; plain vector stores.
#pragma once
#include "mx_crt.hpp"

namespace mx {

// rows of the plan, each `rw` words (the width of a half)
constexpr int ENC_ROW_PSPLIT = 0;     // per prime r: r | 2^s Rp mod r | Rp^2 mod r — the rows crt_split_kernel reads
constexpr int ENC_ROW_P = 6;          // P = p^2 | N R^2 mod P | R mod P | R^2 mod P
constexpr int ENC_ROW_Q = 10;         // Q = q^2 | N R^2 mod Q | R mod Q | R^2 mod Q | P^-1 R mod Q
constexpr int ENC_ROWS = 15;

constexpr int LIFT_NOISE = 0, LIFT_MESSAGE = 1, LIFT_HALVES = 2;

struct CrtLiftArgs {
  const u32* rho_p;    // [batch][rw]: below p^2
  const u32* rho_q;    // [batch][rw]: below q^2
  const u32* factor;   // LIFT_MESSAGE: [batch][factor_stride], m below N;  LIFT_HALVES: [2][batch][rw];  LIFT_NOISE: unused
  u32* out;            // [batch][out_stride]: limbs2 words of c, then (if the row is wider) one status word and zeros
  unsigned char* status;   // [batch], or null
  const u32* plan;     // [ENC_ROWS][rw]
  long long batch;
  int mode, factor_stride, factor_words, limbs2, rw, out_stride, nblk;
};

// c = v rho modulo the square M holds (rows: its plan rows), lazy (< 2 P); true when rho is zero
template <int K, int L, int W>
__device__ __forceinline__ bool crt_times_noise(Mont<K, L, W, true>& M, u32 (&c)[L], const u32* rows, const u32* rho_row,
                                                const u32* v_row, int v_words, int mode, int rw) {
  u32 rho[L];
  M.load(rho, rho_row, rw);
  const bool zero = M.is_zero(rho);
  if (mode == LIFT_NOISE) {
#pragma unroll
    for (int j = 0; j < L; ++j) c[j] = rho[j];
    return zero;
  }
  u32 v[L], k[L];
  M.load(v, v_row, v_words);
  M.load(k, rows + (mode == LIFT_MESSAGE ? 1 : 3) * rw, rw);
  M.mul(v, v, k);                                // m N R or v R, < 2 P
  if (mode == LIFT_MESSAGE) {
    M.load(k, rows + 2 * rw, rw);
    M.add(v, v, k);                              // (1 + m N) R, < 3 P
  }
  M.mul(c, v, rho);
  return zero;
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64) crt_lift_kernel(CrtLiftArgs A) {
  aux_wave_priority();
  using M_t = Mont<K, L, W, true>;
  constexpr int S = K * L;
  constexpr int WIDE_WORDS = 2 * S + 8;          // nblk * L low limbs, S high limbs, 4 words of zeros
  extern __shared__ u32 smem[];
  constexpr int GPW = 64 / K;
  const int gw = threadIdx.x / K;
  const long long elem_raw = (long long)blockIdx.x * GPW + gw;
  const bool valid = elem_raw < A.batch;
  const long long elem = valid ? elem_raw : A.batch - 1;
  u32* wide = smem + GPW * M_t::LDS_WORDS + gw * WIDE_WORDS;
  M_t M;
  M.init(smem + gw * M_t::LDS_WORDS, A.nblk);
  const u32* v_p = nullptr;                      // LIFT_NOISE: there is no factor row, and none is addressed
  const u32* v_q = nullptr;
  if (A.mode == LIFT_MESSAGE) {
    v_p = v_q = A.factor + elem * A.factor_stride;
  } else if (A.mode == LIFT_HALVES) {
    v_p = A.factor + elem * A.rw;
    v_q = A.factor + (A.batch + elem) * A.rw;
  }

  // ---- modulo p^2: c_p canonical, it is a summand of the result
  const u32* rows_p = A.plan + (size_t)ENC_ROW_P * A.rw;
  M.load(M.n, rows_p, A.rw);
  M.setup_modulus();
  u32 cp[L];
  const bool zero_p = crt_times_noise(M, cp, rows_p, A.rho_p + elem * A.rw, v_p, A.factor_words, A.mode, A.rw);
  crt_canonical(M, cp);

  // ---- modulo q^2: c_q stays lazy, then Garner's t = (c_q - c_p) (p^2)^-1 mod q^2
  const u32* rows_q = A.plan + (size_t)ENC_ROW_Q * A.rw;
  M.load(M.n, rows_q, A.rw);
  M.setup_modulus();
  u32 t[L];
  const bool zero_q = crt_times_noise(M, t, rows_q, A.rho_q + elem * A.rw, v_q, A.factor_words, A.mode, A.rw);
  {
    u32 k[L], a[L];
    M.load(k, rows_q + 2 * A.rw, A.rw);
    M.mul(a, cp, k);                             // c_p modulo q^2, < 2 Q (c_p < P <= R / 16)
    u64 c[L];
#pragma unroll
    for (int j = 0; j < L; ++j) c[j] = a[j];
    M.normalize_full(a, c);
    // d = c_q + 2 Q - a in (0, 4 Q): the complement of a's exact limbs plus one, the carry out of the top dropped
#pragma unroll
    for (int j = 0; j < L; ++j) c[j] = (u64)t[j] + 2 * (u64)M.n[j] + (u64)(M_t::MASK - a[j]);
    if (M.p == 0) c[0] += 1;
    M.normalize_full(t, c);
    M.load(k, rows_q + 4 * A.rw, A.rw);
    M.mul(t, t, k);
    crt_canonical(M, t);
  }

  // ---- c = c_p + p^2 t by a plain product: the low limbs leave through `wide`, the high part stays in the lanes
  const bool ok = !zero_p && !zero_q;
  u32 pl[L], hi[L];
  M.load(pl, rows_p, A.rw);
  M.template mulx<M_t::F_INIT | M_t::F_PLAIN>(hi, t, pl, t, pl, cp, nullptr, wide, A.nblk);
  {
    u64 c[L];
#pragma unroll
    for (int j = 0; j < L; ++j) c[j] = hi[j];
    M.normalize_full(hi, c);
  }
  const int it = A.nblk * L;
#pragma unroll
  for (int j = 0; j < L; ++j) wide[it + M.p * L + j] = hi[j];
  if (M.p == 0) { wide[it + S] = 0; wide[it + S + 1] = 0; wide[it + S + 2] = 0; wide[it + S + 3] = 0; }
  __syncthreads();
  u32* dst = A.out + elem * A.out_stride;
  const int nl = it + S;
  for (int k = M.p; k < A.limbs2; k += K) {
    const int bit = 32 * k;
    const int g = bit / W, off = bit - g * W;
    u32 o = 0;
    if (g < nl) {
      u64 v = (u64)wide[g] >> off;
      v |= (u64)wide[g + 1] << (W - off);
      if (2 * W - off < 32) v |= (u64)wide[g + 2] << (2 * W - off);
      o = (u32)v;
    }
    if (valid) dst[k] = ok ? o : 0u;
  }
  if (valid && M.p == 0) {
    const u32 st = (zero_p ? 1u : 0u) | (zero_q ? 2u : 0u);
    if (A.status) A.status[elem] = (unsigned char)st;
    for (int k = A.limbs2; k < A.out_stride; ++k) dst[k] = (k == A.limbs2) ? st : 0u;
  }
}

}  // namespace mx
