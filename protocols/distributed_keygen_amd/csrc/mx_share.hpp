// The step of a key-generation round in front of the candidate moduli (distributed_keygen.py:718-853), batched over
// the candidates of a round — random rows in, additive shares and their Shamir sharings out:
//
//   share_candidates_kernel   out[e] = 2^(L-1) + (r[e] << 2) + m4     (DK:874-875; m4 = 3 for party 1, else 0)
//       r[e]: a row of L - 3 random bits.  A word-wise funnel shift: no big-integer arithmetic.
//   shamir_share_kernel       out[j][e] = s[e] + sum_{k=1..degree} (D[k][e] mod P) * x_j^k  mod P
//       `ShamirVariable.share()` (utils.py:253-260) of every candidate: a polynomial of degree `degree` with constant
//       term s[e] (or 0: the sharing of zero) and coefficients a_k = D[k][e] mod P, evaluated at the public points x_j.
//       D[k][e] has bits(P) + 64 bits, so a_k is uniform on [0, P) up to a bias below 2^-64.
//
// shamir_share_kernel: one group of K lanes per element, the lane-distributed Montgomery engine of mx_field.hpp, one
// modulus per launch.  Per element:
//   1. every draw D is split at s = bits(P) - 1 into lo < 2^s < P and hi < 2^65, and a = hi * (2^s mod P) + lo is one
//      Montgomery product with the host's constant 2^s R mod P and one lazy sum (a < 3 P; a = D mod P as a residue);
//      the `degree` coefficients are parked in LDS, each lane its own limbs (no lane reads another's: no barrier);
//   2. per point Horner from the top coefficient down: acc <- acc * x_j + a_k is one product with the host's constant
//      x_j R mod P — the R cancels, so nothing is ever converted into or out of the Montgomery domain — and one lazy sum
//      (acc < 5 P going into a product whose other operand is below P: acc * x_j R < R P since R >= 16 P, the bound
//      mx_mont.hpp states for a result below 2 P);
//   3. acc + s is reduced as in fma_kernel (a product with R mod P, exact limbs, one conditional subtraction) and
//      stored as the canonical residue in out[j][e]: layout [n_points][batch][limbs], what lincomb_kernel reads.
// degree + degree * n_points + n_points products per element.
//
// Control flow and every address depend on (batch, degree, n_points, limbs, bits(P)) only; no table is read, so nothing
// is indexed by a secret.
#pragma once
#include "mx_mont.hpp"
#include "mx_split.hpp"

namespace mx {

struct CandidateArgs {
  const u32* random;    // [count][in_words], in_words = ceil((prime_length - 3) / 32); bits above prime_length - 3 zero
  u32* out;             // [count][row_words]
  long long count;
  int prime_length, in_words, row_words;
  u32 mod4;             // 3 for the first party, 0 for the others
};

constexpr int CANDIDATE_THREADS = 256;

// One lane per output word.
__global__ void __launch_bounds__(CANDIDATE_THREADS) share_candidates_kernel(const CandidateArgs a) {
  const unsigned long long i = (unsigned long long)blockIdx.x * CANDIDATE_THREADS + threadIdx.x;
  const unsigned long long total = (unsigned long long)a.count * (unsigned)a.row_words;
  if (i >= total) return;
  const unsigned long long e = i / (unsigned)a.row_words;
  const int j = (int)(i - e * (unsigned)a.row_words);
  const u32* r = a.random + e * (unsigned long long)a.in_words;
  const u32 here = j < a.in_words ? r[j] : 0u;
  const u32 below = (j >= 1 && j - 1 < a.in_words) ? r[j - 1] : 0u;
  u32 v = (here << 2) | (below >> 30);                      // r << 2 has prime_length - 1 bits: the top bit is free
  if (j == 0) v |= a.mod4;
  const int top = a.prime_length - 1;
  if (j == (top >> 5)) v |= 1u << (top & 31);
  a.out[i] = v;
}

struct ShareArgs {
  const u32* secrets;   // [batch][limbs], each < P; null: a sharing of zero
  const u32* draws;     // [degree][batch][cw]: D[k][e], bits(P) + 64 bits each
  u32* out;             // [n_points][batch][limbs]
  const u32* mod;       // [limbs]
  const u32* rmodn;     // [limbs]: R mod P
  const u32* split;     // [limbs]: 2^s R mod P, s = split_bit
  const u32* xr;        // [n_points][limbs]: x_j R mod P
  long long batch;
  int limbs, nblk, degree, n_points, cw, split_bit;
};

// Dynamic LDS: 64 / K groups of Mont::LDS_WORDS words, then 64 / K groups of degree * K * L words (the coefficients).
template <int K, int L, int W>
__global__ void __launch_bounds__(64) shamir_share_kernel(ShareArgs A) {
  using M_t = Mont<K, L, W, true>;
  extern __shared__ u32 smem[];
  constexpr int GPW = 64 / K;
  const int gw = threadIdx.x / K;
  const long long elem_raw = (long long)blockIdx.x * GPW + gw;
  const bool valid = elem_raw < A.batch;
  const long long elem = valid ? elem_raw : A.batch - 1;
  M_t M;
  M.init(smem + gw * M_t::LDS_WORDS, A.nblk);
  u32* coef = smem + GPW * M_t::LDS_WORDS + (gw * A.degree) * M_t::S + M.p * L;     // this lane's limbs of a_1
  M.load(M.n, A.mod, A.limbs);
  M.setup_modulus();
  {
    u32 c[L];
    M.load(c, A.split, A.limbs);
    for (int k = 0; k < A.degree; ++k) {
      M.stage_words(A.draws + ((long long)k * A.batch + elem) * A.cw, A.cw);
      u32 lo[L], hi[L];
      limbs_of_bits(M, lo, 0, A.split_bit);
      limbs_of_bits(M, hi, A.split_bit, 32 * M_t::LDS_WORDS);   // up to the end of the draw: the scratch is zero beyond it
      M.mul(hi, hi, c);         // hi 2^s mod P   (lazy, < 2P; its first barrier is behind every lane's reads of the draw)
      M.add(lo, lo, hi);        // a_k < 3P
#pragma unroll
      for (int j = 0; j < L; ++j) coef[k * M_t::S + j] = lo[j];
    }
  }
  u32 one_m[L], s[L];
  M.load(one_m, A.rmodn, A.limbs);
  if (A.secrets) {
    M.load(s, A.secrets + elem * A.limbs, A.limbs);
  } else {
#pragma unroll
    for (int j = 0; j < L; ++j) s[j] = 0;
  }
  for (int pt = 0; pt < A.n_points; ++pt) {
    u32 x[L], acc[L];
    M.load(x, A.xr + (long long)pt * A.limbs, A.limbs);
#pragma unroll
    for (int j = 0; j < L; ++j) acc[j] = coef[(A.degree - 1) * M_t::S + j];
    for (int k = A.degree - 2; k >= 0; --k) {
      u32 a[L];
#pragma unroll
      for (int j = 0; j < L; ++j) a[j] = coef[k * M_t::S + j];
      M.mul(acc, acc, x);       // acc x_j   (lazy, < 2P)
      M.add(acc, acc, a);       // < 5P
    }
    M.mul(acc, acc, x);
    M.add(acc, acc, s);         // the value of the polynomial at x_j, < 3P
    M.mul(acc, acc, one_m);     // the same modulo P, lazy < 2P
    {
      u64 t[L];
#pragma unroll
      for (int j = 0; j < L; ++j) t[j] = acc[j];
      M.normalize_full(acc, t);
    }
    M.cond_sub(acc);
    M.store(A.out + ((long long)pt * A.batch + elem) * A.limbs, A.limbs, acc, valid);
  }
}

}  // namespace mx
