// Multi-exponentiation modulo a GENERIC odd modulus:
//
//   out[r] = prod_{t < terms} inputs[index[r][t]] ^ weights[r][t]  mod M      (weights >= 0, one odd M >= 3 per launch)
//
// the sibling of mx_multiexp_n2.hpp on the plain Montgomery arithmetic of mx_mont.hpp (Mont<K, L, W, true>, as
// mx_field.hpp and mx_powmod.hpp use it).  Interleaved fixed-window (Straus) form:
//
//   table pass  (multiexp_table_kernel): one group of lanes per input; brings the row into the Montgomery domain and
//               writes its 2^w powers, entry 0 being the domain's one (R mod M), into the caller's workspace;
//   main pass   (multiexp_kernel): one group of lanes per output row; acc = one, then for every w-bit window from the
//               top: w squarings (none in the top window) and one multiplication per term by table[index][digit]; then
//               the conversion out of the domain to a canonical residue in [0, M).
//
// Digit 0 multiplies by one and padding terms carry weight 0: every group of a wavefront executes the same number of
// windows and terms, so control flow is wave-uniform; only the table ADDRESS depends on the weights.  The width of the
// weights (wwords, nwin) is an argument of its own and is not tied to bits(M).  Terms may be of unequal LENGTH — the
// products of the range proofs pair a long exponent with a short one —: term_bits[t], a property of the launch and not of
// a row, bounds the weights of term t, and the windows above it skip that term's multiplication (by one) for every row
// alike.  The entry of term 0 is requested before the squarings of its window and used after them, as powmod_kernel does:
// callers put the longest term first.
//
// Table layout: entry (input i, digit d) is L * K contiguous words, word (j * K + p) for limb j of lane p: one group
// reads one contiguous span of K L words, lane-consecutive.  With shared bases (every row indexes the same few inputs)
// all groups read the same entries from L2; with per-row bases each reads its own.
#pragma once
#include "mx_mont.hpp"

namespace mx {

struct MultiexpArgs {
  const u32* inputs;    // [n_inputs][limbs] (table pass): any value below R; residues < M in practice
  u32* tables;          // [n_inputs][1 << window][L][K] (workspace)
  const u32* mod;       // [limbs] M
  const u32* rmodn;     // [limbs] R mod M, the domain's one
  const int* index;     // [rows][terms] input of every term
  const u32* weights;   // [rows][terms][wwords] little-endian words of the non-negative weight
  const int* term_bits; // [terms] bits the weights of term t can have, <= 32 * wwords: windows above them are skipped
  u32* out;             // [rows][limbs]
  i64 n_inputs, rows;
  int terms, wwords, nwin, window;
  int limbs, nblk;
};

template <int K, int L, int W>
__global__ void __launch_bounds__(64) multiexp_table_kernel(MultiexpArgs A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const bool valid = raw < A.n_inputs;
  const i64 e = valid ? raw : A.n_inputs - 1;       // surplus groups redo the last input and store nothing
  M_t M;
  M.init(smem + gw * M_t::LDS_WORDS, A.nblk);
  M.load(M.n, A.mod, A.limbs);
  M.setup_modulus();
  u32 one_m[L], x[L], y[L];
  M.load(one_m, A.rmodn, A.limbs);
  M.compute_r2(y, one_m);
  M.load(x, A.inputs + e * A.limbs, A.limbs);
  M.mul(x, x, y);                                   // x R mod M (lazy)
  const int entries = 1 << A.window;
  const i64 entry_words = (i64)L * K;
  u32* tab = A.tables + e * entries * entry_words + M.p;
  auto put = [&](int d, const u32 (&a)[L]) {
    if (!valid) return;
    u32* dst = tab + d * entry_words;
#pragma unroll
    for (int j = 0; j < L; ++j) dst[j * K] = a[j];
  };
  put(0, one_m);
  put(1, x);
#pragma unroll
  for (int j = 0; j < L; ++j) y[j] = x[j];
  for (int d = 2; d < entries; ++d) {               // x^d = x^(d-1) * x
    M.mul(y, y, x);
    put(d, y);
  }
}

// digit `win` (bits [win * window, (win + 1) * window)) of a little-endian weight of `wwords` words; a digit may
// straddle two words (windows that do not divide 32) and the top one may reach beyond the last word (zeros)
__device__ __forceinline__ u32 multiexp_mod_digit(const u32* w, int wwords, int win, int window) {
  const int bit = win * window, wi = bit >> 5, off = bit & 31;
  const u64 lo = wi < wwords ? w[wi] : 0u;
  const u64 hi = wi + 1 < wwords ? w[wi + 1] : 0u;
  return (u32)((lo | (hi << 32)) >> off) & ((1u << window) - 1u);
}

template <int K, int L, int W>
__global__ void __launch_bounds__(64) multiexp_kernel(MultiexpArgs A) {
  using M_t = Mont<K, L, W, true>;
  constexpr int GPW = 64 / K;
  extern __shared__ u32 smem[];
  const int gw = threadIdx.x / K;
  const i64 raw = (i64)blockIdx.x * GPW + gw;
  const bool valid = raw < A.rows;
  const i64 r = valid ? raw : A.rows - 1;           // surplus groups redo the last row and store nothing
  M_t M;
  M.init(smem + gw * M_t::LDS_WORDS, A.nblk);
  M.load(M.n, A.mod, A.limbs);
  M.setup_modulus();
  u32 acc[L];
  M.load(acc, A.rmodn, A.limbs);                    // the domain's one
  const i64 entry_words = (i64)L * K;
  const i64 input_words = entry_words << A.window;
  const u32* tab = A.tables + M.p;
  const int* idx_row = A.index + r * A.terms;
  const u32* w_row = A.weights + r * A.terms * A.wwords;
  auto entry = [&](u32 (&y)[L], int t, int win) {
    int i = idx_row[t];
    i = i < 0 ? 0 : (i >= A.n_inputs ? (int)A.n_inputs - 1 : i);
    const u32 d = multiexp_mod_digit(w_row + (i64)t * A.wwords, A.wwords, win, A.window);
    const u32* f = tab + (i64)i * input_words + (i64)d * entry_words;
#pragma unroll
    for (int j = 0; j < L; ++j) y[j] = f[j * K];
  };
  for (int win = A.nwin - 1; win >= 0; --win) {
    const int low = win * A.window;                 // the window's lowest bit: term t takes part iff low < term_bits[t]
    const bool first = low < A.term_bits[0];
    u32 y[L];
    if (first) entry(y, 0, win);                    // issued early, used after the squarings
    if (win != A.nwin - 1)
      for (int s = 0; s < A.window; ++s) M.sqr(acc, acc);
    if (first) M.mul(acc, acc, y);
    for (int t = 1; t < A.terms; ++t) {
      if (low >= A.term_bits[t]) continue;
      entry(y, t, win);
      M.mul(acc, acc, y);
    }
  }
  u32 res[L];
  M.from_mont_canonical(res, acc);
  M.store(A.out + r * A.limbs, A.limbs, res, valid);
}

}  // namespace mx
