// Host helpers shared by the translation units of the private-key (CRT) entry points (mx_capi_crt.hip, mx_capi_crt_enc.hip).
#pragma once
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_crt.hpp"

namespace {

bool same_words(const u32* a, const u32* b, int limbs) {
  for (int i = 0; i < limbs; ++i) if (a[i] != b[i]) return false;
  return true;
}

// What both prepare calls derive from the primes: p^2, q^2 and N in 2 limbs words each, N^2 in 4 limbs, the words rw of the
// larger square and those of N.
struct CrtKey {
  int p_bits = 0, q_bits = 0, sq_words = 0, rw = 0, limbs_n = 0;
  std::vector<u32> p2, q2, n, n2;
  int limbs_n2() const { return (bit_length(n2.data(), 2 * sq_words) + 31) / 32; }
};

// MX_ERR_MODULUS for an even prime or one below 2, MX_ERR_ARG for p == q
int crt_key(CrtKey& k, const u32* h_p, const u32* h_q, int limbs) {
  if (!(h_p[0] & 1u) || !(h_q[0] & 1u)) return MX_ERR_MODULUS;
  k.p_bits = bit_length(h_p, limbs);
  k.q_bits = bit_length(h_q, limbs);
  if (k.p_bits < 2 || k.q_bits < 2) return MX_ERR_MODULUS;
  if (same_words(h_p, h_q, limbs)) return MX_ERR_ARG;
  k.sq_words = 2 * limbs;
  k.p2.resize(k.sq_words); k.q2.resize(k.sq_words); k.n.resize(k.sq_words); k.n2.resize(2 * k.sq_words);
  mul_words(k.p2.data(), h_p, limbs, h_p, limbs);
  mul_words(k.q2.data(), h_q, limbs, h_q, limbs);
  mul_words(k.n.data(), h_p, limbs, h_q, limbs);
  mul_words(k.n2.data(), k.n.data(), k.sq_words, k.n.data(), k.sq_words);
  k.rw = (std::max(bit_length(k.p2.data(), k.sq_words), bit_length(k.q2.data(), k.sq_words)) + 31) / 32;
  k.limbs_n = (bit_length(k.n.data(), k.sq_words) + 31) / 32;
  return MX_OK;
}

// v 2^m mod r for any v of `limbs` words, as a row of rw words at dst (r has at most rw words)
void scaled_residue(u32* dst, const u32* v, const u32* r, int limbs, int m) {
  std::vector<u32> q(limbs), t(limbs + 1, 0u);
  divmod_words(q.data(), t.data(), v, limbs, r, limbs);
  shl_mod(t, r, limbs, m);
  std::memcpy(dst, t.data(), (size_t)limbs * 4);
}

int64_t crt_blocks(int64_t batch, int K) { return (batch + 64 / K - 1) / (64 / K); }

// crt_split_kernel over groups of K lanes: the rows of a.cts modulo the two moduli of a.plan
int launch_crt_split(const mx::CrtSplitArgs& a, int K, hipStream_t s) {
  if (crt_blocks(a.batch, K) > 0x7FFFFFFF) return MX_ERR_SIZE;
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(K, [&](auto k) {
    constexpr int Kc = decltype(k)::value;
    using M_t = mx::Mont<Kc, LIMBS_PER_LANE, LIMB_BITS, true>;
    const size_t lds = (size_t)(64 / Kc) * M_t::LDS_WORDS * 4;
    return mx_launch(mx::crt_split_kernel<Kc, LIMBS_PER_LANE, LIMB_BITS>, crt_blocks(a.batch, Kc), 64, lds, s, a);
  });
}

}  // namespace
