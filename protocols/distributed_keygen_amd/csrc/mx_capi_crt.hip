// mx_crt_*: private-key (CRT) Paillier decryption around two half-size modexps — the reduction of a ciphertext modulo p^2
// and q^2 and the recombination of the two results (mx_crt.hpp) — behind the C ABI (translation unit of its own, built in
// parallel with the others).  The modexps themselves are mx_powmod_nsquare_run with (n, exp) = (p, p - 1) and (q, q - 1).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_crt.hpp"
#include "mx_crt_host.hpp"

namespace {

// The two lane geometries of a plan (tools/crt_model.py: CrtPlan): the split's radix covers half a row as well as the
// longer prime's square; the recombination's groups hold a half-width number, its radix R1 covers the longer prime.
struct CrtShape {
  Geometry split, recombine;
  int split_bit = 0, nblk1 = 0;
};

int crt_shape(int p_bits, int q_bits, int limbs2, int limbs_half, CrtShape& sh) {
  const int prime_bits = std::max(p_bits, q_bits);
  if (limbs2 > (MAX_MOD_BITS >> 4)) return MX_ERR_SIZE;
  sh.split_bit = 16 * limbs2;
  if (!choose_geometry(std::max(2 * prime_bits, sh.split_bit), sh.split)) return MX_ERR_SIZE;
  if (!choose_geometry(2 * prime_bits, sh.recombine)) return MX_ERR_SIZE;
  sh.nblk1 = (prime_bits + 4 + sh.recombine.W * sh.recombine.L - 1) / (sh.recombine.W * sh.recombine.L);
  // a row is staged in the group's LDS scratch (Mont::LDS_WORDS, of which limbs_of_bits reads all but the last two words)
  if (limbs2 > 2 * sh.split.K * sh.split.L + 6 || limbs_half > 2 * sh.recombine.K * sh.recombine.L + 6) return MX_ERR_SIZE;
  return MX_OK;
}

}  // namespace

extern "C" int64_t mx_crt_plan_bytes(int limbs, int limbs2) {
  if (limbs <= 0 || limbs2 <= 0) return MX_ERR_ARG;
  return align256((int64_t)mx::CRT_ROWS * 2 * limbs * 4);
}

extern "C" int mx_crt_prepare(mx_crt_plan* plan, const uint32_t* h_p, const uint32_t* h_q, const uint32_t* h_hp,
                              const uint32_t* h_hq, const uint32_t* h_pinv, int limbs, int limbs2, void* d_plan,
                              int64_t plan_bytes, void* stream) {
  if (!plan || !h_p || !h_q || !h_hp || !h_hq || !h_pinv || !d_plan) return MX_ERR_ARG;
  if (limbs <= 0 || limbs2 <= 0) return MX_ERR_ARG;
  CrtKey key;
  MX_TRY(crt_key(key, h_p, h_q, limbs));
  if (key.limbs_n2() > limbs2) return MX_ERR_ARG;      // rows too narrow for N^2
  const int rw = key.rw;
  CrtShape sh;
  MX_TRY(crt_shape(key.p_bits, key.q_bits, limbs2, rw, sh));
  if (mx_crt_plan_bytes(limbs, limbs2) > plan_bytes) return MX_ERR_WORKSPACE;

  std::vector<u32> c((size_t)mx::CRT_ROWS * rw, 0u);
  auto row = [&](int r) { return &c[(size_t)r * rw]; };
  const int rs = sh.split.W * sh.split.L * sh.split.nblk;
  const int r1 = sh.recombine.W * sh.recombine.L * sh.nblk1;
  const std::vector<u32>* squares[2] = {&key.p2, &key.q2};
  for (int half = 0; half < 2; ++half) {
    const u32* sq = squares[half]->data();            // zero above its own words: rw words of it are the modulus
    std::vector<u32> m(sq, sq + rw);
    std::memcpy(row(mx::CRT_ROW_SPLIT + 3 * half), m.data(), (size_t)rw * 4);
    two_pow_mod(row(mx::CRT_ROW_SPLIT + 3 * half + 1), m.data(), rw, sh.split_bit + rs);
    two_pow_mod(row(mx::CRT_ROW_SPLIT + 3 * half + 2), m.data(), rw, 2 * rs);
  }
  std::memcpy(row(mx::CRT_ROW_P), h_p, (size_t)std::min(limbs, rw) * 4);
  scaled_residue(row(mx::CRT_ROW_P + 1), h_hp, h_p, std::min(limbs, rw), r1);
  std::memcpy(row(mx::CRT_ROW_Q), h_q, (size_t)std::min(limbs, rw) * 4);
  scaled_residue(row(mx::CRT_ROW_Q + 1), h_hq, h_q, std::min(limbs, rw), r1);
  two_pow_mod(row(mx::CRT_ROW_Q + 2), h_q, std::min(limbs, rw), r1);
  scaled_residue(row(mx::CRT_ROW_Q + 3), h_pinv, h_q, std::min(limbs, rw), r1);
  MX_TRY(upload_words(d_plan, c.data(), c.size(), (hipStream_t)stream));
  plan->d_plan = d_plan;
  plan->plan_bytes = plan_bytes;
  plan->limbs = limbs;
  plan->limbs2 = limbs2;
  plan->limbs_half = rw;
  plan->limbs_n = key.limbs_n;
  plan->p_bits = key.p_bits;
  plan->q_bits = key.q_bits;
  return MX_OK;
}

extern "C" int mx_crt_split_run(const mx_crt_plan* plan, const uint32_t* d_cts, uint32_t* d_out, int64_t batch, void* stream) {
  if (!plan || !plan->d_plan || !d_cts || !d_out || batch <= 0) return MX_ERR_ARG;
  CrtShape sh;
  MX_TRY(crt_shape(plan->p_bits, plan->q_bits, plan->limbs2, plan->limbs_half, sh));
  mx::CrtSplitArgs a;
  a.cts = d_cts; a.out = d_out; a.plan = (const u32*)plan->d_plan;
  a.batch = batch; a.limbs2 = plan->limbs2; a.rw = plan->limbs_half; a.nblk = sh.split.nblk; a.split_bit = sh.split_bit;
  return launch_crt_split(a, sh.split.K, (hipStream_t)stream);
}

extern "C" int mx_crt_recombine_run(const mx_crt_plan* plan, const uint32_t* d_xp, const uint32_t* d_xq, uint32_t* d_out,
                                    int out_stride, uint8_t* d_status, int64_t batch, void* stream) {
  if (!plan || !plan->d_plan || !d_xp || !d_xq || !d_out || batch <= 0) return MX_ERR_ARG;
  if (out_stride < plan->limbs_n) return MX_ERR_ARG;
  if (!d_status && out_stride == plan->limbs_n) return MX_ERR_ARG;      // the status must go somewhere
  CrtShape sh;
  MX_TRY(crt_shape(plan->p_bits, plan->q_bits, plan->limbs2, plan->limbs_half, sh));
  if (crt_blocks(batch, sh.recombine.K) > 0x7FFFFFFF) return MX_ERR_SIZE;
  mx::CrtRecombineArgs a;
  a.xp = d_xp; a.xq = d_xq; a.out = d_out; a.status = d_status; a.plan = (const u32*)plan->d_plan;
  a.batch = batch; a.limbs = plan->limbs_n; a.rw = plan->limbs_half; a.out_stride = out_stride; a.nblk1 = sh.nblk1;
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(sh.recombine.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    using M_t = mx::Mont<K, LIMBS_PER_LANE, LIMB_BITS, true>;
    // the Montgomery scratch of every group, then every group's wide row of the last product (mx_crt.hpp: WIDE_WORDS)
    const size_t lds = (size_t)(64 / K) * (M_t::LDS_WORDS + 2 * K * LIMBS_PER_LANE + 8) * 4;
    return mx_launch(mx::crt_recombine_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, crt_blocks(batch, K), 64, lds, (hipStream_t)stream, a);
  });
}
