// mx_crt_enc_* / mx_crt_prime_split_run / mx_crt_lift_run: private-key (CRT) Paillier encryption around the half-size
// modexps — the reduction of a randomness row modulo p and q and the lift of the noise (rho_p, rho_q), with the message or a
// ciphertext folded in, to a ciphertext modulo N^2 (mx_crt_enc.hpp) — behind the C ABI (translation unit of its own, built
// in parallel with the others).  The modexps themselves are mx_powmod_shared_lpl modulo p and q and mx_powmod_nsquare_run
// with (n, exp) = (p, p) and (q, q).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_crt_enc.hpp"
#include "mx_crt_host.hpp"

namespace {

// The two lane geometries of a plan (tools/crt_model.py: CrtEncPlan): the prime split's radix covers half a randomness row
// as well as the longer prime; the lift's groups hold a half, its radix R covers the longer prime's square.
struct CrtEncShape {
  Geometry split, lift;
  int split_bit = 0;
};

int crt_enc_shape(int p_bits, int q_bits, int limbs_r, int limbs_half, int limbs_n, CrtEncShape& sh) {
  const int prime_bits = std::max(p_bits, q_bits);
  if (limbs_r > (MAX_MOD_BITS >> 4)) return MX_ERR_SIZE;
  sh.split_bit = 16 * limbs_r;
  if (!choose_geometry(std::max(prime_bits, sh.split_bit), sh.split)) return MX_ERR_SIZE;
  if (!choose_geometry(2 * prime_bits, sh.lift)) return MX_ERR_SIZE;
  // a row is staged in the group's LDS scratch (Mont::LDS_WORDS, of which limbs_of_bits reads all but the last two words)
  if (limbs_r > 2 * sh.split.K * sh.split.L + 6 || (prime_bits + 31) / 32 > 2 * sh.split.K * sh.split.L + 6) return MX_ERR_SIZE;
  if (std::max(limbs_half, limbs_n) > 2 * sh.lift.K * sh.lift.L + 6) return MX_ERR_SIZE;
  return MX_OK;
}

}  // namespace

extern "C" int64_t mx_crt_enc_plan_bytes(int limbs, int limbs_r) {
  if (limbs <= 0 || limbs_r <= 0) return MX_ERR_ARG;
  return align256((int64_t)mx::ENC_ROWS * 2 * limbs * 4);
}

extern "C" int mx_crt_enc_prepare(mx_crt_enc_plan* plan, const uint32_t* h_p, const uint32_t* h_q, const uint32_t* h_p2inv,
                                  int limbs, int limbs_r, void* d_plan, int64_t plan_bytes, void* stream) {
  if (!plan || !h_p || !h_q || !h_p2inv || !d_plan) return MX_ERR_ARG;
  if (limbs <= 0 || limbs_r <= 0) return MX_ERR_ARG;
  CrtKey key;
  MX_TRY(crt_key(key, h_p, h_q, limbs));
  const int rw = key.rw;
  CrtEncShape sh;
  MX_TRY(crt_enc_shape(key.p_bits, key.q_bits, limbs_r, rw, key.limbs_n, sh));
  if (mx_crt_enc_plan_bytes(limbs, limbs_r) > plan_bytes) return MX_ERR_WORKSPACE;

  std::vector<u32> c((size_t)mx::ENC_ROWS * rw, 0u);
  auto row = [&](int r) { return &c[(size_t)r * rw]; };
  const int lw = std::min(limbs, rw);
  const int rp = sh.split.W * sh.split.L * sh.split.nblk;
  const int r2 = sh.lift.W * sh.lift.L * sh.lift.nblk;
  const u32* primes[2] = {h_p, h_q};
  const std::vector<u32>* squares[2] = {&key.p2, &key.q2};
  for (int half = 0; half < 2; ++half) {
    const int r0 = mx::ENC_ROW_PSPLIT + 3 * half;
    std::memcpy(row(r0), primes[half], (size_t)lw * 4);
    two_pow_mod(row(r0 + 1), primes[half], lw, sh.split_bit + rp);
    two_pow_mod(row(r0 + 2), primes[half], lw, 2 * rp);
    // N, the squares and the inverse are below the larger square: rw words hold each of them
    const int s0 = half ? mx::ENC_ROW_Q : mx::ENC_ROW_P;
    const u32* sq = squares[half]->data();
    std::memcpy(row(s0), sq, (size_t)rw * 4);
    scaled_residue(row(s0 + 1), key.n.data(), sq, rw, 2 * r2);
    two_pow_mod(row(s0 + 2), sq, rw, r2);
    two_pow_mod(row(s0 + 3), sq, rw, 2 * r2);
  }
  scaled_residue(row(mx::ENC_ROW_Q + 4), h_p2inv, key.q2.data(), rw, r2);
  MX_TRY(upload_words(d_plan, c.data(), c.size(), (hipStream_t)stream));
  plan->d_plan = d_plan;
  plan->plan_bytes = plan_bytes;
  plan->limbs = limbs;
  plan->limbs_r = limbs_r;
  plan->limbs2 = key.limbs_n2();
  plan->limbs_half = rw;
  plan->limbs_n = key.limbs_n;
  plan->p_bits = key.p_bits;
  plan->q_bits = key.q_bits;
  return MX_OK;
}

extern "C" int mx_crt_prime_split_run(const mx_crt_enc_plan* plan, const uint32_t* d_rows, uint32_t* d_out, int64_t batch,
                                      void* stream) {
  if (!plan || !plan->d_plan || !d_rows || !d_out || batch <= 0) return MX_ERR_ARG;
  CrtEncShape sh;
  MX_TRY(crt_enc_shape(plan->p_bits, plan->q_bits, plan->limbs_r, plan->limbs_half, plan->limbs_n, sh));
  mx::CrtSplitArgs a;
  a.cts = d_rows; a.out = d_out; a.plan = (const u32*)plan->d_plan + (size_t)mx::ENC_ROW_PSPLIT * plan->limbs_half;
  a.batch = batch; a.limbs2 = plan->limbs_r; a.rw = plan->limbs_half; a.nblk = sh.split.nblk; a.split_bit = sh.split_bit;
  return launch_crt_split(a, sh.split.K, (hipStream_t)stream);
}

extern "C" int mx_crt_lift_run(const mx_crt_enc_plan* plan, const uint32_t* d_rho_p, const uint32_t* d_rho_q,
                               const uint32_t* d_messages, int message_stride, const uint32_t* d_halves, uint32_t* d_out,
                               int out_stride, uint8_t* d_status, int64_t batch, void* stream) {
  if (!plan || !plan->d_plan || !d_rho_p || !d_rho_q || !d_out || batch <= 0) return MX_ERR_ARG;
  if (d_messages && d_halves) return MX_ERR_ARG;
  if (d_messages && message_stride < plan->limbs_n) return MX_ERR_ARG;       // message rows narrower than N
  if (out_stride < plan->limbs2) return MX_ERR_ARG;
  if (!d_status && out_stride == plan->limbs2) return MX_ERR_ARG;            // the status must go somewhere
  CrtEncShape sh;
  MX_TRY(crt_enc_shape(plan->p_bits, plan->q_bits, plan->limbs_r, plan->limbs_half, plan->limbs_n, sh));
  if (crt_blocks(batch, sh.lift.K) > 0x7FFFFFFF) return MX_ERR_SIZE;
  mx::CrtLiftArgs a;
  a.rho_p = d_rho_p; a.rho_q = d_rho_q; a.out = d_out; a.status = d_status; a.plan = (const u32*)plan->d_plan;
  a.batch = batch; a.limbs2 = plan->limbs2; a.rw = plan->limbs_half; a.out_stride = out_stride; a.nblk = sh.lift.nblk;
  a.mode = d_messages ? mx::LIFT_MESSAGE : d_halves ? mx::LIFT_HALVES : mx::LIFT_NOISE;
  a.factor = d_messages ? d_messages : d_halves;
  a.factor_stride = d_messages ? message_stride : plan->limbs_half;
  a.factor_words = d_messages ? plan->limbs_n : plan->limbs_half;
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(sh.lift.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    using M_t = mx::Mont<K, LIMBS_PER_LANE, LIMB_BITS, true>;
    // the Montgomery scratch of every group, then every group's wide row of the last product (mx_crt_enc.hpp: WIDE_WORDS)
    const size_t lds = (size_t)(64 / K) * (M_t::LDS_WORDS + 2 * K * LIMBS_PER_LANE + 8) * 4;
    return mx_launch(mx::crt_lift_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, crt_blocks(batch, K), 64, lds, (hipStream_t)stream, a);
  });
}
