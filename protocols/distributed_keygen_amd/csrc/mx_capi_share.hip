// mx_share_candidates / mx_shamir_share: additive shares of the prime candidates and their Shamir sharings
// (mx_share.hpp) behind the C ABI (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_share.hpp"

namespace {

// x <- (x + y) mod n for x, y < n (x has limbs + 1 words)
void add_mod(std::vector<u32>& x, const u32* y, const u32* n, int limbs) {
  u64 carry = 0;
  for (int i = 0; i < limbs; ++i) {
    u64 t = (u64)x[i] + y[i] + carry;
    x[i] = (u32)t;
    carry = t >> 32;
  }
  x[limbs] += (u32)carry;
  if (geq(x, n, limbs)) {
    u64 borrow = 0;
    for (int i = 0; i < limbs; ++i) {
      u64 d = (u64)x[i] - n[i] - borrow;
      x[i] = (u32)d;
      borrow = (d >> 63) & 1;
    }
    x[limbs] -= (u32)borrow;
  }
}

// out[0..limbs) = x * r mod n for a word-sized x and r < n: double-and-add from the top bit of x
void small_times_mod(u32* out, u32 x, const u32* r, const u32* n, int limbs) {
  std::vector<u32> acc(limbs + 1, 0u);
  for (int bit = 31; bit >= 0; --bit) {
    shl_mod(acc, n, limbs, 1);
    if ((x >> bit) & 1u) add_mod(acc, r, n, limbs);
  }
  for (int i = 0; i < limbs; ++i) out[i] = acc[i];
}

// Dynamic LDS of one workgroup: the Montgomery scratch of its 64 / K groups and their `degree` parked coefficients
template <int K>
int64_t share_lds_bytes(int degree) {
  using M_t = mx::Mont<K, LIMBS_PER_LANE, LIMB_BITS, true>;
  return (int64_t)(64 / K) * (M_t::LDS_WORDS + (int64_t)degree * M_t::S) * 4;
}

}  // namespace

extern "C" int mx_share_candidates(const uint32_t* d_random, uint32_t* d_out, int64_t count, int prime_length, int first_party,
                                   int row_words, void* stream) {
  if (!d_random || !d_out || count < 0 || prime_length < 8 || row_words < 1) return MX_ERR_ARG;
  if ((int64_t)prime_length > 32 * (int64_t)row_words) return MX_ERR_SIZE;
  if (count == 0) return MX_OK;
  mx::CandidateArgs a;
  a.random = d_random; a.out = d_out; a.count = count; a.prime_length = prime_length;
  a.in_words = (prime_length - 3 + 31) / 32; a.row_words = row_words; a.mod4 = first_party ? 3u : 0u;
  const int64_t nblocks = (count * row_words + mx::CANDIDATE_THREADS - 1) / mx::CANDIDATE_THREADS;
  if (nblocks > 0x7FFFFFFF) return MX_ERR_SIZE;
  return mx_launch(mx::share_candidates_kernel, nblocks, mx::CANDIDATE_THREADS, 0, (hipStream_t)stream, a);
}

extern "C" int64_t mx_share_workspace_bytes(int limbs, int n_points) {
  if (limbs <= 0 || n_points <= 0) return MX_ERR_ARG;
  return align256((int64_t)(3 + n_points) * limbs * 4);
}

extern "C" int mx_shamir_share(const uint32_t* d_secrets, const uint32_t* d_draws, const uint32_t* h_points, int n_points,
                               int degree, uint32_t* d_out, const uint32_t* h_mod, int limbs, int64_t batch, void* d_ws,
                               int64_t ws_bytes, void* stream) {
  if (!d_draws || !h_points || !d_out || !h_mod || !d_ws || limbs <= 0 || batch <= 0 || degree < 1 || n_points <= degree)
    return MX_ERR_ARG;
  for (int j = 0; j < n_points; ++j) {
    if (h_points[j] < 1 || h_points[j] > 0xFFFFu) return MX_ERR_ARG;
    for (int i = 0; i < j; ++i)
      if (h_points[i] == h_points[j]) return MX_ERR_ARG;
  }
  if (!(h_mod[0] & 1u)) return MX_ERR_MODULUS;
  const int bits = bit_length(h_mod, limbs);
  if (bits < 2) return MX_ERR_MODULUS;
  Geometry geo;
  if (!choose_geometry(bits, geo)) return MX_ERR_SIZE;
  if (degree > MX_SHARE_MAX_DEGREE) return MX_ERR_SIZE;
  if (align256((int64_t)(3 + n_points) * limbs * 4) > ws_bytes) return MX_ERR_WORKSPACE;
  // constants: P, R mod P, 2^s R mod P with s = bits - 1 (the split of a draw), x_j R mod P
  const int m = geo.W * geo.L * geo.nblk;
  std::vector<u32> c((size_t)(3 + n_points) * limbs);
  std::memcpy(c.data(), h_mod, (size_t)limbs * 4);
  two_pow_mod(c.data() + limbs, h_mod, limbs, m);
  two_pow_mod(c.data() + 2 * limbs, h_mod, limbs, m + bits - 1);
  for (int j = 0; j < n_points; ++j)
    small_times_mod(c.data() + (size_t)(3 + j) * limbs, h_points[j], c.data() + limbs, h_mod, limbs);
  hipStream_t s = (hipStream_t)stream;
  MX_TRY(upload_words(d_ws, c.data(), c.size(), s));
  mx::ShareArgs a;
  const u32* w = (const u32*)d_ws;
  a.secrets = d_secrets; a.draws = d_draws; a.out = d_out;
  a.mod = w; a.rmodn = w + limbs; a.split = w + 2 * limbs; a.xr = w + 3 * limbs;
  a.batch = batch; a.limbs = limbs; a.nblk = geo.nblk; a.degree = degree; a.n_points = n_points;
  a.cw = (bits + 64 + 31) / 32; a.split_bit = bits - 1;
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(geo.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    const int gpw = 64 / K;
    const int64_t nblocks = (a.batch + gpw - 1) / gpw;
    const int64_t lds = share_lds_bytes<K>(a.degree);
    if (lds > 65536 || nblocks > 0x7FFFFFFF) return MX_ERR_SIZE;
    return mx_launch(mx::shamir_share_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, (size_t)lds, s, a);
  });
}
