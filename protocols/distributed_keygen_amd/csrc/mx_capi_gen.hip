// mx_generator_shares / mx_generator_sum: the jointly random generators of the biprimality test, drawn shares reduced
// and summed modulo one candidate modulus per group (mx_generators.hpp), behind the C ABI (translation unit of its own,
// built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_generators.hpp"

namespace {

// What both entry points refuse, in the order the header states; then the geometry of the launch.
int generator_check(const void* d_rows, const void* d_out, const uint32_t* d_mods, const uint32_t* h_mods, int limbs, int mod_bits,
                    int words, int64_t groups, int64_t group_size, const void* d_ws, int64_t ws_bytes, Geometry& geo) {
  if (!d_rows || !d_out || !d_mods || !d_ws || limbs < 1 || groups < 0 || group_size < 0) return MX_ERR_ARG;
  if (mod_bits < 2 || mod_bits > 32 * (int64_t)limbs) return MX_ERR_ARG;
  if (h_mods) {
    for (int64_t g = 0; g < groups; ++g) {
      const u32* n = h_mods + g * limbs;
      const int b = bit_length(n, limbs);
      if (!(n[0] & 1u) || b < 2 || b > mod_bits) return MX_ERR_MODULUS;
    }
  }
  if (!choose_geometry(mod_bits, geo)) return MX_ERR_SIZE;
  // a row is staged in the group's LDS scratch, and its piece above the split must be a Montgomery operand (below R)
  const int lds_words = 2 * geo.K * geo.L + 8;
  if (words > lds_words - 2 || 32 * (int64_t)words - (mod_bits - 1) + 5 > (int64_t)geo.W * geo.L * geo.nblk) return MX_ERR_SIZE;
  const int gpw = 64 / geo.K;
  if (groups > 0 && group_size > 0 && (groups > INT64_MAX / group_size || (groups * group_size + gpw - 1) / gpw > 0x7FFFFFFF))
    return MX_ERR_SIZE;
  if (mx_generator_workspace_bytes(limbs, groups) > ws_bytes) return MX_ERR_WORKSPACE;
  return MX_OK;
}

// The setup launch (R^2 mod N_c into the workspace) and the launch of `share` or `sum` over parties * batch rows.
int generator_launch(bool sum, const uint32_t* d_rows, int parties, int words, uint32_t* d_out, const uint32_t* d_mods, int limbs,
                     int mod_bits, int64_t groups, int64_t group_size, void* d_ws, const Geometry& geo, hipStream_t s) {
  mx::GeneratorSetupArgs u;
  u.mods = d_mods; u.r2 = (u32*)d_ws; u.groups = groups; u.limbs = limbs; u.nblk = geo.nblk;
  mx::GeneratorArgs a;
  a.rows = d_rows; a.out = d_out; a.mods = d_mods; a.r2 = (const u32*)d_ws;
  a.batch = groups * group_size; a.group_size = group_size;
  a.limbs = limbs; a.nblk = geo.nblk; a.words = words; a.split_bit = mod_bits - 1; a.parties = parties;
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(geo.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    using M_t = mx::Mont<K, LIMBS_PER_LANE, LIMB_BITS, true>;
    const int gpw = 64 / K;
    const size_t lds = (size_t)gpw * M_t::LDS_WORDS * 4;
    MX_TRY(mx_launch(mx::generator_setup_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, (groups + gpw - 1) / gpw, 64, lds, s, u));
    const int64_t nblocks = (a.batch + gpw - 1) / gpw;
    return sum ? mx_launch(mx::generator_sum_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a)
               : mx_launch(mx::generator_share_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a);
  });
}

}  // namespace

extern "C" int64_t mx_generator_workspace_bytes(int limbs, int64_t groups) {
  if (limbs < 1 || groups < 0) return MX_ERR_ARG;
  return align256(groups * limbs * 4);
}

extern "C" int mx_generator_shares(const uint32_t* d_draws, uint32_t* d_out, const uint32_t* d_mods, const uint32_t* h_mods,
                                   int limbs, int mod_bits, int64_t groups, int64_t group_size, void* d_ws, int64_t ws_bytes,
                                   void* stream) {
  Geometry geo;
  const int cw = mod_bits >= 2 ? (int)(((int64_t)mod_bits + 64 + 31) / 32) : 0;
  MX_TRY(generator_check(d_draws, d_out, d_mods, h_mods, limbs, mod_bits, cw, groups, group_size, d_ws, ws_bytes, geo));
  if (groups == 0 || group_size == 0) return MX_OK;
  return generator_launch(false, d_draws, 1, cw, d_out, d_mods, limbs, mod_bits, groups, group_size, d_ws, geo, (hipStream_t)stream);
}

extern "C" int mx_generator_sum(const uint32_t* d_shares, int n_parties, uint32_t* d_out, const uint32_t* d_mods,
                                const uint32_t* h_mods, int limbs, int mod_bits, int64_t groups, int64_t group_size, void* d_ws,
                                int64_t ws_bytes, void* stream) {
  if (n_parties < 1 || n_parties > MX_GEN_MAX_PARTIES) return MX_ERR_ARG;
  Geometry geo;
  MX_TRY(generator_check(d_shares, d_out, d_mods, h_mods, limbs, mod_bits, limbs, groups, group_size, d_ws, ws_bytes, geo));
  if (groups == 0 || group_size == 0) return MX_OK;
  return generator_launch(true, d_shares, n_parties, limbs, d_out, d_mods, limbs, mod_bits, groups, group_size, d_ws, geo, (hipStream_t)stream);
}
