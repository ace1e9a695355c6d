// mx_mr_split / mx_mr_tail / mx_mr_base2: the strong-pseudoprime test over a batch of candidates (mx_mr.hpp), behind
// the C ABI (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_mr.hpp"

namespace {

// What the three entry points refuse, in the order the header states; then the geometry of the launch.
int mr_check(const uint32_t* h_cands, int limbs, int mod_bits, int64_t groups, int64_t group_size, Geometry& geo) {
  if (limbs < 1 || groups < 0 || group_size < 0) return MX_ERR_ARG;
  if (mod_bits < 2 || mod_bits > 32 * (int64_t)limbs) return MX_ERR_ARG;
  if (h_cands) {
    for (int64_t g = 0; g < groups; ++g) {
      const u32* n = h_cands + g * limbs;
      const int b = bit_length(n, limbs);
      if (!(n[0] & 1u) || b < 2 || b > mod_bits) return MX_ERR_MODULUS;
    }
  }
  if (!choose_geometry(mod_bits, geo)) return MX_ERR_SIZE;
  if (limbs > 2 * geo.K * geo.L + 8 - 2) return MX_ERR_SIZE;      // a row is staged in the group's LDS scratch
  const int gpw = 64 / geo.K;
  if (groups > 0 && group_size > 0 && (groups > INT64_MAX / group_size || (groups * group_size + gpw - 1) / gpw > 0x7FFFFFFF))
    return MX_ERR_SIZE;
  return MX_OK;
}

template <class F>
int mr_dispatch(const Geometry& geo, F&& f) {
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(geo.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    using M_t = mx::Mont<K, LIMBS_PER_LANE, LIMB_BITS, true>;
    return f(k, 64 / K, (size_t)(64 / K) * M_t::LDS_WORDS * 4);
  });
}

}  // namespace

extern "C" int mx_mr_split(const uint32_t* d_cands, const uint32_t* h_cands, uint32_t* d_d, int32_t* d_s, int limbs, int mod_bits,
                           int64_t groups, void* stream) {
  if (!d_cands || !d_d || !d_s) return MX_ERR_ARG;
  Geometry geo;
  MX_TRY(mr_check(h_cands, limbs, mod_bits, groups, 1, geo));
  if (groups == 0) return MX_OK;
  mx::MrSplitArgs a;
  a.cands = d_cands; a.d = d_d; a.s = d_s; a.groups = groups; a.limbs = limbs; a.nblk = geo.nblk;
  return mr_dispatch(geo, [&](auto k, int gpw, size_t lds) {
    constexpr int K = decltype(k)::value;
    return mx_launch(mx::mr_split_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, (groups + gpw - 1) / gpw, 64, lds, (hipStream_t)stream, a);
  });
}

extern "C" int mx_mr_tail(const uint32_t* d_x0, const uint32_t* d_bases, const int32_t* d_s, uint8_t* d_pass,
                          const uint32_t* d_cands, const uint32_t* h_cands, int limbs, int mod_bits, int64_t groups,
                          int64_t group_size, void* stream) {
  if (!d_x0 || !d_bases || !d_s || !d_pass || !d_cands) return MX_ERR_ARG;
  Geometry geo;
  MX_TRY(mr_check(h_cands, limbs, mod_bits, groups, group_size, geo));
  if (groups == 0 || group_size == 0) return MX_OK;
  mx::MrArgs a;
  a.cands = d_cands; a.x0 = d_x0; a.bases = d_bases; a.s = d_s; a.pass = d_pass;
  a.batch = groups * group_size; a.group_size = group_size; a.limbs = limbs; a.nblk = geo.nblk; a.mod_bits = mod_bits;
  return mr_dispatch(geo, [&](auto k, int gpw, size_t lds) {
    constexpr int K = decltype(k)::value;
    return mx_launch(mx::mr_tail_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, (a.batch + gpw - 1) / gpw, 64, lds, (hipStream_t)stream, a);
  });
}

extern "C" int mx_mr_base2(const uint32_t* d_cands, const uint32_t* h_cands, uint8_t* d_pass, int limbs, int mod_bits,
                           int64_t groups, void* stream) {
  if (!d_cands || !d_pass) return MX_ERR_ARG;
  Geometry geo;
  MX_TRY(mr_check(h_cands, limbs, mod_bits, groups, 1, geo));
  if (groups == 0) return MX_OK;
  mx::MrArgs a;
  a.cands = d_cands; a.x0 = nullptr; a.bases = nullptr; a.s = nullptr; a.pass = d_pass;
  a.batch = groups; a.group_size = 1; a.limbs = limbs; a.nblk = geo.nblk; a.mod_bits = mod_bits;
  return mr_dispatch(geo, [&](auto k, int gpw, size_t lds) {
    constexpr int K = decltype(k)::value;
    return mx_launch(mx::mr_base2_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, (groups + gpw - 1) / gpw, 64, lds, (hipStream_t)stream, a);
  });
}
