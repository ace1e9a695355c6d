// Two-wavefront instantiations of the N^2-modulus pair kernel (mx_powmod_n2_split.hpp) for the wide geometry
// (18 limbs per lane; translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_powmod_n2_split.hpp"

namespace mxs {
template <int K, bool TS>
static int launch_form(const mx::PowmodN2Args& a, int64_t nblocks, hipStream_t s) {
  size_t lds = mx::powmod_n2_split_lds_bytes<K, LIMBS_PER_LANE_WIDE>();
  if (lds > 64 * 1024) {     // above the default limit of dynamic LDS per workgroup: opt in once per instance and device
    static bool allowed[MX_MAX_DEVICES] = {};
    MX_HIP(mx_allow_dynamic_lds(reinterpret_cast<const void*>(&mx::powmod_n2_split_kernel<K, LIMBS_PER_LANE_WIDE, LIMB_BITS, TS>), (int)lds, allowed));
  }
  return mx_launch(mx::powmod_n2_split_kernel<K, LIMBS_PER_LANE_WIDE, LIMB_BITS, TS>, nblocks, 64 * 2 * mx::N2_SPLIT_PAIRS, lds, s, a);
}

// Time-sliced instances at 18 limbs per lane: groups of 4 and 8 lanes (key_length 2048 and 4096), one resident
// workgroup per CU.  (Rounds 3 and 4 did not build them: first the unit loop pushed them over 256 registers, then — at
// 239 registers, no scratch — they lost to the 9-limb form, 45.0-47.6 against 42.9 ms for 10 000 ciphertexts.  That was
// the FIFO unit queue, not the instances: mx_powmod_n2_split.hpp, tools/ts_schedule_model.py.)
int launch_n2_split_wide(int K, bool ts, const mx::PowmodN2Args& a, int64_t nblocks, hipStream_t s) {
  return mx_dispatch_lanes<1, 2, 4, 8, 16>(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    if constexpr (KK == 4 || KK == 8) {
      if (ts) return launch_form<KK, true>(a, nblocks, s);
    } else {
      if (ts) return MX_ERR_SIZE;
    }
    return launch_form<KK, false>(a, nblocks, s);
  });
}
}  // namespace mxs
