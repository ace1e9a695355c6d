// Instantiations of the packing kernel modulo N^2 (mx_pack_n2.hpp) for the narrow geometry, every group width of the
// pair kernel (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_pack_n2.hpp"

namespace mxp {
int launch_pack(int K, const mx::PackN2Args& a, int64_t nblocks, hipStream_t s) {
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32>(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    return mx_launch(mx::pack_n2_kernel<KK, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, mx::pack_n2_lds_bytes<KK, LIMBS_PER_LANE>(), s, a);
  });
}
}  // namespace mxp
