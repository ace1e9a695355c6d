// Instantiations of the shared-weight product kernel modulo N^2 (mx_matmul_n2.hpp: matrix products and convolutions)
// for the narrow geometry, every group width of the pair kernel (translation unit of its own, built in parallel with
// the others).  Its table pass is the one of mx_capi_n2m.hip.
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_matmul_n2.hpp"

namespace mxmm {
int launch_shared(int K, const mx::SharedN2Args& a, int64_t nblocks, hipStream_t s) {
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32>(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    return mx_launch(mx::shared_n2_kernel<KK, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, mx::multiexp_n2_lds_bytes<KK, LIMBS_PER_LANE>(), s, a);
  });
}
}  // namespace mxmm
