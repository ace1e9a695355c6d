// Instantiations of the fixed-base kernels modulo N^2 (mx_fixedbase_n2.hpp) for the narrow geometry, every group width
// of the pair kernel (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_fixedbase_n2.hpp"

namespace mxf {
// pass 0: chain, 1: fill, 2: run
int launch_fixedbase(int K, int pass, const mx::FixedBaseN2Args& a, int64_t nblocks, hipStream_t s) {
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32>(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    const size_t lds = mx::fixedbase_n2_lds_bytes<KK, LIMBS_PER_LANE>();
    if (pass == 0) return mx_launch(mx::fixedbase_n2_chain_kernel<KK, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a);
    if (pass == 1) return mx_launch(mx::fixedbase_n2_fill_kernel<KK, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a);
    return mx_launch(mx::fixedbase_n2_run_kernel<KK, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a);
  });
}
}  // namespace mxf
