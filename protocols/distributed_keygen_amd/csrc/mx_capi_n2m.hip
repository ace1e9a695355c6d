// Instantiations of the multi-exponentiation kernels modulo N^2 (mx_multiexp_n2.hpp) for the narrow geometry, every
// group width of the pair kernel (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_multiexp_n2.hpp"

namespace mxm {
int launch_multiexp(int K, bool table, const mx::MultiexpN2Args& a, int64_t nblocks, hipStream_t s) {
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32>(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    const size_t lds = mx::multiexp_n2_lds_bytes<KK, LIMBS_PER_LANE>();
    return table ? mx_launch(mx::multiexp_n2_table_kernel<KK, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a)
                 : mx_launch(mx::multiexp_n2_kernel<KK, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a);
  });
}
}  // namespace mxm
