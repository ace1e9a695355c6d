// Instantiations of the shared-weight product kernel modulo N^2 (mx_matmul_n2.hpp: matrix products and convolutions)
// for the narrow geometry, every group width of the pair kernel (translation unit of its own, built in parallel with
// the others).  Its table pass is the one of mx_capi_n2m.hip.
#include "mx_upload.hpp"
#include "mx_matmul_n2.hpp"

namespace mxmm {
template <int K>
static int launch_k(const mx::SharedN2Args& a, int64_t nblocks, hipStream_t s) {
  const size_t lds = mx::multiexp_n2_lds_bytes<K, LIMBS_PER_LANE>();
  hipLaunchKernelGGL((mx::shared_n2_kernel<K, LIMBS_PER_LANE, LIMB_BITS>), dim3((unsigned)nblocks), dim3(64), lds, s, a);
  MX_HIP(hipGetLastError());
  return MX_OK;
}

int launch_shared(int K, const mx::SharedN2Args& a, int64_t nblocks, hipStream_t s) {
  switch (K) {
    case 1: return launch_k<1>(a, nblocks, s);
    case 2: return launch_k<2>(a, nblocks, s);
    case 4: return launch_k<4>(a, nblocks, s);
    case 8: return launch_k<8>(a, nblocks, s);
    case 16: return launch_k<16>(a, nblocks, s);
    case 32: return launch_k<32>(a, nblocks, s);
  }
  return MX_ERR_SIZE;
}
}  // namespace mxmm
