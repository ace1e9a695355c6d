// Instantiations of the histogram kernels modulo N^2 (mx_hist_n2.hpp) for the narrow geometry, every group width of the
// pair kernel (translation unit of its own, built in parallel with the others).
#include "mx_upload.hpp"
#include "mx_hist_n2.hpp"

namespace mxh {
template <int K>
static int launch_k(bool convert, const mx::HistN2Args& a, int64_t nblocks, hipStream_t s) {
  const size_t lds = mx::hist_n2_lds_bytes<K, LIMBS_PER_LANE>();
  if (convert) {
    hipLaunchKernelGGL((mx::hist_n2_convert_kernel<K, LIMBS_PER_LANE, LIMB_BITS>), dim3((unsigned)nblocks), dim3(64), lds, s, a);
  } else {
    hipLaunchKernelGGL((mx::hist_n2_kernel<K, LIMBS_PER_LANE, LIMB_BITS>), dim3((unsigned)nblocks), dim3(64), lds, s, a);
  }
  MX_HIP(hipGetLastError());
  return MX_OK;
}

int launch_hist(int K, bool convert, const mx::HistN2Args& a, int64_t nblocks, hipStream_t s) {
  switch (K) {
    case 1: return launch_k<1>(convert, a, nblocks, s);
    case 2: return launch_k<2>(convert, a, nblocks, s);
    case 4: return launch_k<4>(convert, a, nblocks, s);
    case 8: return launch_k<8>(convert, a, nblocks, s);
    case 16: return launch_k<16>(convert, a, nblocks, s);
    case 32: return launch_k<32>(convert, a, nblocks, s);
  }
  return MX_ERR_SIZE;
}
}  // namespace mxh
