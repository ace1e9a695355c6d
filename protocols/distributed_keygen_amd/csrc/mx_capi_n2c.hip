// Instantiations of the prefix-product kernels modulo N^2 (mx_scan_n2.hpp) for the narrow geometry, every group width
// of the pair kernel (translation unit of its own, built in parallel with the others).
#include "mx_upload.hpp"
#include "mx_scan_n2.hpp"

namespace mxh {
template <int K>
static int launch_scan_k(bool store, const mx::ScanN2Args& a, int64_t nblocks, hipStream_t s) {
  const size_t lds = mx::hist_n2_lds_bytes<K, LIMBS_PER_LANE>();
  if (store) {
    hipLaunchKernelGGL((mx::scan_n2_store_kernel<K, LIMBS_PER_LANE, LIMB_BITS>), dim3((unsigned)nblocks), dim3(64), lds, s, a);
  } else {
    hipLaunchKernelGGL((mx::scan_n2_kernel<K, LIMBS_PER_LANE, LIMB_BITS>), dim3((unsigned)nblocks), dim3(64), lds, s, a);
  }
  MX_HIP(hipGetLastError());
  return MX_OK;
}

int launch_scan(int K, bool store, const mx::ScanN2Args& a, int64_t nblocks, hipStream_t s) {
  switch (K) {
    case 1: return launch_scan_k<1>(store, a, nblocks, s);
    case 2: return launch_scan_k<2>(store, a, nblocks, s);
    case 4: return launch_scan_k<4>(store, a, nblocks, s);
    case 8: return launch_scan_k<8>(store, a, nblocks, s);
    case 16: return launch_scan_k<16>(store, a, nblocks, s);
    case 32: return launch_scan_k<32>(store, a, nblocks, s);
  }
  return MX_ERR_SIZE;
}
}  // namespace mxh
