// Instantiations of the multi-exponentiation kernels modulo N^2 (mx_multiexp_n2.hpp) for the narrow geometry, every
// group width of the pair kernel (translation unit of its own, built in parallel with the others).
#include "mx_upload.hpp"
#include "mx_multiexp_n2.hpp"

namespace mxm {
template <int K>
static int launch_k(bool table, const mx::MultiexpN2Args& a, int64_t nblocks, hipStream_t s) {
  const size_t lds = mx::multiexp_n2_lds_bytes<K, LIMBS_PER_LANE>();
  if (table) {
    hipLaunchKernelGGL((mx::multiexp_n2_table_kernel<K, LIMBS_PER_LANE, LIMB_BITS>), dim3((unsigned)nblocks), dim3(64), lds, s, a);
  } else {
    hipLaunchKernelGGL((mx::multiexp_n2_kernel<K, LIMBS_PER_LANE, LIMB_BITS>), dim3((unsigned)nblocks), dim3(64), lds, s, a);
  }
  MX_HIP(hipGetLastError());
  return MX_OK;
}

int launch_multiexp(int K, bool table, const mx::MultiexpN2Args& a, int64_t nblocks, hipStream_t s) {
  switch (K) {
    case 1: return launch_k<1>(table, a, nblocks, s);
    case 2: return launch_k<2>(table, a, nblocks, s);
    case 4: return launch_k<4>(table, a, nblocks, s);
    case 8: return launch_k<8>(table, a, nblocks, s);
    case 16: return launch_k<16>(table, a, nblocks, s);
    case 32: return launch_k<32>(table, a, nblocks, s);
  }
  return MX_ERR_SIZE;
}
}  // namespace mxm
