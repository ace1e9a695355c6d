// Instantiations of the fixed-base kernels modulo N^2 (mx_fixedbase_n2.hpp) for the narrow geometry, every group width
// of the pair kernel (translation unit of its own, built in parallel with the others).
#include "mx_upload.hpp"
#include "mx_fixedbase_n2.hpp"

namespace mxf {
template <int K>
static int launch_k(int pass, const mx::FixedBaseN2Args& a, int64_t nblocks, hipStream_t s) {
  const size_t lds = mx::fixedbase_n2_lds_bytes<K, LIMBS_PER_LANE>();
  const dim3 grid((unsigned)nblocks), block(64);
  if (pass == 0) hipLaunchKernelGGL((mx::fixedbase_n2_chain_kernel<K, LIMBS_PER_LANE, LIMB_BITS>), grid, block, lds, s, a);
  else if (pass == 1) hipLaunchKernelGGL((mx::fixedbase_n2_fill_kernel<K, LIMBS_PER_LANE, LIMB_BITS>), grid, block, lds, s, a);
  else hipLaunchKernelGGL((mx::fixedbase_n2_run_kernel<K, LIMBS_PER_LANE, LIMB_BITS>), grid, block, lds, s, a);
  MX_HIP(hipGetLastError());
  return MX_OK;
}

// pass 0: chain, 1: fill, 2: run
int launch_fixedbase(int K, int pass, const mx::FixedBaseN2Args& a, int64_t nblocks, hipStream_t s) {
  switch (K) {
    case 1: return launch_k<1>(pass, a, nblocks, s);
    case 2: return launch_k<2>(pass, a, nblocks, s);
    case 4: return launch_k<4>(pass, a, nblocks, s);
    case 8: return launch_k<8>(pass, a, nblocks, s);
    case 16: return launch_k<16>(pass, a, nblocks, s);
    case 32: return launch_k<32>(pass, a, nblocks, s);
  }
  return MX_ERR_SIZE;
}
}  // namespace mxf
