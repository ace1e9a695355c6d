// Host side of every launcher of libmxpaillier.so: pick the template instance for a group of K lanes, launch a kernel
// with one argument block and report the launch's error.  Host code only.
#pragma once
#include <type_traits>
#include "mx_host.hpp"

// f(std::integral_constant<int, K>{}) for the K among Ks..., MX_ERR_SIZE for any other K: the list at a call site IS the
// set of instances that translation unit builds (f's body is instantiated once per entry of the list, in the list's
// order: a left fold — the order decides where the kernels lie in the code object).
template <int... Ks, class F>
inline int mx_dispatch_lanes(int K, F&& f) {
  int rc = MX_ERR_SIZE;
  (void)(... || (K == Ks ? (rc = f(std::integral_constant<int, Ks>{}), true) : false));
  return rc;
}

template <class Kern, class Args>
inline int mx_launch(Kern kern, int64_t nblocks, int threads, size_t lds, hipStream_t s, const Args& a) {
  mxh::touch_gpu();
  hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3((unsigned)threads), lds, s, a);
  MX_HIP(hipGetLastError());
  return MX_OK;
}
