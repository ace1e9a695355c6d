// Host helpers shared by the translation units of the private-key (CRT) entry points (mx_capi_crt.hip, mx_capi_crt_enc.hip).
#pragma once
#include "mx_upload.hpp"

namespace {

bool same_words(const u32* a, const u32* b, int limbs) {
  for (int i = 0; i < limbs; ++i) if (a[i] != b[i]) return false;
  return true;
}

// v 2^m mod r for any v of `limbs` words, as a row of rw words at dst (r has at most rw words)
void scaled_residue(u32* dst, const u32* v, const u32* r, int limbs, int m) {
  std::vector<u32> q(limbs), t(limbs + 1, 0u);
  divmod_words(q.data(), t.data(), v, limbs, r, limbs);
  shl_mod(t, r, limbs, m);
  std::memcpy(dst, t.data(), (size_t)limbs * 4);
}

int64_t crt_blocks(int64_t batch, int K) { return (batch + 64 / K - 1) / (64 / K); }

}  // namespace
