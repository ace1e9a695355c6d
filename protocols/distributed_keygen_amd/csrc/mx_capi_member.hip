// mx_member_challenges: the challenge arithmetic of the one-of-k membership proofs (mx_member.hpp) behind the C ABI
// (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_member.hpp"

extern "C" int mx_member_challenges(const uint32_t* d_e, const uint32_t* d_sim, const int32_t* d_index, uint32_t* d_out,
                                    uint8_t* d_status, int k, int64_t count, int mode, void* stream) {
  return mx::run_member_challenges(d_e, d_sim, d_index, d_out, d_status, k, count, mode, stream);
}
