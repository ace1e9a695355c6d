// mx_response_mod_rows: the response modulo M with its quotient, of the multiplication proofs (mx_response_mod.hpp),
// behind the C ABI (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_response_mod.hpp"

extern "C" int mx_response_mod_rows(const uint32_t* d_rho, const uint32_t* d_e, const uint32_t* d_x, const uint32_t* d_mod,
                                    uint64_t recip, int shift, uint32_t* d_w, uint32_t* d_t, uint8_t* d_status, int wn, int ew,
                                    int64_t count, void* stream) {
  return mx::run_response_mod(d_rho, d_e, d_x, d_mod, recip, shift, d_w, d_t, d_status, wn, ew, count, stream);
}
