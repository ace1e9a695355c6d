// mx_slots_encode / mx_slots_decode: the slot codec (mx_slots.hpp) behind the C ABI (translation unit of its own, built in
// parallel with the others).
#include "mx_launch.hpp"
#include "mx_slots.hpp"

using namespace mxh;

namespace {

// Checks shared by the two entry points and everything of the argument block that does not depend on the direction.
int slots_args(mx::SlotsArgs& a, int64_t count, const uint32_t* h_n, int limbs_n, int slot_bits, int slots, int is_signed,
               int stride) {
  if (!h_n || count < 0 || limbs_n < 1 || slots < 1) return MX_ERR_ARG;
  if (slot_bits < 1 || slot_bits > (is_signed ? 64 : 63)) return MX_ERR_ARG;
  if (stride < limbs_n) return MX_ERR_ARG;
  if (limbs_n > mx::SLOTS_MAX_WORDS || stride > (1 << 16)) return MX_ERR_SIZE;
  if (!(h_n[0] & 1u)) return MX_ERR_MODULUS;
  const int bits = bit_length(h_n, limbs_n);
  if (bits < 2) return MX_ERR_MODULUS;
  if ((int64_t)slots * slot_bits > bits - 2) return MX_ERR_ARG;
  for (int w = 0; w < mx::SLOTS_MAX_WORDS; ++w) {
    a.n[w] = w < limbs_n ? h_n[w] : 0u;
    a.off[w] = 0u;
  }
  if (is_signed)
    for (int i = 0; i < slots; ++i) {
      const int bit = slot_bits * i + slot_bits - 1;
      a.off[bit >> 5] |= 1u << (bit & 31);
    }
  a.count = count;
  a.outputs = (count + slots - 1) / slots;
  a.limbs = limbs_n;
  a.stride = stride;
  a.slot_bits = slot_bits;
  a.slots = slots;
  a.is_signed = is_signed ? 1 : 0;
  a.lds_stride = (limbs_n + 2) | 1;
  const int fit = mx::SLOTS_LDS_BUDGET / (4 * a.lds_stride);          // >= 47
  a.rows_per_group = fit < 64 ? fit : 64;
  if ((a.outputs + a.rows_per_group - 1) / a.rows_per_group > 0x7FFFFFFF) return MX_ERR_SIZE;
  a.values = nullptr; a.values_out = nullptr; a.rows_in = nullptr; a.rows_out = nullptr; a.status = nullptr;
  return MX_OK;
}

template <typename Kernel>
int slots_launch(Kernel kernel, const mx::SlotsArgs& a, void* stream) {
  const unsigned groups = (unsigned)((a.outputs + a.rows_per_group - 1) / a.rows_per_group);
  const size_t lds = (size_t)a.rows_per_group * a.lds_stride * 4;
  return mx_launch(kernel, groups, mx::SLOTS_THREADS, lds, (hipStream_t)stream, a);
}

}  // namespace

extern "C" int mx_slots_encode(const int64_t* d_values, int64_t count, const uint32_t* h_n, int limbs_n, int slot_bits,
                               int slots, int is_signed, uint32_t* d_out, int out_stride, uint8_t* d_status, void* stream) {
  mx::SlotsArgs a;
  const int rc = slots_args(a, count, h_n, limbs_n, slot_bits, slots, is_signed, out_stride);
  if (rc != MX_OK) return rc;
  if (count == 0) return MX_OK;
  if (!d_values || !d_out || !d_status) return MX_ERR_ARG;
  a.values = d_values;
  a.rows_out = d_out;
  a.status = d_status;
  return slots_launch(mx::slots_encode_kernel, a, stream);
}

extern "C" int mx_slots_decode(const uint32_t* d_rows, int row_stride, int64_t count, const uint32_t* h_n, int limbs_n,
                               int slot_bits, int slots, int is_signed, int64_t* d_out, void* stream) {
  mx::SlotsArgs a;
  const int rc = slots_args(a, count, h_n, limbs_n, slot_bits, slots, is_signed, row_stride);
  if (rc != MX_OK) return rc;
  if (count == 0) return MX_OK;
  if (!d_rows || !d_out) return MX_ERR_ARG;
  a.rows_in = d_rows;
  a.values_out = d_out;
  return slots_launch(mx::slots_decode_kernel, a, stream);
}
