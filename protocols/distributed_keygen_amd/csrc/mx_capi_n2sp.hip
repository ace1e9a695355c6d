// Encrypted sparse matrix products (mx_spmm_n2.hpp): the shape query, the two entry points on either
// side of mx_histogram_nsquare_run and the instantiations of their kernels for the narrow geometry, every group width of
// the pair kernel (translation unit of its own, built in parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_spmm_n2.hpp"

namespace mxh {
// mx_capi_n2.hip: the refusals every launch over histogram row sets starts with, the geometry and the plan's constants
int narrow_rows_launch(const mx_nsquare_plan* plan, int limbs2, int limbs_per_lane, int64_t groups, int* lanes, int* nblk,
                       const uint32_t** consts, int64_t* nblocks);
}

namespace {
constexpr int MX_SPMM_MAX_WINDOW = 8;            // what the caller may ask for
constexpr int MX_SPMM_MODEL_MAX_WINDOW = 6;      // the cost model's range
constexpr int MX_SPMM_MAX_WEIGHT_BITS = 63;      // |val| <= 2^63 - 1
constexpr int MX_SPMM_MAX_POSITIONS = 64;

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Window of the digit histogram, from pair products: 2^w - 2 per table to build its powers, one per stored term and
// digit position (an upper bound: zero digits are dropped), and (D - 1) (w + 1) per output row for Horner's rule.
int spmm_window(int64_t n_tables, int64_t n_rows, int64_t nnz, int weight_bits) {
  if (weight_bits <= 1) return 1;
  int best = 1;
  unsigned __int128 bestc = 0;
  for (int w = 1; w <= MX_SPMM_MODEL_MAX_WINDOW; ++w) {
    const unsigned __int128 d = (unsigned)ceil_div(weight_bits, w);
    const unsigned __int128 c = (unsigned __int128)n_tables * (unsigned)((1 << w) - 2) + (unsigned __int128)nnz * d +
                                (unsigned __int128)n_rows * (d - 1) * (unsigned)(w + 1);
    if (w == 1 || c < bestc) { bestc = c; best = w; }
  }
  return best;
}

enum class SpmmKernel { tables, horner };
int launch_spmm(int K, SpmmKernel which, const mx::SpmmN2Args& a, int64_t nblocks, hipStream_t s) {
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32>(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    const size_t lds = mx::hist_n2_lds_bytes<KK, LIMBS_PER_LANE>();
    return which == SpmmKernel::tables
               ? mx_launch(mx::spmm_n2_table_kernel<KK, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a)
               : mx_launch(mx::spmm_n2_horner_kernel<KK, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a);
  });
}
}  // namespace

extern "C" int mx_spmm_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries) {
  return mx_histogram_nsquare_instances(lanes, limbs_per_lane, max_entries);      // the same narrow instances
}

extern "C" int mx_spmm_nsquare_shape(int n_bits, int64_t n_tables, int64_t n_rows, int64_t nnz, int weight_bits,
                                     int limbs_per_lane, int window, int* lanes, int* limbs_per_lane_out, int* window_out,
                                     int* positions, int64_t* row_bytes) {
  if (!lanes || !limbs_per_lane_out || !window_out || !positions || !row_bytes) return MX_ERR_ARG;
  if (n_tables < 0 || n_rows < 0 || nnz < 0 || weight_bits < 0 || weight_bits > MX_SPMM_MAX_WEIGHT_BITS) return MX_ERR_ARG;
  if (window < 0 || window > MX_SPMM_MAX_WINDOW) return MX_ERR_ARG;
  int chunk = 0;
  MX_TRY(mx_histogram_nsquare_shape(n_bits, 0, 0, 0, limbs_per_lane, 0, lanes, limbs_per_lane_out, &chunk, row_bytes));
  const int w = window > 0 ? window : spmm_window(n_tables, n_rows, nnz, weight_bits);
  *window_out = w;
  *positions = weight_bits > 0 ? ceil_div(weight_bits, w) : 1;
  return MX_OK;
}

extern "C" int64_t mx_spmm_nsquare_workspace_bytes(int n_bits, int64_t n_inputs, int window, int limbs_per_lane) {
  if (n_inputs < 0 || window < 1 || window > MX_SPMM_MAX_WINDOW) return MX_ERR_ARG;
  if (n_inputs >= ((int64_t)1 << 31)) return MX_ERR_ARG;                         // (the product below stays in 64 bits)
  return mx_histogram_nsquare_workspace_bytes(n_bits, n_inputs * ((1 << window) - 1), limbs_per_lane);
}

extern "C" int mx_spmm_nsquare_tables(const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_inputs, int limbs2,
                                      int window, uint32_t* d_rows, int64_t rows_bytes, int limbs_per_lane, void* stream) {
  if (!plan || !plan->d_plan || !d_inputs || !d_rows || plan->limbs_n <= 0) return MX_ERR_ARG;
  if (n_inputs < 1 || limbs2 <= 0 || window < 1 || window > MX_SPMM_MAX_WINDOW) return MX_ERR_ARG;
  if (limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE) return MX_ERR_ARG;
  const int64_t need = mx_spmm_nsquare_workspace_bytes(plan->n_bits, n_inputs, window, LIMBS_PER_LANE);
  if (need == MX_ERR_ARG) return MX_ERR_ARG;                                     // too many rows for one row set
  mx::SpmmN2Args a{};
  int lanes = 0;
  int64_t nblocks = 0;
  MX_TRY(mxh::narrow_rows_launch(plan, limbs2, limbs_per_lane, n_inputs + 1, &lanes, &a.nblk, &a.consts, &nblocks));      // one more group: the one row
  if (need < 0) return (int)need;
  if (need > rows_bytes) return MX_ERR_WORKSPACE;
  a.inputs = d_inputs;
  a.rows_out = d_rows;
  a.n_inputs = n_inputs;
  a.entries = (1 << window) - 1; a.window = window;
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.ksplit = plan->n_bits - 1;
  hipStream_t s = (hipStream_t)stream;
  MxKernelTimer timer(s);
  return launch_spmm(lanes, SpmmKernel::tables, a, nblocks, s);
}

extern "C" int mx_spmm_nsquare_horner(const mx_nsquare_plan* plan, const uint32_t* d_rows, int64_t n_rows, int positions,
                                      int window, const uint32_t* d_bias_rows, uint32_t* d_out, int limbs2, int64_t out_bytes,
                                      int limbs_per_lane, void* stream) {
  if (!plan || !plan->d_plan || !d_rows || !d_out || plan->limbs_n <= 0) return MX_ERR_ARG;
  if (n_rows < 1 || limbs2 <= 0 || positions < 1 || positions > MX_SPMM_MAX_POSITIONS) return MX_ERR_ARG;
  if (window < 1 || window > MX_SPMM_MAX_WINDOW) return MX_ERR_ARG;
  if (limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE) return MX_ERR_ARG;
  if (n_rows >= ((int64_t)1 << 31)) return MX_ERR_ARG;
  // the segment products are a row set of n_rows * positions rows: its refusals are the histogram's
  const int64_t set_bytes = mx_histogram_nsquare_workspace_bytes(plan->n_bits, n_rows * positions, LIMBS_PER_LANE);
  if (set_bytes == MX_ERR_ARG) return MX_ERR_ARG;
  mx::SpmmN2Args a{};
  int lanes = 0;
  int64_t nblocks = 0;
  MX_TRY(mxh::narrow_rows_launch(plan, limbs2, limbs_per_lane, n_rows, &lanes, &a.nblk, &a.consts, &nblocks));
  if (set_bytes < 0) return (int)set_bytes;
  if (n_rows * (int64_t)limbs2 * 4 > out_bytes) return MX_ERR_WORKSPACE;
  a.rows = d_rows;
  a.bias_rows = d_bias_rows;
  a.out = d_out;
  a.n_rows = n_rows;
  a.positions = positions; a.window = window;
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.ksplit = plan->n_bits - 1;
  hipStream_t s = (hipStream_t)stream;
  MxKernelTimer timer(s);
  return launch_spmm(lanes, SpmmKernel::horner, a, nblocks, s);
}
