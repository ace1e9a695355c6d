// mx_multiexp_* / mx_response_rows: the multi-exponentiation over a generic odd modulus (mx_multiexp.hpp) and the per-row
// response z = rho + e x (mx_response.hpp) of the range proofs behind the C ABI (translation unit of its own, built in
// parallel with the others).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_multiexp.hpp"
#include "mx_response.hpp"

namespace {
constexpr int MX_MULTIEXP_MOD_MAX_WINDOW = 8;
constexpr int64_t MX_MULTIEXP_MOD_TABLE_BUDGET = (int64_t)1 << 30;      // bytes of tables the automatic window stays within
constexpr int64_t MX_MULTIEXP_MOD_MAX_COUNT = ((int64_t)1 << 31) - 1;   // inputs and outputs (the index is an int; one grid)

// the narrow geometry of the generic kernel: groups of 1 .. 64 lanes of 9 limbs
bool multiexp_mod_geometry(int mod_bits, Geometry& g) { return choose_geometry(mod_bits, g, LIMBS_PER_LANE); }

int64_t table_bytes(const Geometry& g, int64_t n_inputs, int window) {
  return align256((n_inputs > 0 ? n_inputs : 1) * ((int64_t)g.K * g.L * 4 << window));
}

// Window of the interleaved fixed-window schedule, from Montgomery products: 2^w - 2 per input to build its table,
// ceil(bits / w) multiplications per term and output, (ceil(bits / w) - 1) w squarings per output; the widest window
// whose tables stay within the budget when the cheapest one does not.
int multiexp_mod_window(const Geometry& g, int64_t n_inputs, int64_t n_outputs, int64_t terms, int weight_bits) {
  int best = 1;
  double bestc = -1.0;
  for (int w = 1; w <= MX_MULTIEXP_MOD_MAX_WINDOW; ++w) {
    if (w > 1 && table_bytes(g, n_inputs, w) > MX_MULTIEXP_MOD_TABLE_BUDGET) break;
    const double nwin = (double)((weight_bits + w - 1) / w);
    const double c = (double)n_inputs * (double)((1 << w) - 2) + (double)n_outputs * ((double)terms * nwin + (nwin - 1.0) * w);
    if (bestc < 0 || c < bestc) { bestc = c; best = w; }
  }
  return best;
}

template <int K>
int launch_multiexp_mod(bool table, const mx::MultiexpArgs& a, int64_t count, hipStream_t s) {
  using M_t = mx::Mont<K, LIMBS_PER_LANE, LIMB_BITS, true>;
  const int gpw = 64 / K;
  const size_t lds = (size_t)gpw * M_t::LDS_WORDS * 4;
  const int64_t nblocks = (count + gpw - 1) / gpw;
  return table ? mx_launch(mx::multiexp_table_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a)
               : mx_launch(mx::multiexp_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, nblocks, 64, lds, s, a);
}
}  // namespace

extern "C" int mx_multiexp_instances(int* lanes, int* limbs_per_lane, int max_entries) {
  static const int ks[] = {1, 2, 4, 8, 16, 32, 64};
  const int n = (int)(sizeof(ks) / sizeof(ks[0]));
  if (max_entries < 0 || (max_entries > 0 && (!lanes || !limbs_per_lane))) return MX_ERR_ARG;
  for (int i = 0; i < n && i < max_entries; ++i) { lanes[i] = ks[i]; limbs_per_lane[i] = LIMBS_PER_LANE; }
  return n;
}

extern "C" int mx_multiexp_shape(int mod_bits, int64_t n_inputs, int64_t n_outputs, int terms, int weight_bits, int window,
                                 int* lanes, int* limbs_per_lane_out, int* window_out) {
  if (!lanes || !limbs_per_lane_out || !window_out) return MX_ERR_ARG;
  if (n_inputs < 1 || n_outputs < 1 || terms < 1 || terms > MX_MULTIEXP_MAX_TERMS) return MX_ERR_ARG;
  if (weight_bits < 1 || weight_bits > MX_MULTIEXP_MAX_WEIGHT_BITS) return MX_ERR_ARG;
  if (window < 0 || window > MX_MULTIEXP_MOD_MAX_WINDOW) return MX_ERR_ARG;
  Geometry g;
  if (!multiexp_mod_geometry(mod_bits, g)) return MX_ERR_SIZE;
  *lanes = g.K;
  *limbs_per_lane_out = g.L;
  *window_out = window > 0 ? window : multiexp_mod_window(g, n_inputs, n_outputs, terms, weight_bits);
  return MX_OK;
}

extern "C" int64_t mx_multiexp_workspace_bytes(int mod_bits, int limbs, int64_t n_inputs, int terms, int window) {
  if (limbs < 1 || n_inputs < 1 || n_inputs > MX_MULTIEXP_MOD_MAX_COUNT || terms < 1 || terms > MX_MULTIEXP_MAX_TERMS) return MX_ERR_ARG;
  if (window < 1 || window > MX_MULTIEXP_MOD_MAX_WINDOW) return MX_ERR_ARG;
  Geometry g;
  if (!multiexp_mod_geometry(mod_bits, g)) return MX_ERR_SIZE;
  return 2 * align256((int64_t)limbs * 4) + align256((int64_t)terms * 4) + table_bytes(g, n_inputs, window);
}

extern "C" int mx_multiexp_run(const uint32_t* h_mod, int limbs, const uint32_t* d_inputs, int64_t n_inputs,
                               const int32_t* d_index, const uint32_t* d_weights, int terms, int weight_bits,
                               const int32_t* h_term_bits, uint32_t* d_out, int64_t n_outputs, int window, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!h_mod || !d_inputs || !d_index || !d_weights || !d_out || !d_ws) return MX_ERR_ARG;
  if (limbs < 1 || n_inputs < 1 || n_outputs < 1 || terms < 1 || terms > MX_MULTIEXP_MAX_TERMS) return MX_ERR_ARG;
  if (n_inputs > MX_MULTIEXP_MOD_MAX_COUNT || n_outputs > MX_MULTIEXP_MOD_MAX_COUNT) return MX_ERR_ARG;
  if (weight_bits < 1 || weight_bits > MX_MULTIEXP_MAX_WEIGHT_BITS) return MX_ERR_ARG;
  if (window < 1 || window > MX_MULTIEXP_MOD_MAX_WINDOW) return MX_ERR_ARG;
  std::vector<u32> term_bits((size_t)terms, (u32)weight_bits);
  for (int t = 0; h_term_bits && t < terms; ++t) {
    if (h_term_bits[t] < 0 || h_term_bits[t] > weight_bits) return MX_ERR_ARG;
    term_bits[t] = (u32)h_term_bits[t];
  }
  if (!(h_mod[0] & 1u)) return MX_ERR_MODULUS;
  const int bits = bit_length(h_mod, limbs);
  if (bits < 2) return MX_ERR_MODULUS;
  Geometry g;
  if (!multiexp_mod_geometry(bits, g)) return MX_ERR_SIZE;
  const int64_t need = mx_multiexp_workspace_bytes(bits, limbs, n_inputs, terms, window);
  if (need < 0) return (int)need;
  if (need > ws_bytes) return MX_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)d_ws;
  const int64_t off_rmodn = align256((int64_t)limbs * 4), off_terms = 2 * off_rmodn;
  const int64_t off_tables = off_terms + align256((int64_t)terms * 4);
  std::vector<u32> rmodn((size_t)limbs);
  two_pow_mod(rmodn.data(), h_mod, limbs, g.W * g.L * g.nblk);           // R mod M, the Montgomery form of 1
  MX_TRY(upload_words(ws, h_mod, (size_t)limbs, s));
  MX_TRY(upload_words(ws + off_rmodn, rmodn.data(), (size_t)limbs, s));
  MX_TRY(upload_words(ws + off_terms, term_bits.data(), (size_t)terms, s));
  mx::MultiexpArgs a{};
  a.inputs = d_inputs;
  a.tables = (u32*)(ws + off_tables);
  a.mod = (const u32*)ws;
  a.rmodn = (const u32*)(ws + off_rmodn);
  a.index = d_index;
  a.weights = d_weights;
  a.term_bits = (const int*)(ws + off_terms);
  a.out = d_out;
  a.n_inputs = n_inputs; a.rows = n_outputs;
  a.terms = terms;
  a.window = window;
  a.wwords = (weight_bits + 31) / 32;
  a.nwin = (weight_bits + window - 1) / window;
  a.limbs = limbs; a.nblk = g.nblk;
  MxKernelTimer timer(s);
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(g.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    MX_TRY(launch_multiexp_mod<K>(true, a, n_inputs, s));
    return launch_multiexp_mod<K>(false, a, n_outputs, s);
  });
}

extern "C" int mx_response_rows(const uint32_t* d_rho, const uint32_t* d_e, const uint32_t* d_x, uint32_t* d_z,
                                uint8_t* d_status, int wz, int ew, int wx, int64_t count, void* stream) {
  return mx::run_response<true>(d_rho, d_e, d_x, d_z, d_status, wz, ew, wx, count, stream);
}
