// extern "C" entry points of libmxpaillier.so (declared in include/mxpaillier.h).
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_powmod.hpp"
#include "mx_sieve.hpp"
#include "mx_combine.hpp"
#include "mx_verdict.hpp"
#include "mx_jacobi.hpp"
#include "mx_mulmod.hpp"
#include "mx_select.hpp"
#include "mx_setup.hpp"
#include "mx_field.hpp"
#include "mx_modinv.hpp"
#include "mx_bimont.hpp"
#include "mx_queues.hpp"
#include <cstring>
#include <algorithm>
#include <chrono>
#include <cstdio>

namespace mxh {
thread_local hipError_t g_last_hip = hipSuccess;
std::atomic<bool> g_gpu_touched{false};
Knob g_knob_n2_segments;
Knob g_knob_n2_timeslice;
Knob g_knob_n2_friendly_1w;
Knob g_knob_generic_latency;
Knob g_knob_n2_split;
Knob g_knob_n2_bipair;
Knob g_knob_n2_lift;
Knob g_knob_jacobi_max_batches;
Knob g_knob_bi_pivot;
Knob g_knob_lat_lanes;
}
MxProfile g_mx_profile;

namespace {


// ---- modexp ------------------------------------------------------------------------------
struct PowmodPlan {
  Geometry geo;
  int win = 1;
  int64_t nblocks = 0, nlanes = 0;
  int64_t off_mods = 0, off_rmodn = 0, off_exps = 0, off_ops = 0, off_table = 0, off_bi = 0, total = 0;
};

}  // namespace
// latency instances (3 limbs per lane) live in mx_capi_lat.hip
namespace mxl {
int launch_powmod_lat(int K, const mx::PowmodArgs& a, int64_t nblocks, hipStream_t s);
int launch_rmodn_lat(int K, const mx::RmodnArgs& a, hipStream_t s);
int launch_powmod_bi(int K, const mx::PowmodBiArgs& a, int64_t nblocks, hipStream_t s);
int launch_bisetup(int K, const mx::BiSetupArgs& a, hipStream_t s);
}
namespace {
inline bool generic_lpl_ok(int lpl) {
  return lpl == 0 || lpl == LIMBS_PER_LANE || lpl == LIMBS_PER_LANE_WIDE || lpl == LIMBS_PER_LANE_LAT || lpl == LIMBS_PER_LANE_BI;
}

// Geometry when the caller leaves the choice to the library: the shape with the shortest estimated duration of ONE launch
// on an idle GPU.  A wavefront of the 3- / 9- / 18-limb instances carries 64 / K elements through the whole exponentiation
// in 1 : 1.43 : 2.12 of the time (instructions on its dependent chain: 16 / 28 / 47 per limb step, measured ratios), alone
// on its SIMD; every further wavefront per SIMD adds 0.6 / 0.8 / 0.96 of that (a second wavefront fills the issue slots
// the first one leaves: more of them in the short-limbed instances) — fitted to tools/sweep_generic.py at key_length 1024
// and 2048 (profiles/r04_sweep_generic.txt; the choice matches the fastest measured shape at every point of the sweep
// within 3 %).  Consequences: a keygen round's few hundred to a thousand modexps (2-25 survivors) run the latency
// instances (6.0 instead of 8.7 ms at key_length 2048), 256-384 candidates the wide ones (one wavefront per SIMD: 12.8
// instead of 15.3 ms), the saturating launches whichever packs the SIMDs more evenly.
double generic_estimate(int mod_bits, int64_t batch, int lpl) {
  Geometry g;
  if (!choose_geometry(mod_bits, g, lpl)) return -1.0;
  if (lpl == LIMBS_PER_LANE_WIDE && g.K > 32) return -1.0;          // no <64, 18> instance
  const int64_t simds = (int64_t)4 * mx_device_cus();
  if (g.bi) {
    // One workgroup = two wavefronts per 64 / K elements.  Alone on its compute unit a product costs the longer half plus
    // the hand-over (tools/bi_pivot_sweep.py, tools/sweep_generic.py; profiles/r05_*): relative to the one-wavefront latency
    // instance 0.42 + 22 / steps — 0.94 at key_length 1024 (42 steps), 0.71 at 2048 (75 steps) — and 0.84 for groups of 64
    // lanes (key_length 3072 / 4096: the hand-over costs them more).  A second workgroup on a compute unit adds most of
    // that again, so the form only pays while the launch leaves compute units idle.
    const int steps = g.L * g.nblk + g.L;
    const int64_t wgs = ((batch * g.K + 63) / 64 + mx::BI_PAIRS - 1) / mx::BI_PAIRS;      // four wavefronts each: one per SIMD of a CU
    const int64_t cus = mx_device_cus();
    const int64_t per_cu = (wgs + cus - 1) / cus;
    const double t1 = g.K == 64 ? 0.84 : 0.42 + 22.0 / (double)steps;
    return t1 * (1.0 + 0.9 * (double)(per_cu - 1));
  }
  const int64_t waves = (batch * g.K + 63) / 64;
  const int64_t per_simd = (waves + simds - 1) / simds;
  const double t1 = lpl == LIMBS_PER_LANE_LAT ? 1.0 : lpl == LIMBS_PER_LANE ? 1.43 : 2.12;
  const double more = lpl == LIMBS_PER_LANE_LAT ? 0.6 : lpl == LIMBS_PER_LANE ? 0.8 : 0.96;
  return t1 * (1.0 + more * (double)(per_simd - 1));
}
int auto_limbs_per_lane(int mod_bits, int64_t batch, int64_t groups) {
  (void)groups;
  int best = LIMBS_PER_LANE;
  double best_t = -1.0;
  for (int lpl : {LIMBS_PER_LANE, LIMBS_PER_LANE_WIDE, LIMBS_PER_LANE_LAT, LIMBS_PER_LANE_BI}) {
    if (lpl == LIMBS_PER_LANE_LAT && g_knob_generic_latency == 1) continue;
    if (lpl == LIMBS_PER_LANE_BI && g_knob_generic_latency != 0) continue;      // 1: no latency instances at all, 2: no bipartite form
    const double t = generic_estimate(mod_bits, batch, lpl);
    if (t > 0 && (best_t < 0 || t < best_t * 0.999)) { best_t = t; best = lpl; }
  }
  return best;
}

bool plan_powmod(int mod_bits, int limbs, int exp_limbs, int64_t batch, int64_t groups, PowmodPlan& p,
                 int limbs_per_lane) {
  if (limbs_per_lane == 0) limbs_per_lane = auto_limbs_per_lane(mod_bits, batch, groups);
  if (!choose_geometry(mod_bits, p.geo, limbs_per_lane)) return false;
  p.win = fixed_window(32 * exp_limbs);
  int gpw = 64 / p.geo.K;
  p.nblocks = (batch + gpw - 1) / gpw;
  p.nlanes = p.nblocks * 64;
  if (p.geo.bi) {                               // workgroups of BI_PAIRS wavefront pairs; the table has a column per lane of every pair
    p.nblocks = (p.nblocks + mx::BI_PAIRS - 1) / mx::BI_PAIRS;
    p.nlanes = p.nblocks * mx::BI_PAIRS * 64;
  }
  int64_t o = 0;
  p.off_mods = o;  o += align256((int64_t)groups * limbs * 4);
  p.off_rmodn = o; o += align256((int64_t)groups * limbs * 4);
  p.off_exps = o;  o += align256((int64_t)groups * exp_limbs * 4);
  p.off_ops = o;   o += align256((int64_t)MAX_SLIDING_OPS * 4);
  p.off_table = o; o += align256(((int64_t)1 << p.win) * p.geo.L * p.nlanes * 4);
  p.off_bi = o;
  if (p.geo.bi) o += align256((int64_t)groups * mx::BI_ROWS * p.geo.L * p.geo.K * 4);
  p.total = o;
  return true;
}

template <int K, int L>
int launch_powmod_kl(const mx::PowmodArgs& a, int64_t nblocks, hipStream_t s) {
  using M_t = mx::Mont<K, L, LIMB_BITS, true>;
  size_t lds = (size_t)(64 / K) * M_t::LDS_WORDS * 4;
  MxKernelTimer timer(s);
  return a.nops > 0 ? mx_launch(mx::powmod_kernel<K, L, LIMB_BITS, true>, nblocks, 64, lds, s, a)
                    : mx_launch(mx::powmod_kernel<K, L, LIMB_BITS, false>, nblocks, 64, lds, s, a);
}

// A kernel of the one-wavefront Montgomery form over `count` groups of K lanes: 64 / K groups per wavefront, each with
// its LDS words.
template <int K, int L, class Kern, class Args>
int launch_groups(Kern kern, int64_t count, hipStream_t s, const Args& a) {
  using M_t = mx::Mont<K, L, LIMB_BITS, true>;
  const int gpw = 64 / K;
  return mx_launch(kern, (count + gpw - 1) / gpw, 64, (size_t)gpw * M_t::LDS_WORDS * 4, s, a);
}

// R mod N of every group, on the device (mx_setup.hpp); always the narrow-L instance of the
// geometry's K would give a different R, so the instance follows the geometry of the consumer
int launch_rmodn(const Geometry& g, const u32* d_mods, u32* d_rmodn, int limbs, int64_t groups, hipStream_t s) {
  mx::RmodnArgs a;
  a.mods = d_mods; a.rmodn = d_rmodn; a.groups = groups; a.limbs = limbs; a.nblk = g.nblk;
  if (g.L == LIMBS_PER_LANE_LAT) return mxl::launch_rmodn_lat(g.K, a, s);
  const bool wide = g.L == LIMBS_PER_LANE_WIDE;
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(g.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    if (wide) {                                   // no <64, 18> instance
      if constexpr (K <= 32) return launch_groups<K, LIMBS_PER_LANE_WIDE>(mx::rmodn_kernel<K, LIMBS_PER_LANE_WIDE, LIMB_BITS>, groups, s, a);
      return MX_ERR_SIZE;
    }
    return launch_groups<K, LIMBS_PER_LANE>(mx::rmodn_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, groups, s, a);
  });
}

// Common tail of the modexp entry points: moduli and exponents are device-resident
// (d_mods [groups][limbs], d_exps [groups][exp_limbs]); h_exp0 is the host copy of the exponent when
// the launch shares one (sliding-window schedule), else null.
int powmod_launch(const uint32_t* d_bases, uint32_t* d_out, const u32* d_mods, const u32* d_exps, const u32* h_exp0,
                  int limbs, int exp_limbs, int max_ebits, int64_t groups, int64_t group_size, const PowmodPlan& p,
                  char* ws, hipStream_t s) {
  int ndigits = (max_ebits + p.win - 1) / p.win;
  if (ndigits < 1) ndigits = 1;
  if (p.geo.bi) {
    // the bipartite latency form (mx_bimont.hpp): its own setup kernel (fold constants and the conversion factor of every
    // modulus), fixed windows only, two wavefronts per workgroup
    mx::BiSetupArgs sa;
    sa.mods = d_mods; sa.consts = (u32*)(ws + p.off_bi); sa.groups = groups; sa.limbs = limbs;
    sa.nblk = p.geo.nblk; sa.pd = p.geo.L * p.geo.nblk; sa.h_lo = p.geo.h_lo;
    MX_TRY(mxl::launch_bisetup(p.geo.K, sa, s));
    mx::PowmodBiArgs b;
    b.bases = d_bases; b.out = d_out; b.mods = d_mods; b.exps = d_exps; b.consts = (const u32*)(ws + p.off_bi);
    b.table = (u32*)(ws + p.off_table);
    b.batch = groups * group_size; b.group_size = group_size;
    b.limbs = limbs; b.elimbs = exp_limbs; b.ndigits = ndigits; b.win = p.win;
    b.nblk = p.geo.nblk; b.pd = sa.pd; b.h_lo = p.geo.h_lo;
    return mxl::launch_powmod_bi(p.geo.K, b, p.nblocks, s);
  }
  MX_TRY(launch_rmodn(p.geo, d_mods, (u32*)(ws + p.off_rmodn), limbs, groups, s));
  mx::PowmodArgs a;
  a.bases = d_bases; a.out = d_out;
  a.mods = d_mods;
  a.rmodn = (const u32*)(ws + p.off_rmodn);
  a.exps = d_exps;
  a.table = (u32*)(ws + p.off_table);
  a.batch = groups * group_size; a.group_size = group_size;
  a.limbs = limbs; a.elimbs = exp_limbs; a.ndigits = ndigits; a.win = p.win; a.nblk = p.geo.nblk;
  a.ops = nullptr; a.nops = 0;
  if (groups == 1 && max_ebits > 0 && h_exp0) {
    // one exponent for the whole launch: sliding window (odd powers only)
    int w = sliding_window(max_ebits);
    if (w > p.win) w = p.win;                       // the table region was sized for 2^win entries
    std::vector<u32> ops = pack_sliding_ops(sliding_schedule(h_exp0, exp_limbs, w));
    if ((int)ops.size() <= MAX_SLIDING_OPS) {
      MX_TRY(upload_words(ws + p.off_ops, ops.data(), ops.size(), s));
      a.ops = (const u32*)(ws + p.off_ops);
      a.nops = (int)ops.size();
      a.win = w;
    }
  }
  if (p.geo.L == LIMBS_PER_LANE_LAT) return mxl::launch_powmod_lat(p.geo.K, a, p.nblocks, s);
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(p.geo.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    if (p.geo.L == LIMBS_PER_LANE_WIDE) {
      // the largest supported modulus (MAX_MOD_BITS) needs 32 wide lanes: no <64, 18> instance
      if constexpr (K <= 32) return launch_powmod_kl<K, LIMBS_PER_LANE_WIDE>(a, p.nblocks, s);
      return MX_ERR_SIZE;
    }
    return launch_powmod_kl<K, LIMBS_PER_LANE>(a, p.nblocks, s);
  });
}

// host operands: validate, upload, launch
int powmod_impl(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* h_mods, const uint32_t* h_exps,
                int limbs, int exp_limbs, int64_t groups, int64_t group_size, int limbs_per_lane, void* d_ws,
                int64_t ws_bytes, void* stream) {
  if (!d_bases || !d_out || !h_mods || !h_exps || !d_ws) return MX_ERR_ARG;
  if (limbs <= 0 || exp_limbs <= 0 || groups <= 0 || group_size <= 0) return MX_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int64_t batch = groups * group_size;
  int max_bits = 0;
  for (int64_t g = 0; g < groups; ++g) {
    const u32* n = h_mods + g * limbs;
    if (!(n[0] & 1u)) return MX_ERR_MODULUS;
    int b = bit_length(n, limbs);
    if (b < 2) return MX_ERR_MODULUS;
    if (b > max_bits) max_bits = b;
  }
  PowmodPlan p;
  if (!plan_powmod(max_bits, limbs, exp_limbs, batch, groups, p, limbs_per_lane)) return MX_ERR_SIZE;
  // the sizing call only knows `limbs`; it assumes the largest modulus that fits them
  if (p.total > ws_bytes) return MX_ERR_WORKSPACE;
  int max_ebits = 0;
  for (int64_t g = 0; g < groups; ++g) {
    int b = bit_length(h_exps + g * exp_limbs, exp_limbs);
    if (b > max_ebits) max_ebits = b;
  }
  char* ws = (char*)d_ws;
  MX_TRY(upload_words(ws + p.off_mods, h_mods, (size_t)groups * limbs, s));
  MX_TRY(upload_words(ws + p.off_exps, h_exps, (size_t)groups * exp_limbs, s));
  return powmod_launch(d_bases, d_out, (const u32*)(ws + p.off_mods), (const u32*)(ws + p.off_exps),
                       groups == 1 ? h_exps : nullptr, limbs, exp_limbs, max_ebits, groups, group_size, p, ws, s);
}

// ---- lane self-test ------------------------------------------------------------------------
template <int K>
__device__ int lanes_check(unsigned v) {
  using D = mx::Lanes<K, true>;
  using R = mx::Lanes<K, false>;
  unsigned kn = D::keep_next_mask(), kp = D::keep_prev_mask();
  int bad = 0;
  bad += D::bcast0(v) != R::bcast0(v);
  bad += D::from_next(v, kn) != R::from_next(v, kn);
  bad += D::from_prev(v, kp) != R::from_prev(v, kp);
  // semantic anchors independent of either implementation
  unsigned lane = threadIdx.x & 63, pos = lane & (K - 1), base = lane - pos;
  unsigned f = lane * 2654435761u + 12345u;   // f(lane)
  auto F = [](unsigned l) { return l * 2654435761u + 12345u; };
  bad += D::bcast0(f) != F(base);
  bad += D::from_next(f, kn) != (pos == K - 1 ? 0u : F(lane + 1));
  bad += D::from_prev(f, kp) != (pos == 0 ? 0u : F(lane - 1));
  return bad;
}

// Occupies one wavefront slot for `ticks` periods of the 100 MHz real-time counter and does nothing else:
// the probe with which a caller finds out whether two of its streams run concurrently (mx_spin).
__global__ void spin_kernel(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// One wavefront idles for `ticks` periods of the 100 MHz real-time counter and reports how far the shader clock
// counter (s_memtime) advanced meanwhile: the clock the SIMDs are actually running at while whatever else is in
// flight on the device keeps them busy (mx_clock_probe).
__global__ void clock_probe_kernel(unsigned long long ticks, unsigned long long* out) {
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  unsigned long long r1 = r0;
  while (r1 - r0 < ticks) { __builtin_amdgcn_s_sleep(8); r1 = __builtin_amdgcn_s_memrealtime(); }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; }
}

__global__ void lanes_selftest_kernel(int* out) {
  unsigned v = threadIdx.x * 40503u + 977u;
  int bad = 0;
  bad += lanes_check<1>(v);
  bad += lanes_check<2>(v);
  bad += lanes_check<4>(v);
  bad += lanes_check<8>(v);
  bad += lanes_check<16>(v);
  bad += lanes_check<32>(v);
  bad += lanes_check<64>(v);
  atomicAdd(out, bad);
}

}  // namespace

extern "C" {

int mx_version(void) { return 404; }

const char* mx_error_string(int code) {
  switch (code) {
    case MX_OK: return "ok";
    case MX_ERR_ARG: return "invalid argument";
    case MX_ERR_SIZE: return "modulus too large for the engine";
    case MX_ERR_MODULUS: return "modulus must be odd and >= 3";
    case MX_ERR_WORKSPACE: return "workspace too small";
    case MX_ERR_HIP: return "HIP runtime error";
    case MX_ERR_STATE: return "too late: the library has already used the GPU in this process";
  }
  return "unknown error";
}

const char* mx_last_hip_error(void) { return hipGetErrorString(g_last_hip); }

namespace {
std::mutex g_hw_queues_mu;
int g_hw_queues_configured = 0;      // what mx_configure_hw_queues last wrote or found; 0 = never called
}

int mx_configure_hw_queues(int queues) {
  std::lock_guard<std::mutex> lock(g_hw_queues_mu);
  if (g_gpu_touched.load(std::memory_order_relaxed)) return MX_ERR_STATE;
  const mxq::QueueDecision d = mxq::decide_hw_queues(queues, std::getenv("GPU_MAX_HW_QUEUES"),
                                                     mxq::keep_requested(std::getenv("MX_HW_QUEUES_KEEP")));
  if (d.write) {
    char text[16];
    std::snprintf(text, sizeof text, "%d", d.value);
    if (setenv("GPU_MAX_HW_QUEUES", text, 1) != 0) return MX_ERR_ARG;
  }
  g_hw_queues_configured = d.value;
  return d.value;
}

int mx_hw_queues_configured(void) {
  std::lock_guard<std::mutex> lock(g_hw_queues_mu);
  return g_hw_queues_configured;
}

int mx_debug_knob(int knob, int value) {
  if (value < 0) return MX_ERR_ARG;
  switch (knob) {
    case MX_KNOB_N2_SEGMENTS: if (value > 64) return MX_ERR_ARG; g_knob_n2_segments = value; return MX_OK;
    case MX_KNOB_N2_TIMESLICE: if (value > 2 && (value < 17 || value > 19)) return MX_ERR_ARG; g_knob_n2_timeslice = value; return MX_OK;
    case MX_KNOB_JACOBI_MAX_BATCHES: g_knob_jacobi_max_batches = value; return MX_OK;
    case MX_KNOB_N2_FRIENDLY_1W: if (value > 1) return MX_ERR_ARG; g_knob_n2_friendly_1w = value; return MX_OK;
    case MX_KNOB_GENERIC_LATENCY: if (value > 2) return MX_ERR_ARG; g_knob_generic_latency = value; return MX_OK;
    case MX_KNOB_N2_SPLIT: if (value > 2) return MX_ERR_ARG; g_knob_n2_split = value; return MX_OK;
    case MX_KNOB_N2_BIPAIR: if (value > 1) return MX_ERR_ARG; g_knob_n2_bipair = value; return MX_OK;
    case MX_KNOB_N2_LIFT: if (value > 2) return MX_ERR_ARG; g_knob_n2_lift = (value + 1) % 3; return MX_OK;
    case MX_KNOB_BI_PIVOT: if (value > 192) return MX_ERR_ARG; g_knob_bi_pivot = value; return MX_OK;
    case MX_KNOB_LAT_LANES: if (value > 64) return MX_ERR_ARG; g_knob_lat_lanes = value; return MX_OK;
  }
  return MX_ERR_ARG;
}

int mx_profile(int enable) {
  std::lock_guard<std::mutex> lock(g_mx_profile.mu);
  g_mx_profile.on = enable != 0;
  return MX_OK;
}

int mx_profile_collect(double* total_ms, int* launches) {
  if (!total_ms || !launches) return MX_ERR_ARG;
  touch_gpu();
  std::lock_guard<std::mutex> lock(g_mx_profile.mu);
  double sum = 0;
  int n = 0, rc = MX_OK;
  for (auto& ev : g_mx_profile.events) {
    float ms = 0;
    if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
      sum += ms;
      ++n;
    } else {
      rc = MX_ERR_HIP;
    }
    hipEventDestroy(ev.first);
    hipEventDestroy(ev.second);
  }
  g_mx_profile.events.clear();
  *total_ms = sum;
  *launches = n;
  return rc;
}

int mx_geometry(int mod_bits, int* k, int* l, int* w, int* blocks) {
  Geometry g;
  if (!choose_geometry(mod_bits, g, LIMBS_PER_LANE)) return MX_ERR_SIZE;
  if (k) *k = g.K;
  if (l) *l = g.L;
  if (w) *w = g.W;
  if (blocks) *blocks = g.nblk;
  return MX_OK;
}

int64_t mx_powmod_workspace_bytes(int limbs, int exp_limbs, int64_t batch, int64_t groups) {
  if (limbs <= 0 || exp_limbs <= 0 || batch <= 0 || groups <= 0) return MX_ERR_ARG;
  PowmodPlan p, q;
  if (!plan_powmod(sizing_bits(limbs), limbs, exp_limbs, batch, groups, p, LIMBS_PER_LANE)) return MX_ERR_SIZE;
  int64_t most = p.total;
  if (plan_powmod(sizing_bits(limbs), limbs, exp_limbs, batch, groups, q, LIMBS_PER_LANE_WIDE) && q.total > most) most = q.total;
  // (the latency geometry only exists up to 64 x 3 limbs: rows that could hold a wider modulus are sized with the
  // widest one it takes)
  const int lat_bits = std::min(sizing_bits(limbs), LIMB_BITS * LIMBS_PER_LANE_LAT * 64 - 4 - LIMB_BITS - 2);
  if (plan_powmod(lat_bits, limbs, exp_limbs, batch, groups, q, LIMBS_PER_LANE_LAT) && q.total > most) most = q.total;
  const int bi_bits = std::min(sizing_bits(limbs), LIMB_BITS * LIMBS_PER_LANE_LAT * 62 - 35);
  if (plan_powmod(bi_bits, limbs, exp_limbs, batch, groups, q, LIMBS_PER_LANE_BI) && q.total > most) most = q.total;
  return most;
}

int mx_powmod_shared(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* h_mod, const uint32_t* h_exp,
                     int limbs, int exp_limbs, int64_t batch, void* d_workspace, int64_t workspace_bytes,
                     void* stream) {
  return powmod_impl(d_bases, d_out, h_mod, h_exp, limbs, exp_limbs, 1, batch, 0,
                     d_workspace, workspace_bytes, stream);
}

int mx_powmod_shared_lpl(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* h_mod, const uint32_t* h_exp,
                         int limbs, int exp_limbs, int64_t batch, int limbs_per_lane, void* d_workspace,
                         int64_t workspace_bytes, void* stream) {
  if (!generic_lpl_ok(limbs_per_lane)) return MX_ERR_ARG;
  return powmod_impl(d_bases, d_out, h_mod, h_exp, limbs, exp_limbs, 1, batch, limbs_per_lane, d_workspace,
                     workspace_bytes, stream);
}

int mx_powmod_multi(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* h_mods, const uint32_t* h_exps,
                    int limbs, int exp_limbs, int64_t groups, int64_t group_size, void* d_workspace,
                    int64_t workspace_bytes, void* stream) {
  return powmod_impl(d_bases, d_out, h_mods, h_exps, limbs, exp_limbs, groups, group_size,
                     0, d_workspace, workspace_bytes, stream);
}

int mx_powmod_multi_dev(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* d_mods, const uint32_t* d_exps,
                        int limbs, int exp_limbs, int mod_bits, int exp_bits, int64_t groups, int64_t group_size,
                        int limbs_per_lane, void* d_workspace, int64_t workspace_bytes, void* stream) {
  if (!d_bases || !d_out || !d_mods || !d_exps || !d_workspace) return MX_ERR_ARG;
  if (limbs <= 0 || exp_limbs <= 0 || groups <= 0 || group_size <= 0) return MX_ERR_ARG;
  if (mod_bits < 2 || mod_bits > 32 * limbs || exp_bits < 0 || exp_bits > 32 * exp_limbs) return MX_ERR_ARG;
  if (!generic_lpl_ok(limbs_per_lane)) return MX_ERR_ARG;
  PowmodPlan p;
  if (!plan_powmod(mod_bits, limbs, exp_limbs, groups * group_size, groups, p, limbs_per_lane)) return MX_ERR_SIZE;
  if (p.total > workspace_bytes) return MX_ERR_WORKSPACE;
  return powmod_launch(d_bases, d_out, d_mods, d_exps, nullptr, limbs, exp_limbs, exp_bits, groups, group_size, p,
                       (char*)d_workspace, (hipStream_t)stream);
}

int mx_powmod_geometry_for(int mod_bits, int64_t batch, int64_t groups, int limbs_per_lane, int* k, int* l, int* w,
                           int* blocks) {
  if (!k || !l || !w || !blocks || batch <= 0 || groups <= 0) return MX_ERR_ARG;
  if (!generic_lpl_ok(limbs_per_lane)) return MX_ERR_ARG;
  Geometry g;
  if (!choose_geometry(mod_bits, g, limbs_per_lane ? limbs_per_lane : auto_limbs_per_lane(mod_bits, batch, groups)))
    return MX_ERR_SIZE;
  *k = g.K; *l = g.L; *w = g.W; *blocks = g.nblk;
  return MX_OK;
}

int mx_powmod_launch_form(int mod_bits, int64_t batch, int64_t groups, int limbs_per_lane, int* wavefronts_per_group,
                          int* pivot) {
  if (!wavefronts_per_group || batch <= 0 || groups <= 0) return MX_ERR_ARG;
  if (!generic_lpl_ok(limbs_per_lane)) return MX_ERR_ARG;
  Geometry g;
  if (!choose_geometry(mod_bits, g, limbs_per_lane ? limbs_per_lane : auto_limbs_per_lane(mod_bits, batch, groups)))
    return MX_ERR_SIZE;
  *wavefronts_per_group = g.bi ? 2 : 1;
  if (pivot) *pivot = g.h_lo;
  return MX_OK;
}

int mx_spin(int64_t microseconds, void* stream) {
  if (microseconds < 0 || microseconds > 1000000) return MX_ERR_ARG;
  return mx_launch(spin_kernel, 1, 64, 0, (hipStream_t)stream, (unsigned long long)microseconds * 100ull);
}

int mx_stream_census(void* const* streams, int n, int64_t spin_us, int* group_of) {
  if (!streams || !group_of || n < 1 || n > 64 || spin_us < 1 || spin_us > 1000000) return MX_ERR_ARG;
  // one spin on every stream of `trial`, all waited for: wall time of the best of `rounds` rounds (four where a stream
  // may be new: its first launch binds its queue)
  int rc = MX_OK;
  auto spin_all = [&](const std::vector<int>& trial, int rounds = 4) -> double {
    double best = -1;
    for (int rep = 0; rep < rounds && rc == MX_OK; ++rep) {
      const auto t0 = std::chrono::steady_clock::now();
      for (int i : trial)
        if (rc == MX_OK) rc = mx_spin(spin_us, streams[i]);
      for (int i : trial)                                  // (also after a failed launch: nothing stays in flight)
        if (!hip_ok(hipStreamSynchronize((hipStream_t)streams[i])) && rc == MX_OK) rc = MX_ERR_HIP;
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (best < 0 || dt < best) best = dt;
    }
    return best;
  };
  MX_HIP(hipDeviceSynchronize());
  std::vector<int> accepted;
  double one = 0;      // what ONE spin costs here and now (launch + clock ramp included)
  for (int i = 0; i < n; ++i) {
    group_of[i] = i;
    if (accepted.empty()) {
      one = std::max(spin_all({i}), 1e-6 * (double)spin_us);
      if (rc != MX_OK) return rc;
      accepted.push_back(i);
      continue;
    }
    // side by side: about one spin; sharing a queue with an accepted stream: two
    std::vector<int> trial = accepted;
    trial.push_back(i);
    const bool beside = spin_all(trial) < 1.6 * one;
    if (rc != MX_OK) return rc;
    if (beside) { accepted.push_back(i); continue; }
    // whom it serialises with: halve the accepted streams (the half that still takes two spins together with stream i
    // holds the partner; the earlier half is asked first, so the first partner is found), then confirm the pair alone —
    // ceil(log2(accepted)) + 1 probes of two rounds, every stream's queue being bound by now
    size_t lo = 0, hi = accepted.size();
    while (hi - lo > 1) {
      const size_t mid = lo + (hi - lo) / 2;
      std::vector<int> half(accepted.begin() + lo, accepted.begin() + mid);
      half.push_back(i);
      const bool in_first = spin_all(half, 2) >= 1.6 * one;
      if (rc != MX_OK) return rc;
      if (in_first) hi = mid; else lo = mid;
    }
    const bool pair_serial = spin_all({accepted[lo], i}, 2) >= 1.6 * one;
    if (rc != MX_OK) return rc;
    group_of[i] = pair_serial ? accepted[lo] : -1;
  }
  return (int)accepted.size();
}

int mx_stream_create_cu_slice(int slice, int n_slices, int reserved, void** stream_out) {
  // CU mask bit i is CU (i / n_xcd) of XCD (i % n_xcd) (tools/ubench/cu_mask_probe.hip: 32 consecutive bits = 4 CUs
  // in each of the 8 XCDs; a mask that leaves an XCD without any CU is ignored by the runtime).  A slice is a
  // contiguous range of bits: the same CUs of every XCD.
  if (!stream_out || n_slices < 1 || slice < 0 || slice >= n_slices) return MX_ERR_ARG;
  int dev = 0, cus = 0;
  MX_HIP(hipGetDevice(&dev));
  MX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  if (cus < 32 * n_slices || n_slices > 8) return MX_ERR_ARG;      // at least 4 CUs per XCD and slice
  const int per = cus / n_slices, lo = slice * per, hi = slice == n_slices - 1 ? cus : lo + per;
  std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
  for (int i = lo; i < hi; ++i) mask[(size_t)i / 32] |= 1u << (i % 32);
  hipStream_t s = nullptr;
  (void)reserved;
  MX_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
  *stream_out = (void*)s;
  return MX_OK;
}

int mx_stream_destroy(void* stream) {
  if (!stream) return MX_ERR_ARG;
  MX_HIP(hipStreamDestroy((hipStream_t)stream));
  return MX_OK;
}

int mx_clock_probe(int64_t microseconds, uint64_t* d_ticks, void* stream) {
  if (microseconds <= 0 || microseconds > 1000000 || !d_ticks) return MX_ERR_ARG;
  touch_gpu();
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long)microseconds * 100ull,
                     (unsigned long long*)d_ticks);
  MX_HIP(hipGetLastError());
  return MX_OK;
}

int mx_selftest_lanes(void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int* d = nullptr;
  MX_HIP(hipMalloc(&d, sizeof(int)));
  int h = 0;
  hipError_t e = hipMemsetAsync(d, 0, sizeof(int), s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(lanes_selftest_kernel, dim3(1), dim3(64), 0, s, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  hipFree(d);
  MX_HIP(e);
  return h;
}

}  // extern "C"

// ---- sieve ---------------------------------------------------------------------------------
extern "C" int64_t mx_sieve_workspace_bytes(int limbs, int n_primes) {
  if (limbs <= 0 || n_primes <= 0) return MX_ERR_ARG;
  return mx::plan_sieve(limbs, n_primes).total;
}

extern "C" int mx_sieve(const uint32_t* d_cands, uint8_t* d_out, const uint32_t* h_primes, int n_primes, int limbs,
                        int64_t batch, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!d_cands || !d_out || !h_primes || !d_ws || limbs <= 0 || n_primes <= 0 || batch <= 0) return MX_ERR_ARG;
  if (limbs > 1024) return MX_ERR_SIZE;
  uint32_t top;
  if (!mx::sieve_primes_ok(h_primes, n_primes, top)) return MX_ERR_ARG;
  const mx::SievePlan p = mx::plan_sieve(limbs, n_primes);
  if (p.total > ws_bytes) return MX_ERR_WORKSPACE;
  return mx::run_sieve<false>(d_cands, d_out, h_primes, n_primes, top, limbs, batch, p, d_ws, (hipStream_t)stream);
}

// ---- share recombination -------------------------------------------------------------------
// constant rows of a key, each limbs2 words:
//   N | N^2 | theta_inv * R1 mod N | R2^k mod N^2 for k = 1 .. MX_COMBINE_NP_MAX
// R1 = 2^(W*L*nblk1) and R2 = 2^(W*L*nblk2) are the Montgomery radices of N and N^2 in the lane geometry of N^2.
// Row R2^np folds the np partials' way out of the Montgomery domain into one product (mx_combine.hpp); R2^2 is the
// conversion constant of the route for more partials than the plan has rows for.
constexpr int COMBINE_ROW_THETA = 2, COMBINE_ROW_RPOW = 3;
inline int64_t combine_plan_words(int limbs2) { return (int64_t)(COMBINE_ROW_RPOW + MX_COMBINE_NP_MAX) * limbs2; }

extern "C" int64_t mx_combine_plan_bytes(int limbs, int limbs2) {
  if (limbs <= 0 || limbs2 < limbs) return MX_ERR_ARG;
  return align256(combine_plan_words(limbs2) * 4);
}

namespace {
// the rows above into c (host), the bit lengths of N and N^2 into bits1 / bits2
int combine_constants(std::vector<u32>& c, int& bits1, int& bits2, const uint32_t* h_n, const uint32_t* h_theta_inv, int limbs,
                      int limbs2) {
  if (!h_n || !h_theta_inv) return MX_ERR_ARG;
  if (limbs <= 0 || limbs2 < limbs) return MX_ERR_ARG;
  if (!(h_n[0] & 1u)) return MX_ERR_MODULUS;
  bits1 = bit_length(h_n, limbs);
  if (bits1 < 2) return MX_ERR_MODULUS;
  std::vector<u32> n2((size_t)2 * limbs);
  mul_words(n2.data(), h_n, limbs, h_n, limbs);
  bits2 = bit_length(n2.data(), 2 * limbs);
  if ((bits2 + 31) / 32 > limbs2) return MX_ERR_ARG;   // rows too narrow for N^2
  Geometry g2;
  if (!choose_geometry(bits2, g2)) return MX_ERR_SIZE;
  Geometry g1 = g2;
  g1.nblk = (bits1 + 4 + g1.W * g1.L - 1) / (g1.W * g1.L);
  c.assign((size_t)combine_plan_words(limbs2), 0u);
  std::memcpy(&c[0], h_n, (size_t)limbs * 4);
  std::memcpy(&c[limbs2], n2.data(), (size_t)std::min(limbs2, 2 * limbs) * 4);
  {
    // theta_inv * R1 mod N: theta_inv reduced (a residue is expected, anything else is taken modulo N), then doubled
    std::vector<u32> q(limbs), t(limbs + 1, 0u);
    divmod_words(q.data(), t.data(), h_theta_inv, limbs, h_n, limbs);
    shl_mod(t, h_n, limbs, g1.W * g1.L * g1.nblk);
    std::memcpy(&c[(size_t)COMBINE_ROW_THETA * limbs2], t.data(), (size_t)limbs * 4);
  }
  {
    const u32* n2p = &c[limbs2];
    const int m = g2.W * g2.L * g2.nblk;
    std::vector<u32> x(limbs2 + 1, 0u);
    two_pow_mod(x.data(), n2p, limbs2, m);
    for (int k = 1; k <= MX_COMBINE_NP_MAX; ++k) {
      if (k > 1) shl_mod(x, n2p, limbs2, m);
      std::memcpy(&c[(size_t)(COMBINE_ROW_RPOW + k - 1) * limbs2], x.data(), (size_t)limbs2 * 4);
    }
  }
  return MX_OK;
}
}  // namespace

extern "C" int mx_combine_constants(const uint32_t* h_n, const uint32_t* h_theta_inv, int limbs, int limbs2, uint32_t* h_rows,
                                    int64_t rows_words) {
  if (!h_rows) return MX_ERR_ARG;
  std::vector<u32> c;
  int bits1 = 0, bits2 = 0;
  MX_TRY(combine_constants(c, bits1, bits2, h_n, h_theta_inv, limbs, limbs2));
  if ((int64_t)c.size() > rows_words) return MX_ERR_WORKSPACE;
  std::memcpy(h_rows, c.data(), c.size() * 4);
  return MX_OK;
}

extern "C" int mx_combine_prepare(mx_combine_plan* plan, const uint32_t* h_n, const uint32_t* h_theta_inv, int limbs,
                                  int limbs2, void* d_plan, int64_t plan_bytes, void* stream) {
  if (!plan || !d_plan) return MX_ERR_ARG;
  std::vector<u32> c;
  int bits1 = 0, bits2 = 0;
  MX_TRY(combine_constants(c, bits1, bits2, h_n, h_theta_inv, limbs, limbs2));
  if (mx_combine_plan_bytes(limbs, limbs2) > plan_bytes) return MX_ERR_WORKSPACE;
  MX_TRY(upload_words(d_plan, c.data(), c.size(), (hipStream_t)stream));
  plan->d_plan = d_plan;
  plan->plan_bytes = plan_bytes;
  plan->limbs = limbs;
  plan->limbs2 = limbs2;
  plan->n_bits = bits1;
  plan->n2_bits = bits2;
  return MX_OK;
}

extern "C" int mx_combine_run(const mx_combine_plan* plan, const uint32_t* d_partials, uint32_t* d_out, int out_stride,
                              uint8_t* d_status, int n_partials, int64_t batch, void* stream) {
  if (!plan || !plan->d_plan || !d_partials || !d_out) return MX_ERR_ARG;
  if (n_partials <= 0 || batch <= 0 || out_stride < plan->limbs) return MX_ERR_ARG;
  if (!d_status && out_stride == plan->limbs) return MX_ERR_ARG;      // the status must go somewhere
  Geometry g2;
  if (!choose_geometry(plan->n2_bits, g2)) return MX_ERR_SIZE;
  Geometry g1 = g2;
  g1.nblk = (plan->n_bits + 4 + g1.W * g1.L - 1) / (g1.W * g1.L);
  const int limbs2 = plan->limbs2;
  const u32* w = (const u32*)plan->d_plan;
  mx::CombineArgs a;
  a.partials = d_partials; a.out = d_out; a.status = d_status;
  a.n = w; a.n2 = w + limbs2; a.theta_r1 = w + COMBINE_ROW_THETA * (size_t)limbs2;
  // the plan's row for this many partials, or the two-conversion route through R2^2
  a.direct = n_partials <= MX_COMBINE_NP_MAX;
  a.rpow = w + (COMBINE_ROW_RPOW + (a.direct ? n_partials - 1 : 1)) * (size_t)limbs2;
  a.batch = batch; a.limbs = plan->limbs; a.limbs2 = limbs2; a.np = n_partials; a.out_stride = out_stride;
  a.nblk1 = g1.nblk; a.nblk2 = g2.nblk;
  hipStream_t s = (hipStream_t)stream;
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(g2.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    return launch_groups<K, LIMBS_PER_LANE>(mx::combine_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, a.batch, s, a);
  });
}

// ---- one-shot form: prepare into the workspace, run
extern "C" int64_t mx_combine_workspace_bytes(int limbs, int limbs2, int n_partials, int64_t batch) {
  if (limbs <= 0 || limbs2 < limbs || n_partials <= 0 || batch <= 0) return MX_ERR_ARG;
  return mx_combine_plan_bytes(limbs, limbs2);
}

extern "C" int mx_combine(const uint32_t* d_partials, uint32_t* d_out, uint8_t* d_status, const uint32_t* h_n,
                          const uint32_t* h_theta_inv, int limbs, int limbs2, int n_partials, int64_t batch,
                          void* d_ws, int64_t ws_bytes, void* stream) {
  if (!d_partials || !d_out || !d_status || !h_n || !h_theta_inv || !d_ws) return MX_ERR_ARG;
  if (limbs <= 0 || limbs2 < limbs || n_partials <= 0 || batch <= 0) return MX_ERR_ARG;
  mx_combine_plan plan;
  MX_TRY(mx_combine_prepare(&plan, h_n, h_theta_inv, limbs, limbs2, d_ws, ws_bytes, stream));
  return mx_combine_run(&plan, d_partials, d_out, limbs, d_status, n_partials, batch, stream);
}

// ---- biprimality verdict -------------------------------------------------------------------
extern "C" int64_t mx_verdict_workspace_bytes(int limbs, int n_parties, int64_t groups, int64_t n_slots) {
  if (limbs <= 0 || n_parties <= 0 || groups <= 0 || n_slots <= 0) return MX_ERR_ARG;
  return 2 * align256((int64_t)groups * limbs * 4);
}

extern "C" int mx_biprime_verdict_dev(const uint32_t* d_v, uint8_t* d_pass, const uint32_t* d_mods, int limbs,
                                      int mod_bits, int n_parties, int64_t groups, int64_t n_slots, void* d_ws,
                                      int64_t ws_bytes, void* stream) {
  if (!d_v || !d_pass || !d_mods || !d_ws || limbs <= 0 || n_parties <= 0 || groups <= 0 || n_slots <= 0)
    return MX_ERR_ARG;
  if (mod_bits < 2 || mod_bits > 32 * limbs) return MX_ERR_ARG;
  Geometry geo;
  if (!choose_geometry(mod_bits, geo)) return MX_ERR_SIZE;
  if (align256((int64_t)groups * limbs * 4) > ws_bytes) return MX_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  MX_TRY(launch_rmodn(geo, d_mods, (u32*)d_ws, limbs, groups, s));
  mx::VerdictArgs a;
  a.v = d_v; a.pass = d_pass; a.mods = d_mods; a.rmodn = (const u32*)d_ws;
  a.groups = groups; a.n_slots = n_slots; a.limbs = limbs; a.n_parties = n_parties; a.nblk = geo.nblk;
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(geo.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    return launch_groups<K, LIMBS_PER_LANE>(mx::verdict_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, a.groups * a.n_slots, s, a);
  });
}

extern "C" int mx_biprime_verdict(const uint32_t* d_v, uint8_t* d_pass, const uint32_t* h_mods, int limbs,
                                  int n_parties, int64_t groups, int64_t n_slots, void* d_ws, int64_t ws_bytes,
                                  void* stream) {
  if (!d_v || !d_pass || !h_mods || !d_ws || limbs <= 0 || n_parties <= 0 || groups <= 0 || n_slots <= 0)
    return MX_ERR_ARG;
  int max_bits = 0;
  for (int64_t g = 0; g < groups; ++g) {
    const u32* n = h_mods + g * limbs;
    if (!(n[0] & 1u)) return MX_ERR_MODULUS;
    int b = bit_length(n, limbs);
    if (b < 2) return MX_ERR_MODULUS;
    if (b > max_bits) max_bits = b;
  }
  int64_t part = align256((int64_t)groups * limbs * 4);
  if (2 * part > ws_bytes) return MX_ERR_WORKSPACE;
  char* ws = (char*)d_ws;
  MX_TRY(upload_words(ws, h_mods, (size_t)groups * limbs, (hipStream_t)stream));
  return mx_biprime_verdict_dev(d_v, d_pass, (const u32*)ws, limbs, max_bits, n_parties, groups, n_slots, ws + part,
                                ws_bytes - part, stream);
}

// ---- Jacobi symbol -------------------------------------------------------------------------
namespace {
template <int NL>
int launch_jacobi(const mx::JacobiArgs& a, hipStream_t s) {
  int64_t nblocks = a.skip ? (a.count / a.per_group) * ((a.per_group + 63) / 64) : (a.count + 63) / 64;
  // dynamic LDS: 0 except for the 257-word instance, whose top limbs live there (mx_jacobi.hpp)
  MX_TRY(mx_launch(mx::jacobi_kernel<NL>, nblocks, 64, mx::jacobi_lds_bytes<NL>(), s, a));
  // safety net for symbols the divstep kernel did not finish within its batch bound (mx_jacobi.hpp)
  constexpr size_t lds_fb = mx::jacobi_lds_bytes<NL, true>();
  if constexpr (lds_fb > 64 * 1024) {
    static bool allowed[MX_MAX_DEVICES] = {};
    MX_HIP(mx_allow_dynamic_lds(reinterpret_cast<const void*>(&mx::jacobi_fallback_kernel<NL>), (int)lds_fb, allowed));
  }
  return mx_launch(mx::jacobi_fallback_kernel<NL>, nblocks, 64, lds_fb, s, a);
}
}  // namespace

extern "C" int64_t mx_jacobi_workspace_bytes(int limbs, int64_t groups) {
  if (limbs <= 0 || groups <= 0) return MX_ERR_ARG;
  return align256((int64_t)groups * limbs * 4);
}

extern "C" int mx_jacobi_dev_range(const uint32_t* d_values, int8_t* d_out, const uint32_t* d_mods, int limbs,
                                   int64_t groups, int64_t group_size, int first, int count, const int32_t* d_skip_counts,
                                   int skip_threshold, void* stream) {
  if (!d_values || !d_out || !d_mods || limbs <= 0 || groups <= 0 || group_size <= 0) return MX_ERR_ARG;
  if (first < 0 || count <= 0 || (int64_t)first + count > group_size) return MX_ERR_ARG;
  if (limbs > 257) return MX_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream;
  mx::JacobiArgs a;
  a.a = d_values; a.mods = d_mods; a.out = (signed char*)d_out;
  a.count = groups * count; a.group_size = group_size; a.limbs = limbs;
  a.first = first; a.per_group = count; a.skip = d_skip_counts; a.skip_threshold = skip_threshold;
  a.max_batches = (32 * limbs * 9 / 2) / mx::JSTEPS + 8;
  if (g_knob_jacobi_max_batches > 0) a.max_batches = g_knob_jacobi_max_batches - 1;   // developer knob: exercises the safety net
  if (limbs <= 3) return launch_jacobi<3>(a, s);
  if (limbs <= 5) return launch_jacobi<5>(a, s);
  if (limbs <= 9) return launch_jacobi<9>(a, s);
  if (limbs <= 17) return launch_jacobi<17>(a, s);
  if (limbs <= 33) return launch_jacobi<33>(a, s);
  if (limbs <= 65) return launch_jacobi<65>(a, s);
  if (limbs <= 129) return launch_jacobi<129>(a, s);
  // key_length 8192 (the widest modulus the modexp kernels take for N^2): operands no longer fit the register file —
  // the limbs from 192 upwards live in LDS (mx_jacobi.hpp: jacobi_reg_limbs; one wavefront per SIMD, no scratch)
  return launch_jacobi<257>(a, s);
}

extern "C" int mx_jacobi_dev(const uint32_t* d_values, int8_t* d_out, const uint32_t* d_mods, int limbs,
                             int64_t groups, int64_t group_size, void* stream) {
  if (group_size > 0x7FFFFFFF) return MX_ERR_ARG;
  return mx_jacobi_dev_range(d_values, d_out, d_mods, limbs, groups, group_size, 0, (int)group_size, nullptr, 0, stream);
}

extern "C" int mx_jacobi(const uint32_t* d_values, int8_t* d_out, const uint32_t* h_mods, int limbs, int64_t groups,
                         int64_t group_size, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!d_values || !d_out || !h_mods || !d_ws || limbs <= 0 || groups <= 0 || group_size <= 0) return MX_ERR_ARG;
  if (limbs > 257) return MX_ERR_SIZE;
  for (int64_t g = 0; g < groups; ++g)
    if (!(h_mods[g * limbs] & 1u)) return MX_ERR_MODULUS;
  if (align256((int64_t)groups * limbs * 4) > ws_bytes) return MX_ERR_WORKSPACE;
  MX_TRY(upload_words(d_ws, h_mods, (size_t)groups * limbs, (hipStream_t)stream));
  return mx_jacobi_dev(d_values, d_out, (const u32*)d_ws, limbs, groups, group_size, stream);
}

// ---- modular multiplication ------------------------------------------------------------------
extern "C" int64_t mx_mulmod_workspace_bytes(int limbs) {
  if (limbs <= 0) return MX_ERR_ARG;
  return align256((int64_t)2 * limbs * 4);
}

extern "C" int mx_mulmod_shared(const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, const uint32_t* h_mod,
                                int limbs, int64_t batch, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!d_a || !d_b || !d_out || !h_mod || !d_ws || limbs <= 0 || batch <= 0) return MX_ERR_ARG;
  if (!(h_mod[0] & 1u)) return MX_ERR_MODULUS;
  int bits = bit_length(h_mod, limbs);
  if (bits < 2) return MX_ERR_MODULUS;
  Geometry geo;
  if (!choose_geometry(bits, geo)) return MX_ERR_SIZE;
  if (align256((int64_t)2 * limbs * 4) > ws_bytes) return MX_ERR_WORKSPACE;
  std::vector<u32> c((size_t)2 * limbs);
  std::memcpy(c.data(), h_mod, (size_t)limbs * 4);
  two_pow_mod(c.data() + limbs, h_mod, limbs, geo.W * geo.L * geo.nblk);
  hipStream_t s = (hipStream_t)stream;
  MX_TRY(upload_words(d_ws, c.data(), c.size(), s));
  mx::MulmodArgs a;
  a.a = d_a; a.b = d_b; a.out = d_out; a.mod = (const u32*)d_ws; a.rmodn = (const u32*)d_ws + limbs;
  a.batch = batch; a.limbs = limbs; a.nblk = geo.nblk;
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(geo.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    return launch_groups<K, LIMBS_PER_LANE>(mx::mulmod_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, a.batch, s, a);
  });
}

// ---- Shamir-field arithmetic of the candidate moduli ----------------------------------------------
namespace {
int field_launch(mx::FieldArgs& a, bool lincomb, const uint32_t* h_mod, const uint32_t* h_extra, int extra_words,
                 int limbs, void* d_ws, int64_t ws_bytes, hipStream_t s) {
  if (!(h_mod[0] & 1u)) return MX_ERR_MODULUS;
  int bits = bit_length(h_mod, limbs);
  if (bits < 2) return MX_ERR_MODULUS;
  Geometry geo;
  if (!choose_geometry(bits, geo)) return MX_ERR_SIZE;
  if (align256((int64_t)(2 * limbs + extra_words) * 4) > ws_bytes) return MX_ERR_WORKSPACE;
  std::vector<u32> c((size_t)2 * limbs + extra_words);
  std::memcpy(c.data(), h_mod, (size_t)limbs * 4);
  two_pow_mod(c.data() + limbs, h_mod, limbs, geo.W * geo.L * geo.nblk);
  if (extra_words) std::memcpy(c.data() + 2 * limbs, h_extra, (size_t)extra_words * 4);
  MX_TRY(upload_words(d_ws, c.data(), c.size(), s));
  a.mod = (const u32*)d_ws; a.rmodn = (const u32*)d_ws + limbs;
  if (lincomb) a.b = (const u32*)d_ws + 2 * limbs;
  a.limbs = limbs; a.nblk = geo.nblk;
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32, 64>(geo.K, [&](auto k) {
    constexpr int K = decltype(k)::value;
    return lincomb ? launch_groups<K, LIMBS_PER_LANE>(mx::lincomb_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, a.batch, s, a)
                   : launch_groups<K, LIMBS_PER_LANE>(mx::fma_kernel<K, LIMBS_PER_LANE, LIMB_BITS>, a.batch, s, a);
  });
}
}  // namespace

extern "C" int64_t mx_field_workspace_bytes(int limbs, int terms) {
  if (limbs <= 0 || terms < 0) return MX_ERR_ARG;
  return align256((int64_t)(2 + terms) * limbs * 4);
}

extern "C" int mx_fma_mod(const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_c, uint32_t* d_out,
                          const uint32_t* h_mod, int limbs, int64_t batch, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!d_a || !d_b || !d_c || !d_out || !h_mod || !d_ws || limbs <= 0 || batch <= 0) return MX_ERR_ARG;
  mx::FieldArgs a;
  a.a = d_a; a.b = d_b; a.c = d_c; a.out = d_out; a.batch = batch; a.terms = 0;
  return field_launch(a, false, h_mod, nullptr, 0, limbs, d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int mx_lincomb_mod(const uint32_t* d_x, const uint32_t* h_coeffs, uint32_t* d_out, const uint32_t* h_mod,
                              int limbs, int terms, int64_t batch, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!d_x || !h_coeffs || !d_out || !h_mod || !d_ws || limbs <= 0 || terms <= 0 || batch <= 0) return MX_ERR_ARG;
  mx::FieldArgs a;
  a.a = d_x; a.b = nullptr; a.c = nullptr; a.out = d_out; a.batch = batch; a.terms = terms;
  return field_launch(a, true, h_mod, h_coeffs, terms * limbs, limbs, d_ws, ws_bytes, (hipStream_t)stream);
}

// ---- modular inverse (one wavefront per element) ---------------------------------------------------
namespace {
template <int LPL>
int launch_modinv(const mx::ModinvArgs& a, hipStream_t s) {
  return mx_launch(mx::modinv_kernel<LPL>, a.batch, 64, 0, s, a);
}
}  // namespace

extern "C" int64_t mx_modinv_workspace_bytes(int limbs) {
  if (limbs <= 0) return MX_ERR_ARG;
  return align256((int64_t)limbs * 4);
}

extern "C" int mx_modinv(const uint32_t* d_values, uint32_t* d_out, uint8_t* d_status, const uint32_t* h_mod, int limbs,
                         int64_t batch, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!d_values || !d_out || !d_status || !h_mod || !d_ws || limbs <= 0 || batch <= 0) return MX_ERR_ARG;
  if (!(h_mod[0] & 1u)) return MX_ERR_MODULUS;
  const int bits = bit_length(h_mod, limbs);
  if (bits < 2) return MX_ERR_MODULUS;
  if (bits > MAX_MOD_BITS) return MX_ERR_SIZE;
  if (align256((int64_t)limbs * 4) > ws_bytes) return MX_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  MX_TRY(upload_words(d_ws, h_mod, (size_t)limbs, s));
  mx::ModinvArgs a;
  a.vals = d_values; a.mod = (const u32*)d_ws; a.out = d_out; a.status = d_status; a.batch = batch; a.limbs = limbs;
  // the almost-inverse keeps values below 2 M, the word-wise halvings form x + q M with a one-word q: capacity
  // 64 * LPL words >= bits + 34 bits, and >= limbs words
  const int need = std::max(limbs, (bits + 34 + 31) / 32);
  if (need <= 64) return launch_modinv<1>(a, s);
  if (need <= 128) return launch_modinv<2>(a, s);
  if (need <= 192) return launch_modinv<3>(a, s);
  if (need <= 320) return launch_modinv<5>(a, s);
  if (need <= 576) return launch_modinv<9>(a, s);
  return MX_ERR_SIZE;
}

// ---- selection of the Jacobi-1 generators ---------------------------------------------------
extern "C" int mx_select_first(const uint32_t* d_rows, const int8_t* d_flags, uint32_t* d_out, int32_t* d_counts,
                               int limbs, int64_t groups, int group_size, int keep, void* stream) {
  if (!d_rows || !d_flags || !d_out || !d_counts || limbs <= 0 || groups <= 0 || group_size <= 0 || keep <= 0)
    return MX_ERR_ARG;
  mx::SelectArgs a;
  a.rows = d_rows; a.flags = (const signed char*)d_flags; a.out = d_out; a.counts = d_counts;
  a.groups = groups; a.group_size = group_size; a.keep = keep; a.limbs = limbs;
  return mx_launch(mx::select_first_kernel, groups, 64, 0, (hipStream_t)stream, a);
}

