// extern "C" entry points of the N^2-modulus modexp (second translation unit of libmxpaillier.so:
// compiled in parallel with mx_capi.hip, the pair kernels are the most expensive to build).
#include <cmath>
#include "mx_launch.hpp"
#include "mx_upload.hpp"
#include "mx_powmod_n2_split.hpp"
#include "mx_bipair.hpp"
#include "mx_multiexp_n2.hpp"
#include "mx_matmul_n2.hpp"
#include "mx_pack_n2.hpp"
#include "mx_fixedbase_n2.hpp"
#include "mx_hist_n2.hpp"
#include "mx_scan_n2.hpp"

// ---- modexp modulo N^2 through pairs modulo N --------------------------------------------------
namespace {
// Shape of one launch: geometry, grid, table of pair slots in the caller's workspace.
struct N2Shape {
  Geometry geo;
  int64_t nblocks = 0, nlanes = 0;
  int nslots = 0;
  int64_t table_bytes = 0;
  int64_t groups = 0;          // groups of elements (one per wavefront or pair of wavefronts)
  int64_t sched_bytes = 0;     // scheduling words of the time-sliced form, behind the table in the workspace
};

// limbs_per_lane values of the pair kernel: 9 and 18 in both forms (one or two wavefronts per group of
// elements), 3 — the latency geometry — only in the two-wavefront form (mx_powmod_n2_split.hpp).  (2 limbs per
// lane were tried too: fewer instructions per limb step, but the quotient digit then travels through an SGPR
// (v_readfirstlane for 64-lane groups) and the dependent chain got longer, 18.5 vs 16.8 ms for one ciphertext.)
constexpr int N2_GEOS = 3;                      // constant sets of a plan, in geo_index order
constexpr int N2_LPLS[N2_GEOS] = {LIMBS_PER_LANE, LIMBS_PER_LANE_WIDE, LIMBS_PER_LANE_LAT};
inline int geo_index(int lpl) {
  for (int g = 0; g < N2_GEOS; ++g) if (N2_LPLS[g] == lpl) return g;
  return -1;
}
inline int max_lanes(int lpl, int wpg) {
  if (lpl == LIMBS_PER_LANE_WIDE) return 16;
  if (lpl == LIMBS_PER_LANE) return 32;
  return wpg == 2 ? 64 : 0;                 // L = 3 exists as a split kernel only
}

constexpr int N2_TIMESLICE_MAX_SEGMENTS = mx::N2_TS_LEVELS;      // units per group of a time-sliced launch, at most

// table_rows: pair slots of the table region (2^(window - 1) odd powers for a classic tape; the shape queries pass 1)
bool shape_n2(int n_bits, int table_rows, int64_t batch, int limbs_per_lane, int wpg, N2Shape& p) {
  if (wpg == 4) {                                                // the five-wavefront latency form (mx_bipair.hpp) shares the
    if (limbs_per_lane != LIMBS_PER_LANE_LAT) return false;      // slots of the two-wavefront 3-limb form
    wpg = 2;
  }
  if (geo_index(limbs_per_lane) < 0 || (wpg != 1 && wpg != 2)) return false;
  if (!choose_geometry(n_bits, p.geo, limbs_per_lane)) return false;
  if (p.geo.K > max_lanes(limbs_per_lane, wpg)) return false;   // instances that exist
  int gpw = (64 / p.geo.K) * (wpg == 2 ? mx::N2_SPLIT_PAIRS : 1);      // elements per workgroup
  p.nblocks = (batch + gpw - 1) / gpw;
  p.nlanes = p.nblocks * 64 * (wpg == 2 ? mx::N2_SPLIT_PAIRS : 1);
  p.nslots = mx::N2_SLOT_TABLE + table_rows;
  p.table_bytes = align256((int64_t)p.nslots * 2 * p.geo.L * p.nlanes * 4);
  p.groups = (batch + 64 / p.geo.K - 1) / (64 / p.geo.K);
  p.sched_bytes = wpg == 2 ? align256((mx::N2_TS_HEADER + p.groups * (N2_TIMESLICE_MAX_SEGMENTS - 1)) * 4) : 0;
#ifdef MX_DEV_TS_TRACE          // four words per unit behind the queues (mx_powmod_n2_split.hpp)
  if (wpg == 2) p.sched_bytes += align256(p.groups * N2_TIMESLICE_MAX_SEGMENTS * 16);
#endif
  return true;
}

}  // namespace
// wide-geometry instantiations live in mx_capi_n2w.hip, the two-wavefront kernels in mx_capi_n2s.hip (L = 3, 9) and
// mx_capi_n2sw.hip (L = 18): translation units of their own, built in parallel
namespace mxw { int launch_n2_wide(int K, const mx::PowmodN2Args& a, int64_t nblocks, hipStream_t s); }
namespace mxs {
int launch_n2_split(int K, int L, bool timesliced, const mx::PowmodN2Args& a, int64_t nblocks, hipStream_t s);
int launch_n2_split_wide(int K, bool timesliced, const mx::PowmodN2Args& a, int64_t nblocks, hipStream_t s);
}
namespace mxb {
bool n2_bipair_instance(int K);
int launch_n2_bipair(int K, const mx::PowmodBiPairArgs& a, int64_t nblocks, hipStream_t s);
}
namespace mxl { int launch_bisetup(int K, const mx::BiSetupArgs& a, hipStream_t s); }
namespace {
int launch_n2(const mx::PowmodN2Args& a, const N2Shape& p, int wpg, hipStream_t s, int64_t timesliced_blocks = 0) {
  const int K = p.geo.K, L = p.geo.L;
  if (wpg == 2) {
    const bool ts = timesliced_blocks > 0;
    const int64_t nb = ts ? timesliced_blocks : p.nblocks;
    return L == LIMBS_PER_LANE_WIDE ? mxs::launch_n2_split_wide(K, ts, a, nb, s) : mxs::launch_n2_split(K, L, ts, a, nb, s);
  }
  if (L == LIMBS_PER_LANE_WIDE) return mxw::launch_n2_wide(K, a, p.nblocks, s);
  return mx_dispatch_lanes<1, 2, 4, 8, 16, 32>(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    return mx_launch(mx::powmod_n2_kernel<KK, LIMBS_PER_LANE, LIMB_BITS>, p.nblocks, 64, mx::powmod_n2_lds_bytes<KK, LIMBS_PER_LANE>(), s, a);
  });
}

// Which instances run their tape modulo the friendly multiple of N (mx_powmod_n2.hpp): every 3-limb instance (its
// geometry reserves the room), the 9-limb two-wavefront instances for groups of 8 and 16 lanes and the 18-limb
// one-wavefront instances for groups of 4 and 8 lanes (key_length 2048 and 4096) where the modulus leaves LIMB_BITS + 6
// bits of room in R.  One place decides; the launchers of the other translation units obey PowmodN2Args::friendly.
inline bool n2_friendly_instance(const Geometry& g, int wpg, int n_bits) {
  if (g.L == LIMBS_PER_LANE_LAT) return true;
  if (n_bits + 4 + LIMB_BITS + 2 > g.W * g.L * g.nblk) return false;
  if (wpg == 2) return g.L == LIMBS_PER_LANE && (g.K == 8 || g.K == 16);
  return g.L == LIMBS_PER_LANE_WIDE && (g.K == 4 || g.K == 8) && g_knob_n2_friendly_1w != 1;
}

// Launch shape of the pair kernel when the caller leaves the choice (limbs per lane and/or wavefronts per
// group) to the library: the candidate with the lowest estimated duration for ONE launch of this batch on an
// otherwise idle GPU.  The estimate is a cycle count per pair operation for the wavefront that bounds the launch,
// fitted to tools/sweep_shapes.py (profiles/r03_sweep_shapes.txt; within ~8 % of every measured point at
// key_length 2048 and 4096):
//   a limb step is m multiply-accumulates plus o other instructions (quotient digit, carry hand-over, shifts);
//   a wavefront that has its SIMD to itself issues one instruction every ~5.3 cycles whatever it is, and waits
//   ~80 / L cycles per step for the multiplier limbs it fetches from LDS once per L steps;
//   every further wavefront resident on the same SIMD adds what its instructions cost when the SIMD is shared:
//   4.2 cycles per multiply-accumulate, 2.3 per other instruction (tools/ubench/valu_peak.hip);
//   wavefronts beyond what the register file holds per SIMD (2 at L = 18, 3 at L = 9, 8 at L = 3) are back-filled
//   as the first ones finish.
// Two-wavefront groups: the second pass (m = 2L, o = 11) bounds an operation, its wavefronts sit on SIMDs 1 and 3 of
// a CU, one per workgroup.  One-wavefront groups: both passes (m = L/2 + 1 + 3L, o = 20), a wavefront per workgroup.
// What comes out (key_length 2048): up to ~1000 ciphertexts the latency geometry (3 limbs per lane, two
// wavefronts), to ~4000 L = 9 split, to ~8000 L = 18 split, and the one-wavefront wide kernel once a launch
// fills the machine on its own (from ~24 000).  Callers that keep several launches in flight fill the machine
// between them and should say so by passing limbs_per_lane = 18, wavefronts_per_group = 1 (bench.py's
// steady-state leg does).
struct N2Choice { int lpl, wpg, resident, units; };      // resident: workgroups per CU of the time-sliced form (0 = plain launch), units per group unless the caller says
inline int device_cus() { return mx_device_cus(); }      // of the CURRENT device (mx_upload.hpp)
double n2_estimate(int n_bits, int64_t batch, int lpl, int wpg, int* resident = nullptr, int* units = nullptr) {
  if (resident) *resident = 0;
  if (units) *units = 0;
  N2Shape p;
  if (!shape_n2(n_bits, 1, batch, lpl, wpg, p)) return -1.0;
  const double L = p.geo.L, steps = (double)p.geo.nblk * p.geo.L;
  // (3 limbs per lane: the friendly-modulus passes have 8 other instructions per step, and a second wavefront on
  // the SIMD costs them 1.22x what the issue costs alone would say — 13.0 / 19.9 / 27.4 / 35.3 ms for 1 .. 4 per SIMD)
  const bool lat = lpl == LIMBS_PER_LANE_LAT;
  const double m = wpg == 2 ? 2 * L : (p.geo.L / 2 + 1) + 3 * L, o = lat ? 8.0 : wpg == 2 ? 11.0 : 20.0;
  // (round 5 refit, after the build's alignment pass: a lone 18-limb wavefront runs 3 % / 8 % faster than these counts
  // say — 32.1 ms for 8192 ciphertexts on two wavefronts, 54.4 for 16 384 on one — and a second 9-limb pair on a SIMD
  // costs 8 % more (35.6 ms for 8192), a second 18-limb pair 18 % more (59.5 ms for 16 384); profiles/r05_ts_probe_2048.txt,
  // r05_sweep_shapes.txt)
  const bool wide_geo = lpl == LIMBS_PER_LANE_WIDE;
  const double alone = steps * (5.3 * (m + o) + 80.0 / L) * (wide_geo ? (wpg == 2 ? 0.967 : 0.924) : 1.0);
  const double shared = steps * (4.2 * m + 2.3 * o) * (lat ? 1.22 : wpg == 2 ? (wide_geo ? 1.18 : 1.08) : 1.17);     // one wavefront doing both passes overlaps less
  const int cus = device_cus();
  const int64_t per_simd = wpg == 2 ? (p.nblocks + cus - 1) / cus : (p.nblocks + 4 * cus - 1) / (4 * cus);
  const int64_t fit = lpl == LIMBS_PER_LANE_WIDE ? 2 : lpl == LIMBS_PER_LANE ? 3 : 8;
  // every further wavefront of a two-wavefront shape costs ~12 % more than the one before (L9: 21.3 / 35.7 / 51.1 ms
  // for 1 / 2 / 3 per SIMD; L3: increments of 7.4, 8.1, 8.9 ms)
  auto round = [&](int64_t r) {
    double t = r <= 0 ? 0.0 : alone, add = shared;
    for (int64_t k = 1; k < r; ++k) { t += add; if (wpg == 2) add *= 1.12; }
    return t;
  };
  double plain;
  if (per_simd <= fit) {
    plain = round(per_simd);          // everything resident at once: the fullest SIMD bounds the launch
  } else {
    // more wavefronts than fit: every further one per SIMD (whole ones: the fullest SIMD bounds the launch) adds
    // 0.93 of its share of a full round — measured at 9 limbs per lane, two-wavefront groups: 53.4 ms for 3 per
    // SIMD, then 70 / 86.5 / 102.5 for 4 / 5 / 6; at 18: 59.9 for 2, 89 for 3, 115 for 4
    plain = round(fit) * (1.0 + 0.93 * (double)(per_simd - fit) / (double)fit);
  }
  // Time-sliced form (mx_powmod_n2_split.hpp; instances: 9 limbs per lane, groups of at most 16 lanes): r workgroups
  // per CU stay resident and take the groups' segments from a queue.  Measured over r = 1..3 and 2..8 segments at
  // key_length 2048 and 4096 (tools/ts_probe.py, profiles/r03_ts_probe_*.txt), two settings pay:
  //   r = 2 with 2 segments: the launch costs groups / resident pairs x a full launch of 2 per SIMD (when a wavefront
  //     runs out of work its neighbour speeds up, so the coarse grain costs nothing) — 44-47 ms instead of 54 for
  //     9 200..10 500 ciphertexts at key_length 2048;
  //   r = 1 with 8 segments, for launches just above one workgroup per CU (up to 1.25x): the fine grain costs ~13 %
  //     per operation (hand-overs on a SIMD that has nothing else to issue), still 12-23 % below the plain launch.
  const bool wide = lpl == LIMBS_PER_LANE_WIDE;
  const bool sliceable = wpg == 2 && ((lpl == LIMBS_PER_LANE && p.geo.K <= 16) || (wide && (p.geo.K == 4 || p.geo.K == 8)));
  if (!sliceable || !resident || g_knob_n2_timeslice == 1) return plain;
  const bool forced = g_knob_n2_timeslice >= 2;
  double best = forced ? -1.0 : plain * 0.97;          // a time-sliced launch has to win by 3 %
  int best_units = 0;
  if (wide) {
    // 18 limbs per lane (round 5): ONE workgroup per CU — a second one doubles what every SIMD carries — and the groups'
    // units handed out most-work-left-first (mx_powmod_n2_split.hpp): the launch takes ceil(groups x units / pairs)
    // rounds of 1 / units of a full launch, plus 0.4 % per unit for the hand-overs (key_length 2048: 8704 ciphertexts
    // in 12 units 36.1 ms, 10 000 in 8 units 40.8, 11 264 in 8 units 45.2, 12 288 in 2 units 47.9 where the plain
    // launches take 51-60; key_length 4096: 4352 in 12 units 141 ms, 5000 in 8 units 151, 5632 in 8 units 166 where they
    // take 182; profiles/r05_ts_probe_*.txt).  Four units are not offered: 10 000 ciphertexts are 4.88 rounds of them, and
    // whether the launch then takes five or six (42 or 49 ms) changed from build to build.
    const int64_t pairs = (int64_t)cus * mx::N2_SPLIT_PAIRS;
    if (p.groups > pairs || forced) {
      for (int u : {2, 8, 12}) {
        const int64_t rounds = (p.groups * u + pairs - 1) / pairs;
        const double t = round(1) * (double)rounds / (double)u * (1.0 + 0.004 * u);
        if (best < 0 || t < best) { best = t; best_units = u; *resident = 1; }
      }
    }
    if (units) *units = best_units;
    return *resident ? best : plain;
  }
  for (int64_t r = 1; r <= 2; ++r) {
    int64_t rr = r;
    if (g_knob_n2_timeslice > 16) {               // developer: this many per CU
      if (r != 1) break;
      rr = std::min<int64_t>(fit, g_knob_n2_timeslice - 16);
    }
    const int64_t pairs = rr * cus * mx::N2_SPLIT_PAIRS;
    if (p.groups <= pairs && !forced) continue;
    const double load = std::max(1.0, (double)p.groups / (double)pairs);
    if (rr == 1 && load > 1.5 && !forced) continue;
    // the time-sliced instances run 5 % (shared SIMDs) to 11 % (alone) slower per operation than the plain ones since
    // the build aligns 64-bit instructions (asm_align.py: the plain instances gained, these did not), and one
    // workgroup per CU pays ~13 % for its hand-overs
    // (two per CU, two units: 1.19-1.26 x a full launch for loads of 1.03-1.25 — 42-45 ms for 8448 .. 10 240 ciphertexts)
    const double t = (rr == 2 ? std::max(load, 1.17) : load) * round(rr) * (rr == 1 ? 1.28 : 1.05);
    if (best < 0 || t < best) { best = t; *resident = (int)rr; best_units = rr == 1 ? 8 : 2; }
  }
  if (units) *units = best_units;
  return *resident ? best : plain;
}
bool bipair_geometry(int n_bits, Geometry& gb);
// The candidate shapes that the caller's limbs_per_lane and wavefronts per group (0: any) leave open, each given to
// `estimate` (which may fill in the time-sliced fields of its candidate): the one with the lowest estimate above 0 into
// `best`; false where no candidate has an instance.
template <class F>
bool n2_best_candidate(int limbs_per_lane, int wpg, N2Choice& best, F&& estimate) {
  double best_t = -1.0;
  for (int l : N2_LPLS) {
    if (limbs_per_lane && l != limbs_per_lane) continue;
    for (int w : {1, 2}) {
      if (wpg && w != wpg) continue;
      N2Choice c{l, w, 0, 0};
      const double t = estimate(c);
      if (t > 0 && (best_t < 0 || t < best_t)) { best_t = t; best = c; }
    }
  }
  return best_t >= 0;
}
N2Choice n2_auto_shape(int n_bits, int64_t batch, int limbs_per_lane, int wpg) {
  if (wpg == 4) return N2Choice{LIMBS_PER_LANE_LAT, 4, 0, 0};      // explicit: the five-wavefront latency form (mx_bipair.hpp)
  N2Choice best{LIMBS_PER_LANE, 1, 0, 0};
  if (!n2_best_candidate(limbs_per_lane, wpg, best, [&](N2Choice& c) { return n2_estimate(n_bits, batch, c.lpl, c.wpg, &c.resident, &c.units); }))
    best = N2Choice{limbs_per_lane ? limbs_per_lane : LIMBS_PER_LANE, wpg ? wpg : 1, 0, 0};   // reported as MX_ERR_SIZE by the caller
  // Launches that the two-wavefront latency form would run with at most ONE workgroup of the five-wavefront form per compute
  // unit take that form where it exists (key_length 1024 / 2048 / 4096): both passes of every product on two wavefronts each,
  // 9.4 instead of 12.95 ms for 1 .. 512 ciphertexts at key_length 2048, 31.8 instead of 47 for 1 .. 256 at 4096
  // (tools/lone_decrypt_time.py, profiles/r06_lone_decrypt.txt); a second workgroup per unit costs more than it saves.
  if (wpg == 0 && best.lpl == LIMBS_PER_LANE_LAT && best.wpg == 2 && g_knob_n2_bipair != 1) {
    Geometry gb;
    if (bipair_geometry(n_bits, gb) && batch <= (int64_t)device_cus() * (64 / gb.K)) best.wpg = 4;
  }
  return best;
}

// Segments when the caller leaves the choice to the library: a launch whose wavefronts would live for
// tens of milliseconds is cut so that a burst of such launches drains at a finer grain (measured with
// bench.py --steps 20: the last round of 4 launches in flight costs ~3 % of the run unsegmented).
int n2_auto_segments(int n_sqr, int64_t nblocks) {
  if (g_knob_n2_segments >= 1) return g_knob_n2_segments;
  return (n_sqr >= 2048 && nblocks >= 256) ? 4 : 1;
}

inline int64_t n2_consts_words(int limbs_n) { return (int64_t)8 * limbs_n + 2 * (limbs_n + 1); }
inline int64_t n2_consts_bytes(int limbs_n) { return align256(n2_consts_words(limbs_n) * 4); }

// The five-wavefront latency form (mx_bipair.hpp): exists where the bipartite geometry of the modulus (mx_host.hpp: the
// pivot, Pd data positions) and the pair kernel's 3-limb geometry agree on lanes and blocks, and the kernel is instantiated.
bool bipair_geometry(int n_bits, Geometry& gb) {
  Geometry g3;
  if (!choose_geometry(n_bits, gb, LIMBS_PER_LANE_BI) || !choose_geometry(n_bits, g3, LIMBS_PER_LANE_LAT)) return false;
  if (gb.K != g3.K || gb.nblk != g3.nblk || !mxb::n2_bipair_instance(gb.K)) return false;
  const int pd = gb.L * gb.nblk;
  // The pivot of the PAIR form (tools/bipair_model.py: pair_geometry): 0.52 of the steps on the L wavefronts, to the nearest
  // block — 21 of 42 at key_length 1024, 39 of 75 at 2048, 75 of 147 at 4096.  The generic form's pivot (mx_host.hpp: 24, 39,
  // 54) is fitted to ITS halves; here the H wavefronts record fold digits or carry two product rows, and at K = 64 its 54
  // left the L wavefronts waiting for 45 % of every slot (tools/bp_phase_probe.py; one decrypt 38.9 -> 31.5 ms, 3.55 -> 3.27 ms
  // at key_length 1024; profiles/r06_bipair_pivot_sweep.txt).
  if (g_knob_bi_pivot <= 0) {
    const int steps = pd + gb.L;
    int h = gb.L * ((52 * steps + 150) / (100 * gb.L));
    if (h > steps - gb.L) h = steps - gb.L;
    if (h < gb.L) h = gb.L;
    const int lo_min = gb.L * ((pd - (n_bits - 2) / gb.W + gb.L - 1) / gb.L);
    if (h < lo_min) h = lo_min;
    gb.h_lo = h;
  }
  return gb.h_lo < pd && LIMB_BITS * (pd - gb.h_lo) < n_bits - 1;      // E = 2^(W (Pd - hL)) is a digit below N
}
// its section of a plan's device block, behind the tape: constants for R' = 2^(W hL) | fold rows | quotient rows
inline int64_t bipair_fold_bytes() { return align256((int64_t)mx::BI_ROWS * 3 * 64 * 4); }
inline int64_t bipair_quot_bytes() { return align256((int64_t)mx::BP_QROWS * 3 * 64 * 4); }
inline int64_t bipair_section_bytes(int limbs_n) { return n2_consts_bytes(limbs_n) + bipair_fold_bytes() + bipair_quot_bytes(); }
inline int64_t bipair_section_offset(int limbs_n) { return N2_GEOS * n2_consts_bytes(limbs_n) + align256((int64_t)MAX_SLIDING_OPS * 4); }
// the lifted tape of a plan (mx_nsquare_plan::lift), behind that section: the layout in front of it is that of older plans
inline int64_t n2_tape_bytes() { return align256((int64_t)MAX_SLIDING_OPS * 4); }
inline int64_t lifted_tape_offset(int limbs_n) { return bipair_section_offset(limbs_n) + bipair_section_bytes(limbs_n); }
constexpr int N2_GEO_BIPAIR = 8;      // mx_nsquare_plan::geometries: the plan holds the constants of the five-wavefront form
constexpr int N2_GEO_PIVOT_SHIFT = 8; // ... and, in bits 8-15, the pivot those constants were built with (0: a plan of an older library)

// One resolved launch of the N^2 modexp: what the shape queries and mx_powmod_nsquare_run read their answers from.
struct N2Launch {
  N2Choice ch;            // limbs per lane, wavefronts per group, residents and units of the time-sliced form
  N2Shape p;              // (five-wavefront form: the shape of the two-wavefront 3-limb form, whose slots and lanes it shares)
  bool friendly = false;  // the instance runs its tape modulo the friendly multiple of N
  Geometry bi;            // five-wavefront form only: its geometry, h_lo the pivot of the knob
};
// Refuses, in this order: a batch, limbs_per_lane or wavefronts_per_group that no launch takes (MX_ERR_ARG), then a
// combination without an instance for this modulus (MX_ERR_SIZE).
int resolve_n2(int n_bits, int64_t batch, int limbs_per_lane, int wpg, int table_rows, N2Launch& r) {
  if (batch <= 0) return MX_ERR_ARG;
  if (limbs_per_lane != 0 && geo_index(limbs_per_lane) < 0) return MX_ERR_ARG;
  if (wpg < 0 || (wpg > 2 && wpg != 4)) return MX_ERR_ARG;
  if (wpg == 4 && limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE_LAT) return MX_ERR_SIZE;      // explicit only with 3 limbs
  r.ch = n2_auto_shape(n_bits, batch, limbs_per_lane, wpg);
  if (r.ch.wpg == 4 && !bipair_geometry(n_bits, r.bi)) return MX_ERR_SIZE;
  if (!shape_n2(n_bits, table_rows, batch, r.ch.lpl, r.ch.wpg, r.p)) return MX_ERR_SIZE;
  r.friendly = r.ch.wpg == 4 || n2_friendly_instance(r.p.geo, r.ch.wpg, n_bits);
  return MX_OK;
}


// The eight constant rows of one geometry (R = 2^m), each limbs_n words:
//   N | ONE0 ONE1 | K1_0 K1_1 | K2_0 K2_1 | C'
// followed by two rows of limbs_n + 1 words for the passes modulo the friendly multiple N~ = u N, u = -N^-1 mod 2^W
// (mx_powmod_n2.hpp; read by the 3-limb instances):
//   N~ + 1 | C2' = C2 - u (R - 1),  C2 = N * ceil(u (R - 1) / N)
void n2_constants(u32* c, const u32* h_n, int limbs_n, int m, int k) {
  const int l2 = 2 * limbs_n;
  std::vector<u32> n2(l2), tmp(l2), qq(l2), rr(limbs_n);
  mul_words(n2.data(), h_n, limbs_n, h_n, limbs_n);
  std::memset(c, 0, (size_t)n2_consts_words(limbs_n) * 4);
  std::memcpy(&c[0], h_n, (size_t)limbs_n * 4);
  auto pair_of = [&](int pow2, int row) {                      // N-adic digits of 2^pow2 mod N^2
    pow2_mod(tmp.data(), n2.data(), l2, pow2);
    divmod_words(qq.data(), rr.data(), tmp.data(), l2, h_n, limbs_n);
    std::memcpy(&c[(size_t)row * limbs_n], rr.data(), (size_t)limbs_n * 4);          // digit 0
    std::memcpy(&c[(size_t)(row + 1) * limbs_n], qq.data(), (size_t)limbs_n * 4);    // digit 1 (< N)
  };
  pair_of(m, 1);              // represents 1      (rho * V = 1  ->  V = R)
  pair_of(2 * m, 3);          // represents R      (V = R^2)
  pair_of(2 * m + k, 5);      // represents 2^k R  (V = 2^k R^2)
  // C' = N*ceil(R/N) - R + 1 = N - (R mod N) + 1   (R mod N != 0 as N is odd > 1)
  pow2_mod(rr.data(), h_n, limbs_n, m);          // (R below N for the five-wavefront form: R = 2^(W hL))
  u64 borrow = 0, carry = 1;
  u32* cp = &c[(size_t)7 * limbs_n];
  for (int i = 0; i < limbs_n; ++i) {
    u64 d = (u64)h_n[i] - rr[i] - borrow;
    borrow = (d >> 63) & 1;
    u64 e = (u64)(u32)d + carry;
    cp[i] = (u32)e;
    carry = e >> 32;
  }
  // ---- friendly rows
  u32 inv = h_n[0];                                            // Newton: N^-1 mod 2^32
  for (int i = 0; i < 5; ++i) inv *= 2u - h_n[0] * inv;
  const u32 u = (0u - inv) & ((1u << LIMB_BITS) - 1u);
  u32* nt = &c[(size_t)8 * limbs_n];
  mul_words(nt, h_n, limbs_n, &u, 1);                          // N~ = u N  (limbs_n + 1 words), = -1 mod 2^W
  for (int i = 0; i <= limbs_n; ++i) { if (++nt[i] != 0u) break; }      // + 1
  // C2' = (u (1 - R)) mod N = (u * ((N + 1 - R mod N) mod N)) mod N = (u C') mod N      (R mod N != 0)
  std::vector<u32> prod(limbs_n + 1), quo(limbs_n + 1), rem(limbs_n);
  mul_words(prod.data(), cp, limbs_n, &u, 1);
  divmod_words(quo.data(), rem.data(), prod.data(), limbs_n + 1, h_n, limbs_n);
  std::memcpy(&c[(size_t)8 * limbs_n + (limbs_n + 1)], rem.data(), (size_t)limbs_n * 4);
}
}  // namespace

extern "C" int mx_nsquare_launch_shape(int n_bits, int64_t batch, int limbs_per_lane, int wavefronts_per_group, int* k,
                                       int* l, int* w, int* blocks, int* wavefronts) {
  if (!k || !l || !w || !blocks || !wavefronts) return MX_ERR_ARG;
  N2Launch r;
  MX_TRY(resolve_n2(n_bits, batch, limbs_per_lane, wavefronts_per_group, 1, r));
  *k = r.p.geo.K; *l = r.p.geo.L; *w = r.p.geo.W; *blocks = r.p.geo.nblk; *wavefronts = r.ch.wpg;
  return MX_OK;
}

// Shape for launches that are IN FLIGHT TOGETHER as pieces of `total` elements (several streams, several keys): the plain
// form with the lowest estimate for one launch of the total — the pieces then resemble it — never a time-sliced one, which
// only a lone launch can be (4 x 2500 ciphertexts at key_length 2048: 214 k/s at 9 limbs per lane on two wavefronts, 179 k/s
// in the shape of the time-sliced choice for a lone 10 000).
extern "C" int mx_nsquare_pieces_shape(int n_bits, int64_t total, int limbs_per_lane, int wavefronts_per_group,
                                       int* limbs_per_lane_out, int* wavefronts_per_group_out) {
  if (!limbs_per_lane_out || !wavefronts_per_group_out || total <= 0) return MX_ERR_ARG;
  if (limbs_per_lane != 0 && geo_index(limbs_per_lane) < 0) return MX_ERR_ARG;
  if (wavefronts_per_group < 0 || wavefronts_per_group > 2) return MX_ERR_ARG;      // this entry alone: pieces never take the five-wavefront form
  N2Choice best;
  if (!n2_best_candidate(limbs_per_lane, wavefronts_per_group, best, [&](N2Choice& c) {
        const double t = n2_estimate(n_bits, total, c.lpl, c.wpg);                  // (no `resident` out-parameter: the plain launch)
        // pieces of the wide two-wavefront form overlap better than one launch of their sum (4 x 5000 ciphertexts: 279 k/s
        // against 257 k/s at 9 limbs per lane, where the estimates for one launch of 20 000 say 87 against 83 ms)
        return c.lpl == LIMBS_PER_LANE_WIDE && c.wpg == 2 ? t * 0.93 : t;
      }))
    return MX_ERR_SIZE;
  *limbs_per_lane_out = best.lpl; *wavefronts_per_group_out = best.wpg;
  return MX_OK;
}

extern "C" int mx_nsquare_launch_timesliced(int n_bits, int64_t batch, int limbs_per_lane, int wavefronts_per_group,
                                            int* resident_per_cu, int* units_per_group) {
  if (!resident_per_cu || !units_per_group) return MX_ERR_ARG;
  N2Launch r;
  const int rc = resolve_n2(n_bits, batch, limbs_per_lane, wavefronts_per_group, 1, r);
  // this entry alone: the five-wavefront form is never time-sliced, answered without looking whether the form exists
  if (wavefronts_per_group == 4 && rc != MX_ERR_ARG) { *resident_per_cu = 0; *units_per_group = 0; return MX_OK; }
  MX_TRY(rc);
  *resident_per_cu = r.ch.resident;
  *units_per_group = r.ch.resident ? r.ch.units : 0;
  return MX_OK;
}

extern "C" int mx_nsquare_latency_form(int n_bits, int* lanes, int* positions, int* pivot, int64_t* max_batch) {
  if (n_bits < 2) return MX_ERR_ARG;
  Geometry gb;
  if (!bipair_geometry(n_bits, gb)) return MX_ERR_SIZE;
  if (lanes) *lanes = gb.K;
  if (positions) *positions = gb.L * gb.nblk;
  if (pivot) *pivot = gb.h_lo;
  if (max_batch) *max_batch = (int64_t)device_cus() * (64 / gb.K);
  return MX_OK;
}

extern "C" int mx_nsquare_launch_instance(int n_bits, int64_t batch, int limbs_per_lane, int wavefronts_per_group,
                                          int* k, int* l, int* wavefronts, int* friendly, int* timesliced) {
  if (!k || !l || !wavefronts || !friendly || !timesliced) return MX_ERR_ARG;
  N2Launch r;
  MX_TRY(resolve_n2(n_bits, batch, limbs_per_lane, wavefronts_per_group, 1, r));
  *k = r.p.geo.K; *l = r.p.geo.L; *wavefronts = r.ch.wpg;
  *friendly = r.friendly ? 1 : 0;
  *timesliced = r.ch.resident > 0 ? 1 : 0;
  return MX_OK;
}

// A lone launch above a capacity step of the wide two-wavefront shape (one workgroup of 2 x 64/K elements per CU: 8192
// ciphertexts at key_length 2048) pays for a second workgroup per CU: 55-59 ms for 10 000-12 288 instead of 33 for 8192.
// A caller that owns a second stream has one more option: the first `cap` elements in that shape, the rest at 9 limbs
// per lane on two wavefronts AT THE SAME TIME — a 9-limb workgroup (168 registers per wavefront) fits beside the 18-limb
// one (256) on a CU but not beside another 9-limb one, so the dispatcher spreads the remainder one workgroup per CU.
// Measured (tools/sweep_split.py, profiles/r04_split_launch.txt): a CU that hosts both takes 48-49 ms whatever the
// share of such CUs — the two wavefronts of a SIMD add up almost fully (a lone wavefront already issues 83 % of what
// its SIMD can).  Rounds 3-4 took the split where the single launches were slower still (10 752 .. 12 288 ciphertexts at
// key_length 2048: 48.5 instead of 51-56 ms).  Since round 5 the time-sliced 18-limb launch covers that range in 44-48 ms
// (n2_estimate above): the library no longer proposes a split by itself; the developer knob still forces one (tests,
// tools/sweep_split.py).
extern "C" int mx_nsquare_launch_split(int n_bits, int64_t batch, int64_t* first_rows, int* first_lpl, int* first_wpg,
                                       int* rest_lpl, int* rest_wpg) {
  if (!first_rows || !first_lpl || !first_wpg || !rest_lpl || !rest_wpg || batch <= 0) return MX_ERR_ARG;
  *first_rows = 0; *first_lpl = *first_wpg = *rest_lpl = *rest_wpg = 0;
  if (g_knob_n2_split == 1) return MX_OK;
  N2Shape wide, narrow;
  if (!shape_n2(n_bits, 1, batch, LIMBS_PER_LANE_WIDE, 2, wide) || !shape_n2(n_bits, 1, batch, LIMBS_PER_LANE, 2, narrow)) return MX_OK;
  const int cus = device_cus();
  const int64_t per_wg_wide = (int64_t)mx::N2_SPLIT_PAIRS * (64 / wide.geo.K), per_wg_narrow = (int64_t)mx::N2_SPLIT_PAIRS * (64 / narrow.geo.K);
  const int64_t cap = (int64_t)cus * per_wg_wide;
  if (batch <= cap || batch >= 2 * cap) return MX_OK;
  const int64_t rest = batch - cap;
  const int64_t rest_wgs = (rest + per_wg_narrow - 1) / per_wg_narrow;
  if (g_knob_n2_split != 2) return MX_OK;
  if (rest_wgs > cus) return MX_OK;
  *first_rows = cap; *first_lpl = LIMBS_PER_LANE_WIDE; *first_wpg = 2; *rest_lpl = LIMBS_PER_LANE; *rest_wpg = 2;
  return MX_OK;
}

extern "C" int mx_nsquare_geometry_for(int n_bits, int64_t batch, int limbs_per_lane, int* k, int* l, int* w,
                                       int* blocks) {
  int waves = 0;
  return mx_nsquare_launch_shape(n_bits, batch, limbs_per_lane, 0, k, l, w, blocks, &waves);
}

extern "C" int mx_nsquare_geometry(int n_bits, int64_t batch, int* k, int* l, int* w, int* blocks) {
  return mx_nsquare_geometry_for(n_bits, batch, 0, k, l, w, blocks);
}

extern "C" int64_t mx_nsquare_plan_bytes(int limbs_n, int exp_limbs) {
  if (limbs_n <= 0 || exp_limbs <= 0) return MX_ERR_ARG;
  return lifted_tape_offset(limbs_n) + n2_tape_bytes();
}

extern "C" int mx_powmod_nsquare_prepare(mx_nsquare_plan* plan, const uint32_t* h_n, const uint32_t* h_exp,
                                         int limbs_n, int exp_limbs, void* d_plan, int64_t plan_bytes, void* stream) {
  return mx_powmod_nsquare_prepare_ex(plan, h_n, h_exp, limbs_n, exp_limbs, 0, d_plan, plan_bytes, stream);
}

// Width of the fixed-window schedule (MX_PLAN_FIXED_WINDOW): every window costs a multiplication, so narrower windows
// than the sliding schedule's pay; the table holds x^1 .. x^(2^w - 1) (digit 0 multiplies by the domain's one).
static int fixed_window_n2(int exp_bits) {
  int best = 1;
  long bestc = -1;
  for (int w = 1; w <= 7; ++w) {
    const long c = (exp_bits + w - 1) / w + (1L << w) - 2;
    if (bestc < 0 || c < bestc) { bestc = c; best = w; }
  }
  return best;
}

// The section of the five-wavefront latency form (mx_bipair.hpp) at bp: constants for R' = 2^(W hL), the fold rows
// (computed on the device from N by the bipartite form's setup kernel) and the quotients of the folds,
// floor(2^(W (Pd + k)) / N).  h_lo: the pivot they were built with, 0 where the modulus has no such form.
static int prepare_bipair_section(const u32* h_n, int limbs_n, int bits, char* bp, hipStream_t s, int& h_lo) {
  h_lo = 0;
  Geometry gb;
  if (!bipair_geometry(bits, gb)) return MX_OK;
  std::vector<u32> rows((size_t)n2_consts_words(limbs_n));
  n2_constants(rows.data(), h_n, limbs_n, gb.W * gb.h_lo, bits - 1);
  MX_TRY(upload_words(bp, rows.data(), rows.size(), s));
  const int pd = gb.L * gb.nblk, pw = gb.L * gb.K;
  std::vector<u32> quot((size_t)mx::BP_QROWS * pw, 0u);
  for (int r = 0; r < mx::BP_QROWS; ++r) {
    const int m = gb.W * (pd + r);                            // 2^m / N
    const int la = m / 32 + 1;
    std::vector<u32> num(la, 0u), q(la, 0u), rem(limbs_n, 0u);
    num[m / 32] = 1u << (m % 32);
    divmod_words(q.data(), rem.data(), num.data(), la, h_n, limbs_n);
    for (int i = 0; i < pw; ++i) {                            // W-bit limb i of the quotient
      const int bit = gb.W * i, w0 = bit >> 5, off = bit & 31;
      u64 v = w0 < la ? q[w0] : 0u;
      if (w0 + 1 < la) v |= (u64)q[w0 + 1] << 32;
      quot[(size_t)r * pw + i] = (u32)(v >> off) & ((1u << gb.W) - 1u);
    }
    if (bit_length(q.data(), la) > gb.W * pw) return MX_ERR_SIZE;
  }
  char* qp = bp + n2_consts_bytes(limbs_n) + bipair_fold_bytes();
  MX_TRY(upload_words(qp, quot.data(), quot.size(), s));
  mx::BiSetupArgs sa;
  sa.mods = (const u32*)bp;                                   // row 0 of the constants: N
  sa.consts = (u32*)(bp + n2_consts_bytes(limbs_n));
  sa.groups = 1; sa.limbs = limbs_n; sa.nblk = gb.nblk; sa.pd = pd; sa.h_lo = gb.h_lo;
  MX_TRY(mxl::launch_bisetup(gb.K, sa, s));
  h_lo = gb.h_lo;
  return MX_OK;
}

// ---- the tapes of a plan (mx_powmod_n2.hpp): host arithmetic only
namespace {
struct N2Tape {
  std::vector<u32> words;
  int n_sqr = 0, n_mul = 0, n_sqr0 = 0, n_mul0 = 0;
  int half_reads = 0, n_writes = 6;          // digits read from slots; the prologue writes 4 constant pairs and x_lo, x_hi
  int top_slot = mx::N2_SLOT_TABLE;          // the highest slot the tape touches
  int64_t cost = 0;                          // N2_COST_* units (mx_host.hpp)
  void emit(u32 op, int arg) {
    words.push_back((op << 28) | (u32)arg);
    switch (op) {
      case mx::N2_SQR: n_sqr += arg; cost += (int64_t)arg * N2_COST_SQR; return;
      case mx::N2_SQR0: n_sqr0 += arg; cost += (int64_t)arg * N2_COST_SQR0; return;
      case mx::N2_CLR1: return;
      case mx::N2_MUL: case mx::N2_MULC: n_mul += 1; half_reads += 2; cost += N2_COST_MUL; break;
      case mx::N2_MUL0: n_mul0 += 1; half_reads += 1; cost += N2_COST_MUL0; break;
      case mx::N2_STORE: n_writes += 1; break;
      default: half_reads += 2; break;       // N2_ADD, N2_LOAD
    }
    if (arg > top_slot) top_slot = arg;
  }
  int reads() const { return (half_reads + 1) / 2; }
  int rows() const { return top_slot - mx::N2_SLOT_TABLE + 1; }
  // x = (x_lo, 0) * K1 + (x_hi, 0) * K2, the first row of the table of every schedule
  void convert() {
    emit(mx::N2_LOAD, mx::N2_SLOT_LO); emit(mx::N2_MUL, mx::N2_SLOT_K1); emit(mx::N2_STORE, mx::N2_SLOT_TMP);
    emit(mx::N2_LOAD, mx::N2_SLOT_HI); emit(mx::N2_MUL, mx::N2_SLOT_K2); emit(mx::N2_ADD, mx::N2_SLOT_TMP);
    emit(mx::N2_STORE, mx::N2_SLOT_TABLE);
  }
  // the odd powers 3, 5, .. of the accumulator — which row `first` holds already — into the rows behind it
  void odd_powers(int first, int nodd) {
    if (nodd <= 1) return;
    emit(mx::N2_SQR, 1); emit(mx::N2_STORE, mx::N2_SLOT_SQ); emit(mx::N2_LOAD, first);
    for (int t = 1; t < nodd; ++t) { emit(mx::N2_MUL, mx::N2_SLOT_SQ); emit(mx::N2_STORE, first + t); }
  }
};
struct N2Tapes {
  N2Tape classic, lifted;      // lifted.words empty: none
  int ebits = 0, window = 1;
  bool prefer_lifted = false;
  int lift_pos1 = 0, lift_share1 = 0;
};

// Rows that the table region of a plan may have: what a fixed-window plan of a long exponent takes today (2^7), so that
// the lifted tape — two tables — never asks a caller for a larger workspace per element than the engine already hands out.
// Where both tables at their best widths would not fit, the planner narrows them (the window for N first in its search:
// width 5 instead of 7 costs ~1 % more instructions).
constexpr int N2_MAX_TABLE_ROWS = 128;

// The lifted tape (header of mx_nsquare_plan) for exp = e1 N + e0, e1 >= 1:
//   conversion and the odd powers of x | phase 1: sliding window over e1 with first-digit operations, multipliers the
//   first digits of that table | second digit := 0, the pair (Y0, 0) — a representative of x^e1 modulo N — and its odd
//   powers into a second table | phase 2: ONE chain of max(bits N, bits e0) - 1 pair squarings, a multiplication from the
//   y-table where a window of N ends and from the x-table where a window of e0 ends | times E.
// The three window widths are those that minimise the cost in N2_COST_* units, by exhaustive search over the exact
// recodings (8^3 candidates of a few thousand bits: microseconds).
void build_lifted(const u32* h_n, int limbs_n, const u32* h_exp, int exp_limbs, N2Tapes& tp) {
  std::vector<u32> e1(exp_limbs, 0u), e0(limbs_n, 0u);
  divmod_words(e1.data(), e0.data(), h_exp, exp_limbs, h_n, limbs_n);
  const bool has0 = bit_length(e0.data(), limbs_n) > 0;
  if (bit_length(e1.data(), exp_limbs) < (has0 ? 1 : 2)) return;      // exp <= N: nothing to lift
  constexpr int WMAX = 8;
  std::vector<SlidingWin> r1[WMAX + 1], rn[WMAX + 1], r0[WMAX + 1];
  for (int w = 1; w <= WMAX; ++w) {
    r1[w] = sliding_windows(e1.data(), exp_limbs, w);
    rn[w] = sliding_windows(h_n, limbs_n, w);
    if (has0) r0[w] = sliding_windows(e0.data(), limbs_n, w);
  }
  auto table_cost = [](int nodd) { return nodd > 1 ? (int64_t)N2_COST_SQR + (int64_t)(nodd - 1) * N2_COST_MUL : (int64_t)0; };
  int b1 = 0, bn = 0, b0 = 0;
  int64_t best = -1;
  for (int w1 = 1; w1 <= WMAX; ++w1)
    for (int w0 = 1; w0 <= (has0 ? WMAX : 1); ++w0)
      for (int wn = 1; wn <= WMAX; ++wn) {
        const int rows_x = 1 << (std::max(w1, has0 ? w0 : 1) - 1), rows_y = 1 << (wn - 1);
        if (rows_x + rows_y > N2_MAX_TABLE_ROWS) continue;
        const int chain = std::max(rn[wn][0].low, has0 ? r0[w0][0].low : 0);
        const int64_t c = table_cost(rows_x) + table_cost(rows_y) + (int64_t)r1[w1][0].low * N2_COST_SQR0 +
                          (int64_t)(r1[w1].size() - 1) * N2_COST_MUL0 + (int64_t)chain * N2_COST_SQR +
                          (int64_t)(rn[wn].size() + (has0 ? r0[w0].size() : 0) - 1) * N2_COST_MUL;
        if (best < 0 || c < best) { best = c; b1 = w1; b0 = w0; bn = wn; }
      }
  N2Tape& t = tp.lifted;
  const int rows_x = 1 << (std::max(b1, has0 ? b0 : 1) - 1), rows_y = 1 << (bn - 1);
  const int xtab = mx::N2_SLOT_TABLE, ytab = mx::N2_SLOT_TABLE + rows_x;
  t.convert();
  t.odd_powers(xtab, rows_x);
  // phase 1 (N2_LOAD brings the row's second digit along: nothing reads it, N2_CLR1 drops it)
  const std::vector<SlidingWin>& s1 = r1[b1];
  t.emit(mx::N2_LOAD, xtab + (int)s1[0].index1 - 1);
  for (size_t i = 1; i < s1.size(); ++i) {
    t.emit(mx::N2_SQR0, s1[i - 1].low - s1[i].low);
    t.emit(mx::N2_MUL0, xtab + (int)s1[i].index1 - 1);
  }
  if (s1.back().low) t.emit(mx::N2_SQR0, s1.back().low);
  t.emit(mx::N2_CLR1, 0);
  t.emit(mx::N2_STORE, ytab);
  t.odd_powers(ytab, rows_y);
  tp.lift_pos1 = t.n_sqr + t.n_sqr0;
  const int64_t cost1 = t.cost;
  // phase 2: the windows of N and of e0 merged by the position of their lowest bit (N first where they coincide)
  const std::vector<SlidingWin>& sn = rn[bn];
  const std::vector<SlidingWin> none;
  const std::vector<SlidingWin>& s0 = has0 ? r0[b0] : none;
  size_t in = 0, i0 = 0;
  int pos = -1;
  while (in < sn.size() || i0 < s0.size()) {
    const bool take_n = i0 >= s0.size() || (in < sn.size() && sn[in].low >= s0[i0].low);
    const SlidingWin& win = take_n ? sn[in] : s0[i0];
    const int slot = (take_n ? ytab : xtab) + (int)win.index1 - 1;
    if (pos < 0) {
      t.emit(mx::N2_LOAD, slot);
    } else {
      if (pos > win.low) t.emit(mx::N2_SQR, pos - win.low);
      t.emit(mx::N2_MUL, slot);
    }
    pos = win.low;
    (take_n ? in : i0) += 1;
  }
  if (pos > 0) t.emit(mx::N2_SQR, pos);
  t.emit(mx::N2_MULC, mx::N2_SLOT_E);
  tp.lift_share1 = (int)(cost1 * 65536 / t.cost);
  if ((int)t.words.size() > MAX_SLIDING_OPS) { tp.lifted = N2Tape(); return; }
  // the lifted tape has to pay: 2 % by the model, or the plan stays classic by default
  tp.prefer_lifted = t.cost * 100 < tp.classic.cost * 98;
}

int plan_tapes(const u32* h_n, const u32* h_exp, int limbs_n, int exp_limbs, int flags, N2Tapes& tp) {
  const int ebits = bit_length(h_exp, exp_limbs);
  tp.ebits = ebits;
  // ---- the classic tape: conversion, table of odd powers, sliding window, times E
  N2Tape& c = tp.classic;
  int w = 1;
  if (ebits > 0) c.convert();
  if (ebits == 0) {
    c.emit(mx::N2_LOAD, mx::N2_SLOT_ONE);
  } else if (flags & MX_PLAN_FIXED_WINDOW) {
    // Fixed windows of fw bits from the least significant end: the SEQUENCE of operations — fw squarings and one
    // multiplication per window, whatever the digits — depends on the exponent's bit length only, not on its bits
    // (the sliding schedule's run lengths and multiplication count do).  Which table row a window reads still does.
    const int fw = fixed_window_n2(ebits);
    auto digit = [&](int d) {
      u32 v = 0;
      for (int b = fw - 1; b >= 0; --b) {
        const int i = d * fw + b;
        v = (v << 1) | ((i < 32 * exp_limbs) ? ((h_exp[i >> 5] >> (i & 31)) & 1u) : 0u);
      }
      return (int)v;
    };
    auto slot_of = [&](int dg) { return dg ? mx::N2_SLOT_TABLE + dg - 1 : mx::N2_SLOT_ONE; };
    for (int t = 2; t < (1 << fw); ++t) { c.emit(mx::N2_MUL, mx::N2_SLOT_TABLE); c.emit(mx::N2_STORE, mx::N2_SLOT_TABLE + t - 1); }
    const int nwin = (ebits + fw - 1) / fw;
    c.emit(mx::N2_LOAD, slot_of(digit(nwin - 1)));
    for (int d = nwin - 2; d >= 0; --d) { c.emit(mx::N2_SQR, fw); c.emit(mx::N2_MUL, slot_of(digit(d))); }
    w = fw + 1;                              // the table region: 2^(w - 1) = 2^fw pair slots (one more than used)
  } else {
    w = sliding_window(ebits);
    std::vector<SlidingOp> ops = sliding_schedule(h_exp, exp_limbs, w);
    c.odd_powers(mx::N2_SLOT_TABLE, 1 << (w - 1));
    c.emit(mx::N2_LOAD, mx::N2_SLOT_TABLE + (int)ops[0].index1 - 1);
    for (size_t t = 1; t < ops.size(); ++t) {
      if (ops[t].squarings) c.emit(mx::N2_SQR, ops[t].squarings);     // 28-bit repeat count on the tape
      if (ops[t].index1) c.emit(mx::N2_MUL, mx::N2_SLOT_TABLE + (int)ops[t].index1 - 1);
    }
  }
  c.emit(mx::N2_MULC, mx::N2_SLOT_E);          // the last product: digits below 2N for the epilogue (mx_powmod_n2.hpp)
  if ((int)c.words.size() > MAX_SLIDING_OPS) return MX_ERR_SIZE;
  tp.window = w;
  // ---- the lifted tape: sliding-window plans whose exponent reaches N (a fixed-window plan's sequence of operations
  // must depend on the exponent's length only: it stays classic)
  if (!(flags & MX_PLAN_FIXED_WINDOW) && ebits >= bit_length(h_n, limbs_n)) build_lifted(h_n, limbs_n, h_exp, exp_limbs, tp);
  return MX_OK;
}

// the counting fields of a plan descriptor
void fill_plan_counts(mx_nsquare_plan* plan, const N2Tapes& tp) {
  const bool have = !tp.lifted.words.empty();
  const N2Tape& d = have && tp.prefer_lifted ? tp.lifted : tp.classic;       // what a one-wavefront launch runs by default
  plan->exp_bits = tp.ebits;
  plan->window = tp.window;
  plan->ntape = (int)tp.classic.words.size();
  plan->n_sqr = d.n_sqr;
  plan->n_mul = d.n_mul;
  plan->n_slot_reads = d.reads();
  plan->n_slot_writes = d.n_writes;
  plan->n_sqr_first = d.n_sqr0;
  plan->n_mul_first = d.n_mul0;
  plan->table_rows = std::max(1 << (tp.window - 1), have ? tp.lifted.rows() : 0);
  plan->lift = have ? (tp.prefer_lifted ? 3 : 1) : 0;
  plan->ntape_lift = (int)tp.lifted.words.size();
  plan->n_sqr_classic = tp.classic.n_sqr;
  plan->n_mul_classic = tp.classic.n_mul;
  plan->lift_positions = tp.lifted.n_sqr + tp.lifted.n_sqr0;
  plan->lift_pos1 = tp.lift_pos1;
  plan->lift_share1 = tp.lift_share1;
}
}  // namespace

extern "C" int mx_nsquare_tape(const uint32_t* h_n, const uint32_t* h_exp, int limbs_n, int exp_limbs, int flags, int lifted,
                               uint32_t* h_tape, int max_words, mx_nsquare_plan* plan) {
  if (!h_n || !h_exp || !h_tape || !plan || max_words < 0 || (lifted != 0 && lifted != 1)) return MX_ERR_ARG;
  if (flags & ~MX_PLAN_FIXED_WINDOW) return MX_ERR_ARG;
  if (limbs_n <= 0 || exp_limbs <= 0) return MX_ERR_ARG;
  if (!(h_n[0] & 1u)) return MX_ERR_MODULUS;
  const int bits = bit_length(h_n, limbs_n);
  if (bits < 2) return MX_ERR_MODULUS;
  N2Tapes tp;
  MX_TRY(plan_tapes(h_n, h_exp, limbs_n, exp_limbs, flags, tp));
  std::memset(plan, 0, sizeof(*plan));
  plan->limbs_n = limbs_n;
  plan->n_bits = bits;
  fill_plan_counts(plan, tp);
  const std::vector<u32>& words = lifted ? tp.lifted.words : tp.classic.words;
  if ((int)words.size() > max_words) return MX_ERR_WORKSPACE;
  std::memcpy(h_tape, words.data(), words.size() * 4);
  return (int)words.size();
}

extern "C" int mx_powmod_nsquare_prepare_ex(mx_nsquare_plan* plan, const uint32_t* h_n, const uint32_t* h_exp,
                                            int limbs_n, int exp_limbs, int flags, void* d_plan, int64_t plan_bytes,
                                            void* stream) {
  if (!plan || !h_n || !h_exp || !d_plan) return MX_ERR_ARG;
  if (flags & ~MX_PLAN_FIXED_WINDOW) return MX_ERR_ARG;
  if (limbs_n <= 0 || exp_limbs <= 0) return MX_ERR_ARG;
  if (!(h_n[0] & 1u)) return MX_ERR_MODULUS;
  const int bits = bit_length(h_n, limbs_n);
  if (bits < 2) return MX_ERR_MODULUS;
  // constants of every geometry that has an instance for this modulus (they differ in R = 2^(W*L*blocks))
  const int* lpls = N2_LPLS;
  Geometry geos[N2_GEOS];
  int geometries = 0;
  for (int g = 0; g < N2_GEOS; ++g)
    if (choose_geometry(bits, geos[g], lpls[g]) && geos[g].K <= max_lanes(lpls[g], 2)) geometries |= 1 << g;
  if (!(geometries & 1)) return MX_ERR_SIZE;
  if (mx_nsquare_plan_bytes(limbs_n, exp_limbs) > plan_bytes) return MX_ERR_WORKSPACE;
  const int k = bits - 1;                                      // x = x_lo + 2^k x_hi
  N2Tapes tp;
  MX_TRY(plan_tapes(h_n, h_exp, limbs_n, exp_limbs, flags, tp));
  const int64_t cb = n2_consts_bytes(limbs_n);
  hipStream_t s = (hipStream_t)stream;
  char* dp = (char*)d_plan;
  int done_m[N2_GEOS] = {};
  std::vector<u32> rows[N2_GEOS];
  for (int g = 0; g < N2_GEOS; ++g) {
    if (!(geometries & (1 << g))) continue;
    const int m = geos[g].W * geos[g].L * geos[g].nblk;
    done_m[g] = m;
    int same = -1;
    for (int h = 0; h < g; ++h) if (done_m[h] == m) same = h;       // geometries often share R (2048: all three)
    if (same >= 0) {
      rows[g] = rows[same];
    } else {
      rows[g].resize((size_t)n2_consts_words(limbs_n));
      n2_constants(rows[g].data(), h_n, limbs_n, m, k);
    }
    MX_TRY(upload_words(dp + g * cb, rows[g].data(), rows[g].size(), s));
  }
  MX_TRY(upload_words(dp + N2_GEOS * cb, tp.classic.words.data(), tp.classic.words.size(), s));
  if (!tp.lifted.words.empty()) MX_TRY(upload_words(dp + lifted_tape_offset(limbs_n), tp.lifted.words.data(), tp.lifted.words.size(), s));
  int pivot = 0;
  MX_TRY(prepare_bipair_section(h_n, limbs_n, bits, dp + bipair_section_offset(limbs_n), s, pivot));
  if (pivot) geometries |= N2_GEO_BIPAIR | (pivot << N2_GEO_PIVOT_SHIFT);      // the plan carries the pivot its constants were built with
  plan->d_plan = d_plan;
  plan->plan_bytes = plan_bytes;
  plan->limbs_n = limbs_n;
  plan->n_bits = bits;
  plan->geometries = geometries;
  fill_plan_counts(plan, tp);
  return MX_OK;
}

extern "C" int64_t mx_powmod_nsquare_run_workspace_bytes(const mx_nsquare_plan* plan, int64_t batch) {
  if (!plan || batch <= 0 || plan->window < 1) return MX_ERR_ARG;
  // the largest table any launch shape of this batch needs (the caller may leave the choice to the library)
  // (the lifted tape, one-wavefront launches only, has two tables: sized whatever MX_KNOB_N2_LIFT says now, so that a
  // workspace sized under one value of the knob serves a run under another)
  int64_t most = -1;
  for (int l : N2_LPLS) {
    N2Shape p;
    if (shape_n2(plan->n_bits, 1 << (plan->window - 1), batch, l, 2, p) && p.table_bytes + p.sched_bytes > most) most = p.table_bytes + p.sched_bytes;
    if ((plan->lift & 1) && shape_n2(plan->n_bits, plan->table_rows, batch, l, 1, p) && p.table_bytes > most) most = p.table_bytes;
  }
  return most < 0 ? MX_ERR_SIZE : most;
}

namespace {
// The pivot of the five-wavefront form of a plan: the one prepare built the plan's constants with (bits 8-15 of
// `geometries`), checked against the geometry — a multiple of L, L <= h_lo < Pd, E = 2^(W (Pd - h_lo)) a digit below N.
// A plan of an older library has no pivot recorded: the knob's, as that library did (gb.h_lo on entry).
int plan_pivot(const mx_nsquare_plan* plan, Geometry& gb) {
  const int h = (plan->geometries >> N2_GEO_PIVOT_SHIFT) & 0xFF, pd = gb.L * gb.nblk;
  if (h == 0) return MX_OK;
  if (h % gb.L != 0 || h < gb.L || h >= pd || gb.W * (pd - h) >= plan->n_bits - 1) return MX_ERR_ARG;
  gb.h_lo = h;
  return MX_OK;
}

// What every launch of a run starts from: the whole tape on the constants of geometry gi, one plain segment.
mx::PowmodN2Args n2_run_args(const mx_nsquare_plan* plan, const uint32_t* d_bases, uint32_t* d_out, int limbs2, int64_t batch,
                             void* d_ws, const N2Launch& r) {
  const int64_t cb = n2_consts_bytes(plan->limbs_n);
  const char* dp = (const char*)plan->d_plan;
  mx::PowmodN2Args a;
  a.bases = d_bases; a.out = d_out;
  a.consts = (const u32*)(dp + geo_index(r.ch.lpl) * cb);
  a.tape = (const u32*)(dp + N2_GEOS * cb);
  a.ntape = plan->ntape;
  a.slots = (u32*)d_ws;
  a.batch = batch; a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.nblk = r.p.geo.nblk; a.ksplit = plan->n_bits - 1;
  a.friendly = r.friendly;
  a.sched = nullptr; a.sched_groups = a.sched_segments = a.sched_n_sqr = 0;
  a.first = a.last = 1; a.pos_begin = 0; a.pos_end = 0x7FFFFFFF;
  return a;
}
// The last product and the epilogue as a segment of their own.  (The last product is the last word of the tape: the
// segment is handed that word alone, at position 1 — walking the whole tape to it, a dependent scalar load per word, was
// 100 of the five-wavefront launch's 136 us.)
void last_word_segment(mx::PowmodN2Args& a) {
  a.tape += a.ntape - 1; a.ntape = 1;
  a.first = 0; a.last = 1; a.pos_begin = 1; a.pos_end = 0x7FFFFFFF;
}
}  // namespace

extern "C" int mx_powmod_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_bases, uint32_t* d_out,
                                     int limbs2, int64_t batch, int limbs_per_lane, int wavefronts_per_group,
                                     int segments, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!plan || !plan->d_plan || !d_bases || !d_out || !d_ws) return MX_ERR_ARG;
  if (limbs2 <= 0 || plan->limbs_n <= 0 || plan->ntape <= 0) return MX_ERR_ARG;
  if (segments < 0 || segments > 64) return MX_ERR_ARG;
  const int bits = plan->n_bits;
  if (2 * bits - 1 > 32 * limbs2) return MX_ERR_ARG;          // rows too narrow for N^2
  // this entry alone: MX_ERR_ARG where the shape queries say MX_ERR_SIZE
  if (wavefronts_per_group == 4 && limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE_LAT) return MX_ERR_ARG;
  N2Launch r;
  const int classic_rows = 1 << (plan->window - 1);
  MX_TRY(resolve_n2(bits, batch, limbs_per_lane, wavefronts_per_group, classic_rows, r));
  if (r.ch.wpg == 4 && wavefronts_per_group != 4 && !(plan->geometries & N2_GEO_BIPAIR)) r.ch.wpg = 2;      // a plan of an older layout
  // The lifted tape (header of mx_nsquare_plan): one-wavefront launches of a plan that holds one, as MX_KNOB_N2_LIFT says,
  // where the workspace has room for its two tables (a caller that sized it by mx_powmod_nsquare_run_workspace_bytes
  // does); every other form reads the classic tape and its squaring count.
  const int classic_n_sqr = (plan->lift & 1) ? plan->n_sqr_classic : plan->n_sqr;
  bool lifted = r.ch.wpg == 1 && (plan->lift & 1) && plan->ntape_lift > 0 && g_knob_n2_lift != 1 && ((plan->lift & 2) || g_knob_n2_lift == 2);
  if (lifted) {
    N2Shape pl;
    if (shape_n2(bits, plan->table_rows, batch, r.ch.lpl, 1, pl) && pl.table_bytes <= ws_bytes) r.p = pl; else lifted = false;
  }
  // squarings, of either kind, of the tape this run executes: the positions of its segments
  const int run_n_sqr = !lifted ? classic_n_sqr : plan->lift_positions;
  const N2Choice& ch = r.ch;
  const N2Shape& p = r.p;
  const bool five = ch.wpg == 4;
  if (!(plan->geometries & (five ? N2_GEO_BIPAIR : 1 << geo_index(ch.lpl)))) return MX_ERR_SIZE;
  if (p.table_bytes + (ch.resident ? p.sched_bytes : 0) > ws_bytes) return MX_ERR_WORKSPACE;
  if (2 * p.geo.K * p.geo.L + 8 < limbs2 + 2) return MX_ERR_ARG;   // row wider than the staging area
  mx::PowmodN2Args a = n2_run_args(plan, d_bases, d_out, limbs2, batch, d_ws, r);
  if (lifted) {
    a.tape = (const u32*)((const char*)plan->d_plan + lifted_tape_offset(plan->limbs_n));
    a.ntape = plan->ntape_lift;
  }
  hipStream_t s = (hipStream_t)stream;
  if (five) {
    // the five-wavefront latency form: its own kernel for everything in front of the last product, then the last product and
    // the epilogue as a last segment of the two-wavefront 3-limb kernel, whose slots it shares
    Geometry gb = r.bi;
    MX_TRY(plan_pivot(plan, gb));
    const int64_t cb = n2_consts_bytes(plan->limbs_n);
    const char* bp = (const char*)plan->d_plan + bipair_section_offset(plan->limbs_n);
    const int pd = gb.L * gb.nblk;
    mx::PowmodBiPairArgs b;
    b.bases = d_bases;
    b.consts = (const u32*)bp;
    b.fold = (const u32*)(bp + cb);
    b.quot = (const u32*)(bp + cb + bipair_fold_bytes());
    b.tape = a.tape;
    b.slots = (u32*)d_ws;
    b.batch = batch; b.nlanes = p.nlanes;
    b.limbsn = plan->limbs_n; b.limbs2 = limbs2; b.ntape = plan->ntape;
    b.nblk = gb.nblk; b.pd = pd; b.h_lo = gb.h_lo; b.ksplit = bits - 1;
    b.nc = (gb.W * (pd + 6) - bits + 1) / gb.W + 1;           // c = floor(2^(W (Pd + 6)) / N) <= 2^(W (Pd + 6) - bits + 1)
    if (b.nc > 11) return MX_ERR_SIZE;
    b.pos_end = 0x7FFFFFFF;
    b.e_pos = pd - gb.h_lo;
    MxKernelTimer timer(s);
    MX_TRY(mxb::launch_n2_bipair(gb.K, b, p.nblocks * mx::N2_SPLIT_PAIRS, s));
    last_word_segment(a);
    return launch_n2(a, p, 2, s);
  }
  // segments: consecutive launches that each execute a stretch of the tape (mx_powmod_n2.hpp); positions
  // are counted in squarings, the accumulator travels through a scratch slot of the workspace
  int nseg = segments > 0 ? segments : n2_auto_segments(run_n_sqr, p.nlanes / 64 * ch.wpg);
  if (nseg > run_n_sqr / 16) nseg = run_n_sqr / 16;
  if (nseg < 1) nseg = 1;
  MxKernelTimer timer(s);                        // one timed interval per exponentiation (all its segments)
  if (ch.resident > 0) {
    // time-sliced: one launch of resident workgroups, the segments are units of its own scheduler
    nseg = segments > 0 ? segments : ch.units;
    if (nseg > N2_TIMESLICE_MAX_SEGMENTS) nseg = N2_TIMESLICE_MAX_SEGMENTS;
    if (nseg > classic_n_sqr / 16) nseg = classic_n_sqr / 16;
    if (nseg < 1) nseg = 1;
    a.sched = (u32*)((char*)d_ws + p.table_bytes);
    a.sched_groups = (int)p.groups; a.sched_segments = nseg; a.sched_n_sqr = classic_n_sqr;
    MX_HIP(hipMemsetAsync(a.sched, 0, (size_t)(mx::N2_TS_HEADER + p.groups * (nseg - 1)) * 4, s));
    // no more workgroups than there are groups for their pairs
    int64_t wgs = (int64_t)ch.resident * device_cus();
    if (wgs > p.nblocks) wgs = p.nblocks;
    return launch_n2(a, p, ch.wpg, s, wgs);
  }
  // The friendly-modulus instances of the one-wavefront wide kernel (mx_capi_n2w.hip: groups of 4 and 8 lanes) run the
  // tape up to, not including, its last product (N2_MULC, tape position n_sqr + 1); that product and the epilogue run as
  // one more segment on the plain instance (mx_powmod_n2.hpp).
  const bool fr_tape = ch.wpg == 1 && a.friendly;
  // Where segment sg begins.  Classic tape: by squaring count — its multiplications are spread evenly.  Lifted tape: by
  // estimated cost — a first-digit squaring costs ~0.45 of a pair squaring, so equal counts would make the segments of
  // phase 1 less than half as long as the others and a burst of launches would drain unevenly.  The
  // planner walked the tape with its cost constants and left the summary: lift_pos1 positions in front of phase 2 carry
  // lift_share1 / 65536 of the cost; within either stretch cost is linear in position to within a window.
  auto segment_begin = [&](int sg) -> int {
    if (!lifted) return (int)((int64_t)run_n_sqr * sg / nseg);
    const double f = (double)sg / nseg, f1 = plan->lift_share1 / 65536.0;
    const int p1 = plan->lift_pos1, p2 = run_n_sqr - p1;
    if (f1 <= 0.0 || f1 >= 1.0) return (int)((int64_t)run_n_sqr * sg / nseg);
    return f <= f1 ? (int)(p1 * f / f1) : p1 + (int)(p2 * (f - f1) / (1.0 - f1));
  };
  for (int sg = 0; sg < nseg; ++sg) {
    const bool final_sg = sg == nseg - 1;
    a.first = sg == 0;
    a.last = final_sg && !fr_tape;
    a.pos_begin = segment_begin(sg);
    a.pos_end = final_sg ? (fr_tape ? run_n_sqr + 1 : 0x7FFFFFFF) : segment_begin(sg + 1);
    MX_TRY(launch_n2(a, p, ch.wpg, s));
  }
  if (fr_tape) {
    a.friendly = 0;
    last_word_segment(a);
    MX_TRY(launch_n2(a, p, ch.wpg, s));
  }
  return MX_OK;
}

// ---- one-shot form: prepare into the head of the workspace, run with the rest
extern "C" int64_t mx_powmod_nsquare_workspace_bytes(int limbs_n, int exp_limbs, int64_t batch) {
  if (limbs_n <= 0 || exp_limbs <= 0 || batch <= 0) return MX_ERR_ARG;
  mx_nsquare_plan sizing{};
  sizing.n_bits = sizing_bits(limbs_n);
  sizing.window = sliding_window(32 * exp_limbs);
  sizing.lift = 1;                                 // room for the two tables of a lifted tape, whatever the exponent turns out to be
  sizing.table_rows = N2_MAX_TABLE_ROWS;
  int64_t run = mx_powmod_nsquare_run_workspace_bytes(&sizing, batch);
  if (run < 0) return run;
  return mx_nsquare_plan_bytes(limbs_n, exp_limbs) + run;
}

extern "C" int mx_powmod_nsquare(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* h_n, const uint32_t* h_exp,
                                 int limbs_n, int limbs2, int exp_limbs, int64_t batch, void* d_ws, int64_t ws_bytes,
                                 void* stream) {
  if (!d_bases || !d_out || !h_n || !h_exp || !d_ws) return MX_ERR_ARG;
  if (limbs_n <= 0 || limbs2 <= 0 || exp_limbs <= 0 || batch <= 0) return MX_ERR_ARG;
  const int64_t pb = mx_nsquare_plan_bytes(limbs_n, exp_limbs);
  if (pb > ws_bytes) {
    if (!(h_n[0] & 1u) || bit_length(h_n, limbs_n) < 2) return MX_ERR_MODULUS;
    return MX_ERR_WORKSPACE;
  }
  mx_nsquare_plan plan;
  MX_TRY(mx_powmod_nsquare_prepare(&plan, h_n, h_exp, limbs_n, exp_limbs, d_ws, pb, stream));
  return mx_powmod_nsquare_run(&plan, d_bases, d_out, limbs2, batch, 0, 0, 0,
                               (char*)d_ws + pb, ws_bytes - pb, stream);
}

// ---- multi-exponentiation modulo N^2 (mx_multiexp_n2.hpp): homomorphic linear maps of ciphertexts -----------------
namespace mxm { int launch_multiexp(int K, bool table, const mx::MultiexpN2Args& a, int64_t nblocks, hipStream_t s); }
namespace mxmm { int launch_shared(int K, const mx::SharedN2Args& a, int64_t nblocks, hipStream_t s); }
namespace {
constexpr int MX_MULTIEXP_MAX_WINDOW = 8;
// limits of the narrow-geometry entries
constexpr int64_t MX_GRID_WAVEFRONTS = (int64_t)1 << 31;       // one grid holds fewer wavefronts than this; columns, rows and shared tables of a map: at most this many
constexpr int64_t MX_MAX_ROWS = ((int64_t)1 << 31) - 1;        // row counts of the histogram and scan entries stay below (one more group: the one row)
constexpr int64_t MX_MAX_POSITIONS = (int64_t)1 << 30;         // samples of a tile, positions of a convolution (they travel as int)
constexpr int64_t MX_MAX_LOCAL_TABLES = (int64_t)1 << 36;      // tables of a convolution's own grids
constexpr int MX_MULTIEXP_MODEL_MAX_WINDOW = 6;         // the cost model's range (the caller may ask for up to 8)
// the narrow geometry of the pair kernel: groups of 1 .. 32 lanes
bool multiexp_geometry(int n_bits, int limbs_per_lane, Geometry& g) {
  if (limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE) return false;
  return choose_geometry(n_bits, g, LIMBS_PER_LANE) && g.K <= 32;
}
// Window of the interleaved fixed-window schedule, from pair products: 2^w - 2 per input to build its table (plus the two
// of its conversion, the same for every w), ceil(bits / w) multiplications per term and output, (ceil(bits / w) - 1) w
// squarings per output.
int multiexp_window(int64_t n_inputs, int64_t n_outputs, int64_t terms, int weight_bits) {
  if (weight_bits <= 1) return 1;
  int best = 1;
  double bestc = -1.0;
  for (int w = 1; w <= MX_MULTIEXP_MODEL_MAX_WINDOW; ++w) {
    const double nwin = (double)((weight_bits + w - 1) / w);
    const double c = (double)n_inputs * (double)((1 << w) - 2) + (double)n_outputs * ((double)terms * nwin + (nwin - 1.0) * w);
    if (bestc < 0 || c < bestc) { bestc = c; best = w; }
  }
  return best;
}

// What every launch of a homomorphic kernel starts from, after the entry point's own argument checks: the narrow
// geometry of the plan's modulus, the plan's constant rows of that geometry and the groups per wavefront.  Refuses, in
// this order, rows too narrow for N^2 (MX_ERR_ARG), a plan or modulus without the narrow geometry — or a
// limbs_per_lane that is not the narrow one, where the entry point has not refused it as an argument before —
// (MX_ERR_SIZE), and rows wider than the staging area (MX_ERR_ARG).
struct NarrowLaunch {
  Geometry g;
  const u32* consts;
  int gpw;
  int64_t blocks(int64_t groups) const { return (groups + gpw - 1) / gpw; }
};
int narrow_launch(const mx_nsquare_plan* plan, int limbs2, int limbs_per_lane, NarrowLaunch& o) {
  const int bits = plan->n_bits;
  if (32 * (int64_t)limbs2 < 2 * (int64_t)bits) return MX_ERR_ARG;
  if (!(plan->geometries & 1) || !multiexp_geometry(bits, limbs_per_lane, o.g)) return MX_ERR_SIZE;
  if (2 * o.g.K * o.g.L + 8 < limbs2 + 2) return MX_ERR_ARG;
  o.consts = (const u32*)((const char*)plan->d_plan + geo_index(LIMBS_PER_LANE) * n2_consts_bytes(plan->limbs_n));
  o.gpw = 64 / o.g.K;
  return MX_OK;
}

// split-K: outputs too few to give every SIMD of the device a wavefront have their terms cut into chunks that run on
// groups of their own (a second launch multiplies the partial products together)
int64_t splitk_chunk(const Geometry& g, int64_t n_outputs, int64_t terms) {
  const int64_t target = (int64_t)device_cus() * 4 * (64 / g.K);
  int64_t chunk = terms;
  if (n_outputs > 0 && n_outputs < target && terms > 64) {
    chunk = (terms * n_outputs + target - 1) / target;
    if (chunk < 64) chunk = 64;
  }
  return chunk < 1 ? 1 : chunk;
}

// the table pass (multiexp_n2_table_kernel): one group per input row, tables into the workspace
int launch_table_pass(const NarrowLaunch& o, const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_inputs,
                      int limbs2, int window, void* d_ws, hipStream_t s) {
  mx::MultiexpN2Args t{};
  t.inputs = d_inputs;
  t.tables = (u32*)d_ws;
  t.consts = o.consts;
  t.n_inputs = n_inputs;
  t.window = window;
  t.limbsn = plan->limbs_n; t.limbs2 = limbs2; t.nblk = o.g.nblk; t.ksplit = plan->n_bits - 1;
  return mxm::launch_multiexp(o.g.K, true, t, o.blocks(n_inputs), s);
}

// words of a weight and windows of the schedule (none where there are no terms)
void weight_fields(int terms, int weight_bits, int window, int& wwords, int& nwin) {
  wwords = (weight_bits + 31) / 32;
  nwin = terms > 0 ? (weight_bits + window - 1) / window : 0;
}

// a sizing query's answer (negative: its refusal) against what the caller brought
inline int workspace_fits(int64_t need, int64_t have) {
  if (need < 0) return (int)need;
  return need > have ? MX_ERR_WORKSPACE : MX_OK;
}

// What the weighted maps (multiexp, matmul, conv) all refuse as arguments, after the counts of their own; then the
// refusals of narrow_launch.
int weighted_launch(const mx_nsquare_plan* plan, const void* d_out, const void* d_ws, int64_t n_rows, int limbs2,
                    const int32_t* d_index, const uint32_t* d_weights, int terms, int weight_bits, int limbs_per_lane,
                    int window, NarrowLaunch& o) {
  if (!plan || !plan->d_plan || !d_out || !d_ws || plan->limbs_n <= 0) return MX_ERR_ARG;
  if (n_rows <= 0 || limbs2 <= 0 || terms < 0 || weight_bits < 0) return MX_ERR_ARG;
  if (terms > 0 && (!d_index || !d_weights)) return MX_ERR_ARG;
  if (window < 1 || window > MX_MULTIEXP_MAX_WINDOW) return MX_ERR_ARG;
  if (limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE) return MX_ERR_ARG;
  if (weight_bits > 2 * plan->n_bits + 64) return MX_ERR_ARG;                // the documented weight bound
  return narrow_launch(plan, limbs2, limbs_per_lane, o);
}

// Workspace of n_tables tables.  The table pass runs one group per table in one grid: at most 2^31 wavefronts — which
// also keeps the byte count (below 2^37 tables of at most 2^19 bytes) inside 64 bits.
int64_t tables_workspace_bytes(int n_bits, int64_t n_tables, int limbs_per_lane, int window) {
  if (window < 1 || window > MX_MULTIEXP_MAX_WINDOW) return MX_ERR_ARG;
  Geometry g;
  if (!multiexp_geometry(n_bits, limbs_per_lane, g)) return MX_ERR_SIZE;
  const int gpw = 64 / g.K;
  if ((n_tables + gpw - 1) / gpw >= MX_GRID_WAVEFRONTS) return MX_ERR_SIZE;
  return mx_multiexp_nsquare_workspace_bytes(n_bits, n_tables, limbs_per_lane, window);
}

// rows x blocks_per_row workgroups in one grid
inline bool rows_fit_grid(int64_t n_rows, int64_t blocks_per_row) { return n_rows <= MX_GRID_WAVEFRONTS / blocks_per_row - 1; }

// The maps with weights shared among positions (matmul: the samples of a tile; conv: the positions of the output grids),
// after the entry point's checks: the table pass over n_local + n_shared tables (d_inputs NULL: the tables already in the
// workspace, built by an earlier call with the same inputs and window), then the shared-weight pass — output row r at
// position p reads table column * stride + p (+ origin[p] where there are origins), out [p / image_positions][r][p % ..].
int launch_shared_map(const NarrowLaunch& o, const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_local,
                      int64_t n_shared, int limbs2, const int32_t* d_index, const uint32_t* d_weights, int terms,
                      int weight_bits, const int64_t* d_origin, int64_t stride, int64_t positions, int64_t image_positions,
                      uint32_t* d_out, int64_t n_rows, int window, void* d_ws, int64_t ws_bytes, hipStream_t s) {
  const int64_t pos_blocks = o.blocks(positions);
  if (!rows_fit_grid(n_rows, pos_blocks)) return MX_ERR_SIZE;                 // more wavefronts than one grid holds
  MX_TRY(workspace_fits(tables_workspace_bytes(plan->n_bits, n_local + n_shared, LIMBS_PER_LANE, window), ws_bytes));
  MxKernelTimer timer(s);
  if (d_inputs) MX_TRY(launch_table_pass(o, plan, d_inputs, n_local + n_shared, limbs2, window, d_ws, s));
  mx::SharedN2Args a{};
  a.tables = (const u32*)d_ws;
  a.consts = o.consts;
  a.index = d_index;
  a.weights = d_weights;
  a.origin = (const mx::i64*)d_origin;
  a.out = d_out;
  a.n_local = n_local; a.n_shared = n_shared; a.rows = n_rows;
  a.stride = (int)stride;
  a.image_positions = (int)image_positions;      // (conv: divides n_positions <= 2^30)
  a.positions = (int)positions; a.pos_blocks = (int)pos_blocks;
  a.terms = terms;
  a.window = window;
  weight_fields(terms, weight_bits, window, a.wwords, a.nwin);
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.nblk = o.g.nblk;
  return mxmm::launch_shared(o.g.K, a, n_rows * pos_blocks, s);
}
}  // namespace

extern "C" int mx_multiexp_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries) {
  static const int ks[] = {1, 2, 4, 8, 16, 32};
  const int n = (int)(sizeof(ks) / sizeof(ks[0]));
  if (max_entries < 0 || (max_entries > 0 && (!lanes || !limbs_per_lane))) return MX_ERR_ARG;
  for (int i = 0; i < n && i < max_entries; ++i) { lanes[i] = ks[i]; limbs_per_lane[i] = LIMBS_PER_LANE; }
  return n;
}

extern "C" int mx_multiexp_nsquare_shape(int n_bits, int64_t n_inputs, int64_t n_outputs, int64_t terms, int weight_bits,
                                         int limbs_per_lane, int window, int* lanes, int* limbs_per_lane_out,
                                         int* window_out, int64_t* chunk_terms) {
  if (!lanes || !limbs_per_lane_out || !window_out || !chunk_terms) return MX_ERR_ARG;
  if (n_inputs < 0 || n_outputs < 0 || terms < 0 || weight_bits < 0 || window < 0 || window > MX_MULTIEXP_MAX_WINDOW) return MX_ERR_ARG;
  Geometry g;
  if (limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE) return MX_ERR_ARG;
  if (!multiexp_geometry(n_bits, limbs_per_lane, g)) return MX_ERR_SIZE;
  *lanes = g.K;
  *limbs_per_lane_out = g.L;
  *window_out = window > 0 ? window : multiexp_window(n_inputs, n_outputs, terms, weight_bits);
  *chunk_terms = splitk_chunk(g, n_outputs, terms);
  return MX_OK;
}

extern "C" int64_t mx_multiexp_nsquare_workspace_bytes(int n_bits, int64_t n_inputs, int limbs_per_lane, int window) {
  Geometry g;
  if (n_inputs < 0 || window < 1 || window > MX_MULTIEXP_MAX_WINDOW) return MX_ERR_ARG;
  if (!multiexp_geometry(n_bits, limbs_per_lane, g)) return MX_ERR_SIZE;
  return align256((n_inputs > 0 ? n_inputs : 1) * ((int64_t)2 * g.K * g.L * 4 << window));
}

extern "C" int mx_multiexp_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_inputs, int limbs2,
                                       const int32_t* d_index, const uint32_t* d_weights, int terms, int weight_bits,
                                       uint32_t* d_out, int64_t n_outputs, int limbs_per_lane, int window, void* d_ws,
                                       int64_t ws_bytes, void* stream) {
  if (n_inputs <= 0) return MX_ERR_ARG;
  NarrowLaunch o;
  MX_TRY(weighted_launch(plan, d_out, d_ws, n_outputs, limbs2, d_index, d_weights, terms, weight_bits, limbs_per_lane, window, o));
  MX_TRY(workspace_fits(mx_multiexp_nsquare_workspace_bytes(plan->n_bits, n_inputs, LIMBS_PER_LANE, window), ws_bytes));
  mx::MultiexpN2Args a{};
  a.tables = (u32*)d_ws;
  a.consts = o.consts;
  a.index = d_index;
  a.weights = d_weights;
  a.out = d_out;
  a.n_inputs = n_inputs; a.rows = n_outputs;
  a.terms = terms;
  a.window = window;
  weight_fields(terms, weight_bits, window, a.wwords, a.nwin);
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.nblk = o.g.nblk;
  hipStream_t s = (hipStream_t)stream;
  MxKernelTimer timer(s);
  // (d_inputs NULL: the tables already in the workspace, built by an earlier call with the same inputs and window)
  if (d_inputs) MX_TRY(launch_table_pass(o, plan, d_inputs, n_inputs, limbs2, window, d_ws, s));
  return mxm::launch_multiexp(o.g.K, false, a, o.blocks(n_outputs), s);
}

// ---- packing modulo N^2 (mx_pack_n2.hpp): many small plaintexts per ciphertext ---------------------------------------
namespace mxp { int launch_pack(int K, const mx::PackN2Args& a, int64_t nblocks, hipStream_t s); }

extern "C" int mx_pack_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries) {
  return mx_multiexp_nsquare_instances(lanes, limbs_per_lane, max_entries);      // the same narrow instances
}

extern "C" int mx_pack_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_cts, int64_t count, int limbs2,
                                   int slot_bits, int slots, uint32_t* d_out, int limbs_per_lane, void* stream) {
  if (!plan || !plan->d_plan || !d_cts || !d_out || plan->limbs_n <= 0) return MX_ERR_ARG;
  if (count < 1 || slots < 1 || slot_bits < 1 || limbs2 <= 0 || limbs_per_lane < 0) return MX_ERR_ARG;
  const int bits = plan->n_bits;
  if ((int64_t)slot_bits * slots > bits - 2) return MX_ERR_ARG;     // a packed plaintext must decrypt unambiguously
  NarrowLaunch o;
  MX_TRY(narrow_launch(plan, limbs2, limbs_per_lane, o));
  mx::PackN2Args a;
  a.cts = d_cts;
  a.consts = o.consts;
  a.out = d_out;
  a.count = count;
  a.outputs = (count + slots - 1) / slots;
  a.slots = slots; a.slot_bits = slot_bits;
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.nblk = o.g.nblk; a.ksplit = bits - 1;
  hipStream_t s = (hipStream_t)stream;
  MxKernelTimer timer(s);
  return mxp::launch_pack(o.g.K, a, o.blocks(a.outputs), s);
}

// ---- fixed-base exponentiation modulo N^2 (mx_fixedbase_n2.hpp): encryption and re-randomisation ------------------------
namespace mxf { int launch_fixedbase(int K, int pass, const mx::FixedBaseN2Args& a, int64_t nblocks, hipStream_t s); }
namespace {
constexpr int MX_FIXEDBASE_MAX_WINDOW = 8;
constexpr int64_t MX_FIXEDBASE_TABLE_BUDGET = (int64_t)256 << 20;      // default budget of the window model
constexpr double MX_FIXEDBASE_TABLE_USES = 16.0;                       // calls a table is expected to serve (it is cached per key)
int64_t fixedbase_table_bytes(const Geometry& g, int exp_bits, int window) {
  const int64_t windows = (exp_bits + window - 1) / window;
  return align256(windows * ((int64_t)2 * g.K * g.L * 4 << window));
}
// Window of the fixed-base schedule, in pair products ONE GROUP executes one after the other.  Both passes spread over
// the machine, so what a pass costs is its products per group times the rounds of groups it needs (two wavefronts per
// SIMD resident): ceil(exp_bits / w) per round of outputs; for the table, built once, exp_bits squarings of the chain (the
// same for every w) plus 2 (w - 1) products per round of entries from digit 2 on.  (A first model summed the table's
// products as if one group built them all and chose w = 5 / 7 for 10^3 / 10^4 outputs, where w = 8 measured 1.6x / 1.15x
// faster and every table of a key took the same 8-9 ms.)  The table is kept per key, so a call is charged
// 1 / MX_FIXEDBASE_TABLE_USES of its pass: charged in full to one call of 10^3 outputs at key_length 4096 the model
// chose w = 7 (5.53 ms a call) where w = 8 takes 4.90 ms a call and 2 ms longer to build, once
// (profiles/r09_fixed_base_probe.txt).
int fixedbase_window(const Geometry& g, int exp_bits, int64_t count, int64_t budget) {
  const double resident = (double)device_cus() * 4 * 2 * (64 / g.K);
  auto rounds = [&](double groups) { return std::ceil(groups / resident); };
  int best = 1;
  double bestc = -1.0;
  for (int w = 1; w <= MX_FIXEDBASE_MAX_WINDOW; ++w) {
    if (w > 1 && fixedbase_table_bytes(g, exp_bits, w) > budget) break;
    const double nwin = (double)((exp_bits + w - 1) / w);
    const double table = (double)exp_bits + rounds(nwin * (double)((1 << w) - 2)) * 2.0 * (w - 1);
    const double c = rounds((double)count) * nwin + table / MX_FIXEDBASE_TABLE_USES;
    if (bestc < 0 || c < bestc) { bestc = c; best = w; }
  }
  return best;
}
bool fixedbase_args_ok(int bits, int exp_bits, int window) {
  return exp_bits >= 1 && exp_bits <= 2 * bits + 64 && window >= 1 && window <= MX_FIXEDBASE_MAX_WINDOW;
}
}  // namespace

extern "C" int mx_fixedbase_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries) {
  return mx_multiexp_nsquare_instances(lanes, limbs_per_lane, max_entries);      // the same narrow instances
}

extern "C" int mx_fixedbase_nsquare_shape(int n_bits, int exp_bits, int64_t count, int64_t table_budget_bytes,
                                          int limbs_per_lane, int window, int* lanes, int* limbs_per_lane_out,
                                          int* window_out, int* windows_out) {
  if (!lanes || !limbs_per_lane_out || !window_out || !windows_out) return MX_ERR_ARG;
  if (count < 1 || table_budget_bytes < 0 || window < 0 || limbs_per_lane < 0) return MX_ERR_ARG;
  if (!fixedbase_args_ok(n_bits, exp_bits, window ? window : 1)) return MX_ERR_ARG;
  if (limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE) return MX_ERR_ARG;
  Geometry g;
  if (!multiexp_geometry(n_bits, limbs_per_lane, g)) return MX_ERR_SIZE;
  const int w = window > 0 ? window
                           : fixedbase_window(g, exp_bits, count, table_budget_bytes ? table_budget_bytes : MX_FIXEDBASE_TABLE_BUDGET);
  *lanes = g.K;
  *limbs_per_lane_out = g.L;
  *window_out = w;
  *windows_out = (exp_bits + w - 1) / w;
  return MX_OK;
}

extern "C" int64_t mx_fixedbase_nsquare_table_bytes(int n_bits, int exp_bits, int limbs_per_lane, int window) {
  if (!fixedbase_args_ok(n_bits, exp_bits, window)) return MX_ERR_ARG;
  Geometry g;
  if (!multiexp_geometry(n_bits, limbs_per_lane, g)) return MX_ERR_SIZE;
  return fixedbase_table_bytes(g, exp_bits, window);
}

extern "C" int mx_fixedbase_nsquare_prepare(const mx_nsquare_plan* plan, const uint32_t* d_base, int limbs2, int exp_bits,
                                            int limbs_per_lane, int window, void* d_table, int64_t table_bytes,
                                            void* stream) {
  if (!plan || !plan->d_plan || !d_base || !d_table || plan->limbs_n <= 0 || limbs2 <= 0 || limbs_per_lane < 0) return MX_ERR_ARG;
  const int bits = plan->n_bits;
  if (!fixedbase_args_ok(bits, exp_bits, window)) return MX_ERR_ARG;
  NarrowLaunch o;
  MX_TRY(narrow_launch(plan, limbs2, limbs_per_lane, o));
  if (table_bytes < fixedbase_table_bytes(o.g, exp_bits, window)) return MX_ERR_ARG;
  mx::FixedBaseN2Args a{};
  a.base = d_base;
  a.table = (u32*)d_table;
  a.consts = o.consts;
  a.exp_bits = exp_bits; a.window = window; a.windows = (exp_bits + window - 1) / window;
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.nblk = o.g.nblk; a.ksplit = bits - 1;
  hipStream_t s = (hipStream_t)stream;
  MxKernelTimer timer(s);
  MX_TRY(mxf::launch_fixedbase(o.g.K, 0, a, 1, s));
  const int64_t fill = (int64_t)a.windows * ((1 << window) - 2);
  if (fill > 0) return mxf::launch_fixedbase(o.g.K, 1, a, o.blocks(fill), s);
  return MX_OK;
}

extern "C" int mx_fixedbase_nsquare_run(const mx_nsquare_plan* plan, const void* d_table, int exp_bits, int window, int mode,
                                        const uint32_t* d_exps, const uint32_t* d_operand, int operand_limbs,
                                        uint32_t* d_out, int64_t count, int limbs2, int limbs_per_lane, void* stream) {
  if (!plan || !plan->d_plan || !d_table || !d_exps || !d_out || plan->limbs_n <= 0) return MX_ERR_ARG;
  if (count < 1 || limbs2 <= 0 || limbs_per_lane < 0) return MX_ERR_ARG;
  if (mode != mx::FIXEDBASE_POWER && mode != mx::FIXEDBASE_ENCRYPT && mode != mx::FIXEDBASE_RANDOMIZE) return MX_ERR_ARG;
  const int bits = plan->n_bits;
  if (!fixedbase_args_ok(bits, exp_bits, window)) return MX_ERR_ARG;
  if (mode != mx::FIXEDBASE_POWER) {
    if (!d_operand || operand_limbs <= 0) return MX_ERR_ARG;
    const int64_t need = mode == mx::FIXEDBASE_ENCRYPT ? bits : 2 * bits;
    if (32 * (int64_t)operand_limbs < need) return MX_ERR_ARG;       // rows too narrow for N (ENCRYPT) or N^2
  }
  NarrowLaunch o;
  MX_TRY(narrow_launch(plan, limbs2, limbs_per_lane, o));
  if (mode != mx::FIXEDBASE_POWER && 2 * o.g.K * o.g.L + 8 < operand_limbs + 2) return MX_ERR_ARG;
  mx::FixedBaseN2Args a{};
  a.table = (u32*)d_table;
  a.consts = o.consts;
  a.exps = d_exps;
  a.operand = d_operand;
  a.out = d_out;
  a.count = count;
  a.exp_bits = exp_bits; a.ewords = (exp_bits + 31) / 32; a.window = window; a.windows = (exp_bits + window - 1) / window;
  a.mode = mode; a.oplimbs = mode == mx::FIXEDBASE_POWER ? 0 : operand_limbs;
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.nblk = o.g.nblk; a.ksplit = bits - 1;
  hipStream_t s = (hipStream_t)stream;
  MxKernelTimer timer(s);
  return mxf::launch_fixedbase(o.g.K, 2, a, o.blocks(count), s);
}

// ---- encrypted matrix products over a batch of ciphertext vectors (mx_matmul_n2.hpp) ---------------------------------
extern "C" int mx_matmul_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries) {
  return mx_multiexp_nsquare_instances(lanes, limbs_per_lane, max_entries);      // the same narrow instances
}

extern "C" int mx_matmul_nsquare_shape(int n_bits, int64_t n_cols, int64_t n_rows, int64_t terms, int weight_bits,
                                       int64_t batch, int64_t table_budget_bytes, int limbs_per_lane, int window,
                                       int* lanes, int* limbs_per_lane_out, int* window_out, int64_t* tile_batch,
                                       int64_t* chunk_terms) {
  if (!lanes || !limbs_per_lane_out || !window_out || !tile_batch || !chunk_terms) return MX_ERR_ARG;
  if (n_cols < 0 || n_rows < 0 || terms < 0 || weight_bits < 0 || batch < 0 || table_budget_bytes < 0) return MX_ERR_ARG;
  if (window < 0 || window > MX_MULTIEXP_MAX_WINDOW) return MX_ERR_ARG;
  if (limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE) return MX_ERR_ARG;
  Geometry g;
  if (!multiexp_geometry(n_bits, limbs_per_lane, g)) return MX_ERR_SIZE;
  // counts beyond what one launch takes (mx_matmul_nsquare_run) are refused here too; this keeps every product below
  // inside 64 bits: 2^31 columns of at most 2^20 bytes, 2^31 rows of at most 2^30 samples, and terms * outputs is formed
  // only for fewer outputs than fill the device
  if (n_cols > MX_GRID_WAVEFRONTS || n_rows > MX_GRID_WAVEFRONTS || terms > MX_GRID_WAVEFRONTS) return MX_ERR_SIZE;
  *lanes = g.K;
  *limbs_per_lane_out = g.L;
  // the window of ONE sample's map (every sample pays for its own tables), limited so that one sample's tables fit
  const int64_t entry_bytes = (int64_t)2 * g.K * g.L * 4;
  int w = window > 0 ? window : multiexp_window(n_cols, n_rows, terms, weight_bits);
  if (window == 0)
    while (w > 1 && n_cols * (entry_bytes << w) > table_budget_bytes) --w;
  *window_out = w;
  const int64_t per_sample = n_cols * (entry_bytes << w);
  int64_t tile = per_sample > 0 ? table_budget_bytes / per_sample : batch;
  if (tile > batch) tile = batch;
  if (tile > MX_MAX_POSITIONS) tile = MX_MAX_POSITIONS;
  if (tile < 1) tile = 1;
  *tile_batch = tile;
  *chunk_terms = splitk_chunk(g, n_rows * tile, terms);      // on the outputs of one tile
  return MX_OK;
}

extern "C" int64_t mx_matmul_nsquare_workspace_bytes(int n_bits, int64_t n_cols, int64_t n_shared, int64_t tile_batch,
                                                     int limbs_per_lane, int window) {
  if (n_cols < 0 || n_shared < 0 || tile_batch < 1 || tile_batch > MX_MAX_POSITIONS || n_cols > MX_GRID_WAVEFRONTS ||
      n_shared > MX_GRID_WAVEFRONTS) return MX_ERR_ARG;
  return tables_workspace_bytes(n_bits, n_cols * tile_batch + n_shared, limbs_per_lane, window);
}

extern "C" int mx_matmul_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_cols, int64_t n_shared,
                                     int64_t tile_batch, int limbs2, const int32_t* d_index, const uint32_t* d_weights,
                                     int terms, int weight_bits, uint32_t* d_out, int64_t n_rows, int limbs_per_lane,
                                     int window, void* d_ws, int64_t ws_bytes, void* stream) {
  if (n_cols < 0 || n_shared < 0 || n_cols > MX_GRID_WAVEFRONTS || n_shared > MX_GRID_WAVEFRONTS) return MX_ERR_ARG;
  if (tile_batch < 1 || tile_batch > MX_MAX_POSITIONS || n_cols * tile_batch + n_shared <= 0) return MX_ERR_ARG;
  NarrowLaunch o;
  MX_TRY(weighted_launch(plan, d_out, d_ws, n_rows, limbs2, d_index, d_weights, terms, weight_bits, limbs_per_lane, window, o));
  // the samples of the tile as positions: table column * tile + sample, out [tile][rows]
  return launch_shared_map(o, plan, d_inputs, n_cols * tile_batch, n_shared, limbs2, d_index, d_weights, terms, weight_bits,
                           nullptr, tile_batch, tile_batch, 1, d_out, n_rows, window, d_ws, ws_bytes, (hipStream_t)stream);
}

// ---- encrypted convolutions of ciphertext grids with a public kernel (mx_matmul_n2.hpp) ------------------------------
extern "C" int mx_conv_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries) {
  return mx_multiexp_nsquare_instances(lanes, limbs_per_lane, max_entries);      // the same narrow instances
}

extern "C" int64_t mx_conv_nsquare_workspace_bytes(int n_bits, int64_t n_local, int64_t n_shared, int limbs_per_lane,
                                                   int window) {
  if (n_local < 0 || n_shared < 0 || n_local + n_shared < 1 || n_local > MX_MAX_LOCAL_TABLES || n_shared > MX_GRID_WAVEFRONTS)
    return MX_ERR_ARG;
  return tables_workspace_bytes(n_bits, n_local + n_shared, limbs_per_lane, window);
}

extern "C" int mx_conv_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_local, int64_t n_shared,
                                   int limbs2, const int32_t* d_index, const uint32_t* d_weights, int terms,
                                   int weight_bits, const int64_t* d_origin, int64_t n_positions, int64_t image_positions,
                                   uint32_t* d_out, int64_t n_rows, int limbs_per_lane, int window, void* d_ws,
                                   int64_t ws_bytes, void* stream) {
  if (!d_origin) return MX_ERR_ARG;
  if (n_local < 0 || n_shared < 0 || n_local + n_shared < 1 || n_local > MX_MAX_LOCAL_TABLES || n_shared > MX_GRID_WAVEFRONTS)
    return MX_ERR_ARG;
  if (n_positions < 1 || n_positions > MX_MAX_POSITIONS || image_positions < 1 || n_positions % image_positions != 0) return MX_ERR_ARG;
  NarrowLaunch o;
  MX_TRY(weighted_launch(plan, d_out, d_ws, n_rows, limbs2, d_index, d_weights, terms, weight_bits, limbs_per_lane, window, o));
  // the table of the tap at position 0 + the position's origin, out [image][rows][position]
  return launch_shared_map(o, plan, d_inputs, n_local, n_shared, limbs2, d_index, d_weights, terms, weight_bits, d_origin, 1,
                           n_positions, image_positions, d_out, n_rows, window, d_ws, ws_bytes, (hipStream_t)stream);
}

// ---- encrypted histograms: sums of ciphertexts by a public bin index (mx_hist_n2.hpp) --------------------------------
namespace mxh { int launch_hist(int K, bool convert, const mx::HistN2Args& a, int64_t nblocks, hipStream_t s); }
namespace {
constexpr int MX_HIST_MAX_CHUNK = 1 << 16;
constexpr int MX_HIST_MIN_AUTO_CHUNK = 16, MX_HIST_MAX_AUTO_CHUNK = 4096;
// Terms per piece.  Enough pieces to give every SIMD of the device its three wavefronts (the kernel's launch bound),
// but pieces of at least 16 terms (a piece costs a launch slot and a row of output), at most 4096 — and, last, never
// longer than the mean segment rounded up: every segment is padded to whole pieces, so with many short segments
// (grouped statistics over many categories) a longer chunk would multiply by the one row more often than by a term.
int hist_chunk(const Geometry& g, int64_t n_segments, int64_t total_terms) {
  const int64_t target = (int64_t)device_cus() * 4 * 3 * (64 / g.K);
  int64_t chunk = (total_terms + target - 1) / target;
  if (chunk < MX_HIST_MIN_AUTO_CHUNK) chunk = MX_HIST_MIN_AUTO_CHUNK;
  if (chunk > MX_HIST_MAX_AUTO_CHUNK) chunk = MX_HIST_MAX_AUTO_CHUNK;
  const int64_t mean = n_segments > 0 ? (total_terms + n_segments - 1) / n_segments : total_terms;
  if (chunk > mean) chunk = mean;
  return (int)(chunk < 1 ? 1 : chunk);
}
int64_t hist_row_bytes(const Geometry& g) { return (int64_t)2 * g.K * g.L * 4; }
// a row count of the histogram and scan entries: at least `least`, and room for one more group (the one row)
inline bool row_count_ok(int64_t n, int64_t least) { return n >= least && n < MX_MAX_ROWS; }
// What the histogram and scan launches all refuse after their own arguments: a limbs_per_lane other than the narrow one
// (MX_ERR_ARG), the refusals of narrow_launch, and more groups than one grid holds wavefronts for (MX_ERR_SIZE).
int rows_launch(const mx_nsquare_plan* plan, int limbs2, int limbs_per_lane, int64_t groups, NarrowLaunch& o) {
  if (limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE) return MX_ERR_ARG;
  MX_TRY(narrow_launch(plan, limbs2, limbs_per_lane, o));
  return o.blocks(groups) >= MX_GRID_WAVEFRONTS ? MX_ERR_SIZE : MX_OK;
}
}  // namespace

// rows_launch for the entry points that live in a translation unit of their own (mx_capi_n2sp.hip): the lanes and
// blocks of the geometry, the plan's constant rows and the grid of `groups` groups.
namespace mxh {
int narrow_rows_launch(const mx_nsquare_plan* plan, int limbs2, int limbs_per_lane, int64_t groups, int* lanes, int* nblk,
                       const uint32_t** consts, int64_t* nblocks) {
  NarrowLaunch o;
  MX_TRY(rows_launch(plan, limbs2, limbs_per_lane, groups, o));
  *lanes = o.g.K; *nblk = o.g.nblk; *consts = o.consts; *nblocks = o.blocks(groups);
  return MX_OK;
}
}  // namespace mxh

extern "C" int mx_histogram_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries) {
  return mx_multiexp_nsquare_instances(lanes, limbs_per_lane, max_entries);      // the same narrow instances
}

extern "C" int mx_histogram_nsquare_shape(int n_bits, int64_t n_samples, int64_t n_segments, int64_t total_terms,
                                          int limbs_per_lane, int chunk, int* lanes, int* limbs_per_lane_out,
                                          int* chunk_out, int64_t* row_bytes) {
  if (!lanes || !limbs_per_lane_out || !chunk_out || !row_bytes) return MX_ERR_ARG;
  if (n_samples < 0 || n_segments < 0 || total_terms < 0 || chunk < 0 || chunk > MX_HIST_MAX_CHUNK) return MX_ERR_ARG;
  if (limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE) return MX_ERR_ARG;
  Geometry g;
  if (!multiexp_geometry(n_bits, limbs_per_lane, g)) return MX_ERR_SIZE;
  *lanes = g.K;
  *limbs_per_lane_out = g.L;
  *chunk_out = chunk > 0 ? chunk : hist_chunk(g, n_segments, total_terms);
  *row_bytes = hist_row_bytes(g);
  return MX_OK;
}

extern "C" int64_t mx_histogram_nsquare_workspace_bytes(int n_bits, int64_t n_rows, int limbs_per_lane) {
  Geometry g;
  if (!row_count_ok(n_rows, 0)) return MX_ERR_ARG;
  if (limbs_per_lane != 0 && limbs_per_lane != LIMBS_PER_LANE) return MX_ERR_ARG;
  if (!multiexp_geometry(n_bits, limbs_per_lane, g)) return MX_ERR_SIZE;
  return align256((n_rows + 1) * hist_row_bytes(g));
}

extern "C" int mx_histogram_nsquare_convert(const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_samples, int limbs2,
                                            uint32_t* d_rows, int64_t rows_bytes, int limbs_per_lane, void* stream) {
  if (!plan || !plan->d_plan || !d_inputs || !d_rows || plan->limbs_n <= 0) return MX_ERR_ARG;
  if (!row_count_ok(n_samples, 1) || limbs2 <= 0) return MX_ERR_ARG;
  NarrowLaunch o;
  MX_TRY(rows_launch(plan, limbs2, limbs_per_lane, n_samples + 1, o));       // one more group: the one row
  MX_TRY(workspace_fits(mx_histogram_nsquare_workspace_bytes(plan->n_bits, n_samples, LIMBS_PER_LANE), rows_bytes));
  mx::HistN2Args a{};
  a.inputs = d_inputs;
  a.rows_out = d_rows;
  a.consts = o.consts;
  a.n_samples = n_samples;
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.nblk = o.g.nblk; a.ksplit = plan->n_bits - 1;
  hipStream_t s = (hipStream_t)stream;
  MxKernelTimer timer(s);
  return mxh::launch_hist(o.g.K, true, a, o.blocks(n_samples + 1), s);
}

extern "C" int mx_histogram_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_rows, int64_t n_rows, const int32_t* d_index,
                                        int64_t n_pieces, int chunk, uint32_t* d_out, int pair_form_out, int limbs2,
                                        int64_t out_bytes, int limbs_per_lane, void* stream) {
  if (!plan || !plan->d_plan || !d_rows || !d_index || !d_out || plan->limbs_n <= 0) return MX_ERR_ARG;
  if (!row_count_ok(n_rows, 0) || n_pieces <= 0 || limbs2 <= 0) return MX_ERR_ARG;
  if (chunk < 1 || chunk > MX_HIST_MAX_CHUNK) return MX_ERR_ARG;
  NarrowLaunch o;
  const int64_t groups = n_pieces + (pair_form_out ? 1 : 0);                  // one more group: the one row of the next level
  MX_TRY(rows_launch(plan, limbs2, limbs_per_lane, groups, o));
  MX_TRY(workspace_fits(pair_form_out ? mx_histogram_nsquare_workspace_bytes(plan->n_bits, n_pieces, LIMBS_PER_LANE)
                                      : n_pieces * (int64_t)limbs2 * 4, out_bytes));
  mx::HistN2Args a{};
  a.rows = d_rows;
  a.consts = o.consts;
  a.index = d_index;
  a.out = d_out;
  a.n_rows = n_rows; a.pieces = n_pieces;
  a.chunk = chunk; a.pair_out = pair_form_out ? 1 : 0;
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.nblk = o.g.nblk; a.ksplit = plan->n_bits - 1;
  hipStream_t s = (hipStream_t)stream;
  MxKernelTimer timer(s);
  return mxh::launch_hist(o.g.K, false, a, o.blocks(groups), s);
}

// ---- encrypted prefix sums: running totals over series of ciphertexts (mx_scan_n2.hpp) -------------------------------
namespace mxh { int launch_scan(int K, bool store, const mx::ScanN2Args& a, int64_t nblocks, hipStream_t s); }

extern "C" int mx_scan_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries) {
  return mx_multiexp_nsquare_instances(lanes, limbs_per_lane, max_entries);      // the same narrow instances
}

extern "C" int mx_scan_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_rows, int64_t n_rows, const int32_t* d_index,
                                   int64_t n_pieces, int chunk, const uint32_t* d_carry_rows, int64_t n_carry_rows,
                                   const int32_t* d_carry_index, int exclusive, uint32_t* d_out, int limbs2, int64_t out_bytes,
                                   int limbs_per_lane, void* stream) {
  if (!plan || !plan->d_plan || !d_rows || !d_index || !d_out || plan->limbs_n <= 0) return MX_ERR_ARG;
  if (!row_count_ok(n_rows, 1) || n_pieces <= 0 || limbs2 <= 0) return MX_ERR_ARG;
  if (d_carry_rows && (!d_carry_index || !row_count_ok(n_carry_rows, 0))) return MX_ERR_ARG;
  if (chunk < 1 || chunk > MX_HIST_MAX_CHUNK) return MX_ERR_ARG;
  NarrowLaunch o;
  MX_TRY(rows_launch(plan, limbs2, limbs_per_lane, n_pieces + 1, o));         // one more group: the one row of the output set
  MX_TRY(workspace_fits(mx_histogram_nsquare_workspace_bytes(plan->n_bits, n_rows, LIMBS_PER_LANE), out_bytes));
  mx::ScanN2Args a{};
  a.rows = d_rows;
  a.carry_rows = d_carry_rows;
  a.consts = o.consts;
  a.index = d_index;
  a.carry_index = d_carry_rows ? d_carry_index : nullptr;
  a.out = d_out;
  a.n_rows = n_rows; a.n_carry_rows = d_carry_rows ? n_carry_rows : 0; a.pieces = n_pieces;
  a.chunk = chunk; a.exclusive = exclusive ? 1 : 0;
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.nblk = o.g.nblk;
  hipStream_t s = (hipStream_t)stream;
  MxKernelTimer timer(s);
  return mxh::launch_scan(o.g.K, false, a, o.blocks(n_pieces + 1), s);
}

extern "C" int mx_scan_nsquare_store(const mx_nsquare_plan* plan, const uint32_t* d_rows, int64_t n_rows, uint32_t* d_out,
                                     int limbs2, int64_t out_bytes, int limbs_per_lane, void* stream) {
  if (!plan || !plan->d_plan || !d_rows || !d_out || plan->limbs_n <= 0) return MX_ERR_ARG;
  if (!row_count_ok(n_rows, 1) || limbs2 <= 0) return MX_ERR_ARG;
  NarrowLaunch o;
  MX_TRY(rows_launch(plan, limbs2, limbs_per_lane, n_rows, o));
  MX_TRY(workspace_fits(n_rows * (int64_t)limbs2 * 4, out_bytes));
  mx::ScanN2Args a{};
  a.rows = d_rows;
  a.consts = o.consts;
  a.out = d_out;
  a.n_rows = n_rows;
  a.limbsn = plan->limbs_n; a.limbs2 = limbs2; a.nblk = o.g.nblk;
  hipStream_t s = (hipStream_t)stream;
  MxKernelTimer timer(s);
  return mxh::launch_scan(o.g.K, true, a, o.blocks(n_rows), s);
}
