// msm_plan.hpp — the host's plan of an MSM (csrc/msm.hip): tuning overrides, window layout, the decisions of make_plan and the layout of the
// workspace the kernels write.  Plain host C++ without a HIP header, so that a native check (tests/native/msm_plan_check.cpp) can compare
// every plan with recorded ones (tests/golden/msm_plans.txt) and replay the allocation arithmetic of the kernels without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>

// Tuning overrides of the MSM plan (benchmarks/sweep_window.py and friends): the BPPP_* environment is read ONCE, when the context is
// created; 0 / false = the library's heuristic.  No entry point reads the environment per call.
struct MsmTune {
  double gcost = 0;                // BPPP_GCOST: choose_window's cost of a bucket on the grouped reduction
  int cmin = 0;                    // BPPP_CMIN: narrowest window choose_window tries
  int lw = 0;                      // BPPP_LW: buckets per lane of k_reduce1
  int rg = 0;                      // BPPP_RG: lanes per window of k_reduce_groups
  int marg_s = 0;                  // BPPP_MARG_S: serial length per lane of k_reduce_marg
  int lacc = 0;                    // BPPP_LACC: sorted entries per lane of k_acc_points
  int window_batched = 0;          // BPPP_WINDOW_BATCHED: window width of a batch (> 4 instances) that names none
  int comb_wpe = 0;                // BPPP_COMB_WPE (csrc/comb.hip.h)
  int small_c = 0;                 // BPPP_MSM_SMALL_C: window width of the small route, 5..8
  int small_len = 0;               // BPPP_MSM_SMALL_LEN: terms per slice of the small route
  int small_max = 0;               // BPPP_MSM_SMALL_MAX: longest MSM on the small route
  int hist_ch = 0;                 // BPPP_HIST_CH: chunks per digit row of the sort, 1..64
  int num_cus = 0;                 // the device's compute units (bppp_ctx_create), not from the environment
  int sort_ranges = 4;             // bucket ranges per window of the ranged scatter, BPPP_SORT_RANGES: 0 = k_scatter
  int hist16 = 1;                  // per-chunk counts and cursors of a ranged scatter's sort as 16-bit values (MsmPlan::hist16), BPPP_HIST16: 0 = 32-bit words always
  int scatter_one_read = 1;        // the ranged scatter reads a chunk's digits once for all ranges (k_scatter_one_read), BPPP_SCATTER_ONE_READ: 0 = k_scatter_ranges always
  int acc_sized = -1;              // whole buckets by size (k_acc_points_sized), BPPP_ACC_SIZED: 1 = every one-MSM plan, 0 = none, -1 = the plans where it measured faster (plan_accumulate)
  int acc_fq29 = 1;                // the sized accumulation on 9 x 29-bit limbs (k_acc_points_sized29), BPPP_ACC_FQ29: not 0 = every sized plan (the default, by measurement: DESIGN.md 0.2), 0 = k_acc_points_sized on 10 x 26
  int acc_fast = 1;                // the fq29 accumulation on exception-free additions with one ZZ test per item, flagged items redone (k_acc_points_sized29_fast), BPPP_ACC_FAST: 0 = k_acc_points_sized29's complete addition in every step
  bool no_small = false;           // BPPP_MSM_NO_SMALL: the general pipeline for every length
  bool no_balance = false;         // BPPP_MSM_NO_BALANCE: uniform window widths
  size_t comb_rows_min_bytes = (size_t)4 << 30;   // BPPP_COMB_ROWS_MIN_MB (csrc/comb.hip.h)
  int comb_rows_waves = 0;         // BPPP_COMB_ROWS_WAVES (csrc/comb.hip.h)
  void from_env();
};

namespace bppp {

// bump allocator over the context workspace; over a null base it only adds up the size
struct Carver {
  char *base; size_t off = 0, cap;
  Carver(void *b, size_t c) : base((char *)b), cap(c) {}
  template <typename T> T *take(size_t count) {
    size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    T *p = (T *)(base ? base + off : nullptr);
    off += bytes;
    return p;
  }
};

// ---- constants the kernels and the plan agree on
static constexpr int MSM_XYZZ_WORDS = 40;                  // u32 per stored XYZZ point (XYZZ_WORDS of ec.hip.h; msm.hip asserts they agree)
static constexpr int SCAN_TILE = 4096;                     // buckets per workgroup of k_scan_apply and k_order
// An ITEM of the sized accumulation: a bucket of at most ACC_CAP entries, or a piece of ACC_CAP entries (the last one: the rest) of a larger
// one.  A bin of the size histogram has a 128-byte line (ACC_LINE words) to itself (k_scan_apply).
static constexpr uint32_t ACC_CAP = 128, ACC_LINE = 32;
static constexpr int SCATTER_AHEAD = 4;                    // 2^20 terms in 32 chunks of 1024 lanes: 4 steps, all in flight at once
static constexpr int MERGE_SERIAL_MAX = 8;                 // longer spans go to the wavefront-cooperative kernels
static constexpr int HEAVY_CHUNK = 256;                    // partial sums per wavefront in k_merge_heavy
static constexpr uint32_t MSM_SMALL_MAX = 4096;            // terms per slice (LDS: 6 bytes each)
static constexpr size_t MSM_SMALL_DEFAULT_MAX = 8192;      // terms per MSM on this route unless BPPP_MSM_SMALL_MAX says otherwise: every (window, slice) workgroup
                                                           // pays the ~17-operation reduction chain with most lanes idle, so the general pipeline wins from ~2^14 terms
                                                           // (benchmarks/sweep_small_msm.py: 858 terms 0.36 -> 0.21 ms, 4096 0.38 -> 0.27, 8192 0.40 -> 0.33, 22016 0.45 -> 0.43, 65536 0.52 -> 0.78)
// the pairs and quadruples of words the kernels read as uint2 / uint4 (same size and alignment)
struct MsmPair { uint32_t x, y; };
struct alignas(16) MsmQuad { uint32_t x, y, z, w; };

inline int choose_window(size_t n, size_t batch, const MsmTune &tune) {
  // Cost model in units of one mixed addition (~68 ps chip-wide, measured at 2^20; profiles/):
  //   accumulate: one addition per (scalar, window that holds real bits): ceil(255/c) windows (+ half a window when
  //               c divides 255: the top digit then wraps for half the scalars and a carry window appears — the only widths
  //               that still have one, window_layout);
  //   reduce:     ~10 per bucket (the wave-prefix bucket reduction is latency-bound; fitted at c = 13..16); ~3.5 per
  //               bucket for a large batch of small MSMs, which goes through k_reduce_groups (throughput-bound);
  //   heavy top:  when the top window has few real bits its buckets hold n / 2^r entries each and go through the
  //               wave-cooperative merge tree: a flat ~1.5e6 (0.1 ms) once they span many lanes.
  // One large MSM: the reduction is latency-bound and nearly flat in the bucket count (0.12 ms at c = 11 .. 0.26 ms at c = 16),
  // so the model above overprices wide windows; thresholds read off the (n, c, L) table of benchmarks/sweep_window.py
  // (profiles/r02_window_sweep.txt): c = 16 has 16 windows (17 when that table was read, window_layout) against 20 at c = 13 and no heavy top window.
  // (re-read after the balanced windows of plan_windows, which removed the heavy top window of every width that does not divide 256:
  // 9000-12000 terms 0.47 ms at c = 8 against 0.33 at c = 11; 22 016 terms 0.376 at c = 12; 43 782 terms 0.423 at c = 13)
  if (batch == 1 && n >= 4096) return n < 20000 ? 11 : n < 30000 ? 12 : n < 200000 ? 13 : 16;
  const double gcost = tune.gcost > 0 ? tune.gcost : 3.5;               // tuning sweeps override both
  const int cmin = tune.cmin ? std::max(2, tune.cmin) : 4;
  double best = 1e300; int bc = 8;
  for (int c = cmin; c <= 16; c++) {
    int full = 254 / c, r = 255 - c * full, W = full + 1 + (r == c ? 1 : 0);   // r = real bits in the top window (1..c); W as window_layout's
    double weff = full + 1 + (r == c ? 0.5 : 0.0);
    const bool groups = c <= 9 && (double)batch * W >= 4096.0;
    double cost = weff * (double)n + (groups ? gcost : 10.0) * W * (double)(1u << (c - 1));
    double top_bucket = r == c ? n / 2.0 : (double)n / (double)(1u << (r < 20 ? r : 20));
    if ((r == c || r < c - 1) && top_bucket > 1024.0) cost += 1.5e6;
    if (cost < best) { best = cost; bc = c; }
  }
  return bc;
}

// The windows of a scalar over arbitrary points.  A folded scalar has 255 bits (recode.hip.h) and the signed digits carry upwards, so the top
// window holds d in [0, 2^r] for its r real bits.  r <= cw - 2: d + 2^(cw-1) fits the window's cw bits as every other digit does.
// r = cw - 1: only d = 2^(cw-1) does not, and rather than a further window for that one carry the top window is left unbiased and stored
// negated (top = its index; k_digits, k_msm_small) — its largest magnitude is then the bucket of -2^(cw-1) that every window has.
// r = cw (uniform widths, c divides 255): half of the scalars carry, the window above stays.
//   balanced (one MSM, c does not divide 256): ceil(256 / c) windows, the first acnt c bits wide, the others c - 1; r = cw - 1 always;
//   uniform: ceil(255 / c) windows, r = cw - 1 exactly when c divides 256 (16 windows at c = 16, 32 at c = 8), + 1 when c divides 255.
// A registered basis (flat plans, basis.hip, comb.hip) keeps 256 / c + 1 biased rows: its tables are laid out by them.
struct WindowLayout { int W, acnt, top; };
inline WindowLayout window_layout(int c, bool balanced) {
  WindowLayout l;
  if (balanced) {
    l.W = (256 + c - 1) / c; l.acnt = 256 - l.W * (c - 1); l.top = l.W - 1;
  } else {
    const int T = (255 + c - 1) / c, r = 255 - c * (T - 1);
    l.W = T + (r == c ? 1 : 0); l.acnt = l.W; l.top = r == c - 1 ? l.W - 1 : -1;
  }
  return l;
}

// ---- the small route: ONE MSM of a few thousand terms in k_msm_small (+ k_msm_small_join), msm.hip section 0
struct MsmSmallPlan {
  int c, W, acnt, top;         // window width and layout (window_layout)
  size_t len, S;               // terms per slice, slices
  size_t lds;                  // k_msm_small's dynamic LDS request, bytes
};
inline bool msm_small_route(size_t n, size_t batch, int window_bits, size_t table_stride, bool to_device, const MsmTune &tune) {
  const size_t small_max = tune.small_max ? (size_t)tune.small_max : MSM_SMALL_DEFAULT_MAX;
  return batch == 1 && !table_stride && !window_bits && n <= small_max && !tune.no_small && !to_device;
}
inline MsmSmallPlan make_small_plan(size_t n, const MsmTune &tune) {
  MsmSmallPlan s;
  s.c = tune.small_c >= 5 && tune.small_c <= 8 ? tune.small_c : 6;
  const int M = 1 << (s.c - 1);
  const WindowLayout wl = window_layout(s.c, 256 % s.c != 0 && !tune.no_balance);
  s.W = wl.W; s.acnt = wl.acnt; s.top = wl.top;
  s.len = tune.small_len >= 64 && tune.small_len <= (int)MSM_SMALL_MAX ? (size_t)tune.small_len : (n <= 2048 ? 512 : 1024);
  if (n <= s.len + s.len / 2) s.len = n;                              // a second slice has to pay for the join launch
  s.S = (n + s.len - 1) / s.len;
  // hist[M], start[M + 1], sorted[len], key[len] (u16), rounded to 16 bytes; then M + 4 bucket sums and wavefront results
  s.lds = (((size_t)(2 * M + 1) + s.len + (s.len + 1) / 2 + 3) & ~(size_t)3) * 4 + (size_t)(M + 4) * MSM_XYZZ_WORDS * 4;
  return s;
}
struct MsmSmallWorkspace { uint32_t *partials, *winsum; };
inline MsmSmallWorkspace carve_small(Carver &cv, const MsmSmallPlan &s) {
  MsmSmallWorkspace w;
  w.partials = cv.take<uint32_t>((size_t)s.W * s.S * MSM_XYZZ_WORDS);
  w.winsum = cv.take<uint32_t>((size_t)s.W * MSM_XYZZ_WORDS);
  return w;
}

// ---- the general pipeline
// k_reduce_marg / k_reduce_tail_quad: the bucket index splits as i = hi * LO + lo (msm.hip section 4'); rows and columns are summed by PR / PC
// lanes of SR / SC buckets each, and the tail works on TR = HI / 16 row and TC = LO / 16 column blocks of 16 elements
struct MargGeom { int a, LO, HI, PR, PC, SR, SC; uint32_t row_tiles, col_tiles; int TR, TC; };

struct MsmPlan {
  size_t n, batch; int c, W, acnt, M, CH, hist_threads, Lw, WPW;   // acnt: windows [0, acnt) are c bits wide, the others c - 1
  int top;                     // the digit row stored negated (window_layout), -1: none
  bool flat;                   // precomputed table 2^(c w) P_i: all windows of an instance share ONE bucket set
  int Wc;                      // windows left for the window combine (1 when flat)
  uint64_t NB, NS, FB, total_max;   // digit rows (batch * W), bucket sets (batch * W, or batch when flat), buckets, sorted entries
  int L; uint64_t G;           // sorted entries per lane, number of lanes
  int RG;                      // k_reduce_groups lanes per window (0 = wave-per-window path)
  bool marg; MargGeom mg;      // marginal-sum reduction (M >= 256, not the grouped path)
  int ntiles;
  int Q;                       // bucket ranges per window of the ranged scatter (k_scatter_ranges, k_scatter_one_read); 0 = k_scatter
  bool one_read;               // ranged scatter from (window, chunk) workgroups that read their digits once (k_scatter_one_read)
  bool hist16;                 // blockhist holds 16-bit counts, then 16-bit prefixes modulo 2^16 (k_hist, k_count_tiles16, the ranged scatters), in the front half of its allocation
  bool sized;                  // accumulate whole buckets in order of size (k_order, k_acc_points_sized) instead of slices of L entries
  bool fq29;                   // sized, with the accumulator in 9 x 29-bit limbs (k_acc_points_sized29)
  bool acc_fast;               // fq29, with the exception-free additions and one test per item (k_acc_points_sized29_fast)
};

// windows: n, batch, c, flat, W, acnt, top, M, Wc and the counts that follow from them
inline void plan_windows(MsmPlan &p, size_t n, size_t batch, int c, bool flat, const MsmTune &tune) {
  p.n = n; p.batch = batch; p.c = c; p.W = 256 / c + 1; p.M = 1 << (c - 1);
  p.acnt = p.W; p.top = -1;
  // Balanced windows (one MSM over arbitrary points, c not a divisor of 256): with uniform widths the top window holds only
  // 256 - c floor(256 / c) real bits, i.e. a few buckets with n / 2^r entries each — the "heavy" merges (0.05 ms at 2^16 terms, c = 13:
  // 256 buckets of 256 entries).  Instead ceil(256 / c) windows of widths c (the low ones) and c - 1 share the 256 bits, so every
  // window's buckets are evenly filled.
  if (!flat) {
    const WindowLayout l = window_layout(c, batch == 1 && c >= 3 && 256 % c != 0 && !tune.no_balance);
    p.W = l.W; p.acnt = l.acnt; p.top = l.top;
  }
  p.flat = flat; p.Wc = flat ? 1 : p.W;
  p.NB = (uint64_t)batch * p.W; p.NS = flat ? batch : p.NB; p.FB = p.NS * p.M; p.total_max = p.NB * n;
  p.ntiles = (int)((p.FB + SCAN_TILE - 1) / SCAN_TILE);
}

// sort: hist_threads, the chunk count CH (k_hist, k_count_tiles and the blockhist layout use it too), the scatter's form Q and one_read
inline void plan_sort(MsmPlan &p, const MsmTune &tune) {
  const size_t n = p.n, batch = p.batch;
  p.hist_threads = p.M >= 8192 ? 1024 : 256;
  size_t per_block = (size_t)p.hist_threads * 64;
  p.CH = (int)std::max<size_t>(1, std::min<size_t>(64, (n + per_block - 1) / per_block));
  // ranged scatter (k_scatter_ranges, k_scatter_one_read): a window is cut into as many chunks as an XCD has CUs (num_cus / 8: 32) and ONE
  // workgroup is resident per CU (the launches' LDS requests), so that the workgroups of one (window, range) unit fill an XCD and ONE unit is
  // live per L2: 1 MiB of `sorted` (n * 4 / Q bytes for evenly spread digits) at 2^20 terms and Q = 4, a quarter of the L2.  A second live
  // unit — two workgroups per CU, or the wavefronts of k_scatter_one_read left to drift over the ranges — loses the merging.
  // Measured with k_scatter_ranges, loads four steps ahead, sort stage: Q = 4 0.175 / 0.176 / 0.222 ms at 16 / 32 / 64 chunks, Q = 2 0.258 /
  // 0.171 / 0.221 (k_scatter: 0.248 / 0.268 / 0.284); under k_scatter_one_read Q = 2 at 32 chunks is no faster than Q = 4.  A shorter
  // input takes fewer chunks, of the same length, but never fewer than the rule above gives.
  p.Q = 0;
  if (batch == 1 && !p.flat && (size_t)p.M * 4 > 80 * 1024 && tune.num_cus >= 8 && (tune.sort_ranges == 2 || tune.sort_ranges == 4)) {
    p.Q = tune.sort_ranges;
    const uint64_t cus = (uint64_t)tune.num_cus / 8, unit_bytes = (uint64_t)n * 4 / p.Q;
    const uint64_t ch = (cus * unit_bytes + (1u << 20) - 1) >> 20;
    p.CH = (int)std::min<uint64_t>(std::min<uint64_t>(cus, 64), std::max<uint64_t>((uint64_t)p.CH, ch));
  } else if ((size_t)p.M * 4 > 80 * 1024 && tune.num_cus > 0) {
    // the histogram of a wide window (>= 80 KB of LDS) leaves room for ONE k_hist / k_scatter workgroup per CU: a grid a few workgroups
    // over a whole number of rounds (17 windows x 16 chunks on 256 CUs) runs a nearly empty extra round — take the chunk count that fills
    // the rounds instead (15: sort stage 0.301 -> 0.277 ms at 2^20)
    const double rounds = (double)p.NB * p.CH / tune.num_cus;
    if (rounds >= 0.75) {
      const uint64_t r = (uint64_t)(rounds + 0.5) ? (uint64_t)(rounds + 0.5) : 1;
      const uint64_t ch = r * (uint64_t)tune.num_cus / p.NB;
      if (ch >= 1 && ch <= 64 && 4 * ch >= 3 * (uint64_t)p.CH) p.CH = (int)ch;
    }
  }
  if (tune.hist_ch >= 1 && tune.hist_ch <= 64) p.CH = tune.hist_ch;
  // one read of the digits (k_scatter_one_read): a lane holds SCATTER_AHEAD steps of 8 digits in registers, so the form is possible exactly
  // when a chunk is no longer than that many steps of the workgroup — a rule in steps per lane, whatever n and the chunk count are.  With the
  // chunk rule above that is every n up to 2^15 x (CUs of an XCD); a longer chunk keeps k_scatter_ranges, which refills its registers.
  // Its W x CH workgroups run one per CU and each lasts Q range passes, so the form is taken only for grids that fill their rounds:
  // - at least one whole round.  A smaller grid is a shorter MSM that often shares the chip with another stream's: two verifiers at once
  //   (345 k terms each, 176 workgroups) ran 2.25 -> 2.34 ms per batch with the long workgroups, for 0.007 ms less sort stage when alone;
  // - no last round for fewer than a quarter of the CUs, which costs a whole workgroup's time for little work where k_scatter_ranges'
  //   workgroups of one pass each fill the CUs evenly — 17 chunks of 16 windows on 256 CUs (16 workgroups in the second round): sort stage
  //   0.127 ms ranged, 0.134 read once; 20 chunks (64): 0.139 either way; 16 and 24 to 32 chunks are faster read once.
  // Every other plan keeps k_scatter_ranges too.
  const uint64_t chunk = ((((uint64_t)n + p.CH - 1) / p.CH) + 7u) & ~(uint64_t)7, lane_steps = (chunk + (uint64_t)p.hist_threads * 8 - 1) / ((uint64_t)p.hist_threads * 8);
  const uint64_t wgs = (uint64_t)p.W * p.CH, cus = (uint64_t)std::max(tune.num_cus, 1), last_round = wgs % cus;
  const bool full_rounds = wgs >= cus && !(last_round && 4 * last_round < cus);
  p.one_read = p.Q && tune.scatter_one_read && lane_steps <= (uint64_t)SCATTER_AHEAD && full_rounds;
  // 16-bit per-chunk histograms under a ranged scatter: a chunk's count of a bucket is at most the chunk's length, and a bucket's prefix over
  // the chunks is kept modulo 2^16 — exact for every bucket of fewer than 65536 entries; the scatters rebuild a larger ("wide") bucket's prefix
  // from the wraps in its stored sequence (scatter_load_cursors16, msm.hip).  Half the bytes of k_hist's output, of k_count_tiles' pass in place
  // and of the scatters' cursor loads.  The arrays take the front half of the blockhist allocation: carve() is the same either way.
  p.hist16 = p.Q && chunk <= 65535 && tune.hist16 != 0;
}

// bucket reduction: k_reduce1/2 (Lw, WPW), k_reduce_groups (RG) or the marginal sums (marg, mg)
inline void plan_reduce(MsmPlan &p, const MsmTune &tune) {
  // lanes per window T = M / Lw, at most 64 wavefronts per window
  if (p.M <= 64) { p.Lw = 1; p.WPW = 1; }
  else {
    p.Lw = 1;
    while (p.M / p.Lw > 64 * 64) p.Lw <<= 1;     // cap at 4096 lanes per window
    if (p.M / p.Lw >= 1024 && p.Lw < 4) p.Lw = std::min(4, p.M / 1024);  // amortise the wave scan
    if (p.Lw < 1) p.Lw = 1;
    if (tune.lw) { const int v = tune.lw; if (v >= 1 && (v & (v - 1)) == 0 && p.M / v >= 64 && p.M / v <= 4096) p.Lw = v; }
    p.WPW = p.M / p.Lw / 64;
    if (p.WPW < 1) p.WPW = 1;
  }
  p.RG = 0;
  if (p.M <= 256 && p.NS >= 4096) {                            // M is a power of two >= 2
    // lanes per window: the serial part costs 2 additions per bucket, the in-group scan and tree ~3 log2(RG) more per lane, so
    // keep >= 16 buckets per lane (RG = 8 on 8 buckets is 11 additions per bucket, RG = 1 is 2) unless the launch would
    // then be under ~2 wavefronts per SIMD
    const int cap = std::min(8, p.M);
    p.RG = std::max(1, std::min(cap, p.M / 16));
    while (p.RG < cap && p.NS * (uint64_t)p.RG < 131072) p.RG <<= 1;
    if (tune.rg) { const int v = tune.rg; if (v >= 1 && v <= cap && (v & (v - 1)) == 0) p.RG = v; }
  }
  p.marg = !p.RG && p.M >= 256 && p.NS <= 65535;
  memset(&p.mg, 0, sizeof p.mg);
  if (p.marg) {
    MargGeom &g = p.mg;
    g.a = (p.c - 1 + 1) / 2; g.LO = 1 << g.a; g.HI = p.M / g.LO;        // LO >= HI, both <= 256
    // serial length S per lane: about one wavefront per SIMD over the whole launch (2 * FB bucket reads over ~64K lanes)
    int S = 1;
    while (S < 16 && (2.0 * (double)p.FB) / S > 98304.0) S <<= 1;
    if (tune.marg_s) { const int v = tune.marg_s; if (v >= 1 && v <= 64 && (v & (v - 1)) == 0) S = v; }
    g.SR = std::min(S, g.LO); g.SC = std::min(S, g.HI);
    g.PR = g.LO / g.SR; g.PC = g.HI / g.SC;
    while (g.PR > 64) { g.PR >>= 1; g.SR <<= 1; }                        // the segmented tree lives inside one wavefront
    while (g.PC > 64) { g.PC >>= 1; g.SC <<= 1; }
    g.row_tiles = (uint32_t)(((size_t)g.HI * g.PR + 63) / 64); g.col_tiles = (uint32_t)(((size_t)g.LO * g.PC + 63) / 64);
    // M >= 256: c is 9..16, so LO = 2^a is in [16, 256] and HI = M / LO in [16, 128]: at least one row block, at most 16 column blocks,
    // which is what k_reduce_tail_quad's second step (one quad per block) holds
    g.TR = g.HI / 16; g.TC = g.LO / 16;
  }
}

// accumulation: the slice length L and lane count G of k_acc_points, or whole buckets by size (sized, fq29)
inline void plan_accumulate(MsmPlan &p, const MsmTune &tune) {
  const size_t n = p.n, batch = p.batch;
  // slice length: short enough to keep >= ~150K lanes (two to four wavefronts per SIMD), but at least a quarter of a bucket's
  // expected entries, so that a bucket straddles few lanes and stays on the serial merge path (sweep_window.py table)
  if (batch == 1 && !p.flat) {
    const uint64_t occ = n / (uint64_t)p.M;
    int lo = 8; while (lo < 64 && (uint64_t)(4 * lo) < occ) lo <<= 1;
    p.L = 64; while (p.L > lo && p.total_max / (uint64_t)p.L < 150000) p.L >>= 1;
  } else {
    p.L = 4;
    while (p.L < 64 && p.total_max / (uint64_t)(2 * p.L) >= 65536) p.L <<= 1;
  }
  // one bucket set for all windows: buckets hold W times more entries; a longer slice keeps a bucket within a few lanes (the
  // serial merge path) while the launch still has two wavefronts per SIMD
  // (L = 256 leaves one wavefront per SIMD and the gathers are no longer hidden: 1.39 ms against 1.15 ms at 2^20)
  if (p.flat) while (p.L < 128 && (double)p.total_max / (double)p.FB > 4.0 * p.L && p.total_max / (uint64_t)(2 * p.L) >= 65536) p.L <<= 1;
  if (tune.lacc >= 1 && tune.lacc <= 4096) p.L = tune.lacc;
  p.G = (p.total_max + p.L - 1) / p.L; if (!p.G) p.G = 1;
  // sized accumulation: one MSM over arbitrary points.  The default is by measurement ("whole buckets by size"): at 2^20 terms
  // and c = 16 the accumulation stage falls 1.113 -> 1.010 ms; at 2^16 and c = 13 it has 86 K items of 16 entries, a third of the chip's wave
  // slots on chains twice as long as the slices', and rises 0.186 -> 0.311 ms
  p.sized = batch == 1 && !p.flat && (tune.acc_sized > 0 || (tune.acc_sized < 0 && p.c == 16));
  // on 9 x 29-bit limbs by default ("9 x 29-bit limbs"): accumulation 1.010 -> 0.892 ms at 2^20 terms, 8 interleaved pairs
  p.fq29 = p.sized && tune.acc_fq29 != 0;
  p.acc_fast = p.fq29 && tune.acc_fast != 0;
}

inline MsmPlan make_plan(size_t n, size_t batch, int c, bool flat, const MsmTune &tune) {
  MsmPlan p;
  plan_windows(p, n, batch, c, flat, tune);
  plan_sort(p, tune);
  plan_reduce(p, tune);
  plan_accumulate(p, tune);
  return p;
}

// ---- launch figures that follow from the plan
// dynamic LDS of k_hist, k_scatter and k_scatter_one_read: a counter or cursor per bucket of a window
inline size_t sort_lds_bytes(const MsmPlan &p) { return (size_t)p.M * 4; }
// k_scatter_ranges keeps the cursors of one range (M * 4 / Q bytes); the request is for more than half of a CU's 160 KiB, so that ONE workgroup is
// resident per CU (k_scatter_ranges)
inline size_t ranges_lds_bytes(const MsmPlan &p) { return std::max<size_t>(sort_lds_bytes(p) / p.Q, 84 * 1024); }
// 1-D grids of the ranged scatters: 8 slots x ceil(units / 8) x CH chunks, a unit being a (window, range) or, read once, a window
inline uint32_t ranges_units(const MsmPlan &p) { return (uint32_t)p.W * p.Q; }
inline uint32_t ranged_grid(const MsmPlan &p) { return 8u * (((p.one_read ? (uint32_t)p.W : ranges_units(p)) + 7) / 8) * p.CH; }

// ---- capacities of the accumulation's lists
// sized: a bucket of several pieces has more than ACC_CAP entries and ceil(count / ACC_CAP) <= 2 count / ACC_CAP pieces, so there are at
// most total / ACC_CAP such buckets, 2 total / ACC_CAP piece sums (they take rec_pt's place) and total / ACC_CAP + 2 total / (ACC_CAP *
// HEAVY_CHUNK) (bucket, chunk) items; every non-empty bucket adds at most one item to the total / ACC_CAP full pieces
inline size_t sized_tcap(const MsmPlan &p) { return (size_t)(p.total_max / ACC_CAP); }
inline size_t sized_items_max(const MsmPlan &p) { return std::min<size_t>((size_t)p.total_max, (size_t)p.FB + sized_tcap(p)); }
// partial sums in rec_pt: the sized route's piece slots, or a head and a tail slot per lane of k_acc_points
inline size_t partial_slots(const MsmPlan &p) { return p.sized ? 2 * sized_tcap(p) + 2 : (size_t)p.G * 2; }
// heavy buckets span > 9 lanes: at most G/9 of them, and at most G/256 + G/9 (bucket, chunk) items
inline size_t heavy_max(const MsmPlan &p) { return p.sized ? sized_tcap(p) + 2 * sized_tcap(p) / HEAVY_CHUNK + 4 : (size_t)(p.G / 8 + 2); }
// counters and tickets, zeroed by k_digits (with the scan's tile sums): [0], [1] heavy items / buckets, [2], [3] the sized route's piece
// slots / items, [4..] k_reduce_tail_quad's tickets, then the sized route's size histogram and class cursors
inline size_t tail_tickets(const MsmPlan &p) { return p.marg ? 2 * (size_t)p.NS : 0; }
inline size_t counter_words(const MsmPlan &p) { return 4 + tail_tickets(p) + (p.sized ? 2 * ACC_CAP * ACC_LINE : 0); }

struct MsmWorkspace {
  uint32_t stride;             // u16 per digit row: n rounded up to 8 (rows are 16-byte aligned)
  uint16_t *dig; unsigned long long *negmask;
  uint32_t *blockhist, *count, *start, *tiles, *sorted, *buckets;
  uint32_t *rec_pt;            // partial sums: partial_slots
  MsmPair *items; size_t items_max; uint32_t *piece_base;            // sized route only
  size_t hmax; MsmPair *heavy_items; MsmQuad *heavy_buckets; uint32_t *chunk_sums, *heavy_slot;
  size_t nzero; uint32_t *heavy_count, *tail_cnt, *size_hist, *cursors;   // the counter block (counter_words) and its parts; the last two sized only, else null
  uint32_t *tail_part, *red, *winsum, *out_aff;
};
inline MsmWorkspace carve(Carver &cv, const MsmPlan &p, size_t n, size_t batch) {
  MsmWorkspace w;
  w.stride = (uint32_t)((n + 7) & ~(size_t)7);     // digit rows are 16-byte aligned
  w.dig = cv.take<uint16_t>((size_t)p.NB * w.stride + 8);
  w.negmask = cv.take<unsigned long long>((batch * n + 63) / 64 + 1);
  w.blockhist = cv.take<uint32_t>((size_t)p.NB * p.CH * p.M);
  w.count = cv.take<uint32_t>(p.FB + 1);
  w.start = cv.take<uint32_t>(p.FB + 1);
  w.tiles = cv.take<uint32_t>(p.ntiles + 1);
  w.sorted = cv.take<uint32_t>(p.total_max + 4);
  w.buckets = cv.take<uint32_t>((size_t)p.FB * MSM_XYZZ_WORDS);
  w.items_max = sized_items_max(p);
  w.rec_pt = cv.take<uint32_t>(partial_slots(p) * MSM_XYZZ_WORDS);
  w.items = cv.take<MsmPair>(p.sized ? w.items_max + 1 : 0);
  w.piece_base = cv.take<uint32_t>(p.sized ? (size_t)p.FB : 0);
  w.hmax = heavy_max(p);
  w.heavy_items = cv.take<MsmPair>(w.hmax);
  w.heavy_buckets = cv.take<MsmQuad>(w.hmax);
  w.chunk_sums = cv.take<uint32_t>(w.hmax * MSM_XYZZ_WORDS);
  w.nzero = counter_words(p);
  w.heavy_count = cv.take<uint32_t>(w.nzero);
  w.tail_cnt = w.heavy_count + 4;
  w.size_hist = p.sized ? w.tail_cnt + tail_tickets(p) : nullptr; w.cursors = p.sized ? w.size_hist + ACC_CAP * ACC_LINE : nullptr;
  w.tail_part = cv.take<uint32_t>(p.marg ? (size_t)p.NS * 2 * 16 * 2 * MSM_XYZZ_WORDS : 0);   // (A_b, S_b) of <= 16 blocks per (window, kind)
  w.red = cv.take<uint32_t>(p.marg ? (size_t)p.NS * (p.mg.HI + p.mg.LO) * MSM_XYZZ_WORDS : (size_t)p.NS * p.WPW * 2 * MSM_XYZZ_WORDS);
  w.winsum = cv.take<uint32_t>((size_t)p.NS * 2 * MSM_XYZZ_WORDS);
  w.out_aff = cv.take<uint32_t>((size_t)batch * 16);
  w.heavy_slot = cv.take<uint32_t>(w.hmax);     // per heavy item: its bucket's entry in heavy_buckets (the chunks' ticket)
  return w;
}

}  // namespace bppp
