// msm_plan_check.cpp — the host's plan of an MSM (csrc/msm_plan.hpp) checked without a GPU, in three parts:
//  1. every line of tests/golden/msm_plans.txt (recorded from the code before the plan moved into its header) is recomputed and must
//     come out the same: inputs, route, every field of the plan, the workspace's size and the offset of each of its buffers;
//  2. every plan satisfies the relations the kernels rely on (chunks cover the row, LDS requests, grid limits, reduction geometry);
//  3. the allocation arithmetic of k_order and of k_merge's heavy registration is replayed on integers over bucket-count vectors that
//     stress the capacities carve() gives the lists: no count may exceed its buffer.
// Built with the sanitizers by tests/test_msm_plan_host.py.
//
// A fixture line, all numbers:  n batch window_bits flat table_stride  sort_ranges hist_ch scatter_one_read acc_sized acc_fq29 marg_s
// no_balance no_small lw rg lacc  route  and then, route 1 (small):  c W acnt top len S lds_bytes workspace_bytes;  route 0 (general):
// c W acnt M CH hist_threads Lw WPW top flat Wc NB NS FB total_max L G RG marg a LO HI PR PC SR SC row_tiles col_tiles TR TC ntiles Q
// one_read sized fq29 workspace_bytes and the 20 buffer offsets in carve() order.  num_cus = 256 throughout.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <fstream>
#include <random>
#include <set>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>
#include "msm_plan.hpp"

using namespace bppp;

#define REQUIRE(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n  at: %s\n", __FILE__, __LINE__, #c, g_line.c_str()); return 1; } } while (0)
static std::string g_line;

// carve() with the offset of every buffer recorded.  The layout is taken over a reserved, inaccessible address range of the workspace's size,
// so that the pointers carve() hands out are real addresses that nothing here can read or write.
struct Layout { MsmWorkspace ws; size_t bytes; std::vector<size_t> offs; };
static bool layout(const MsmPlan &p, Layout &l) {
  Carver sizing(nullptr, 0);
  carve(sizing, p, p.n, p.batch);
  l.bytes = sizing.off;
  char *base = (char *)mmap(nullptr, l.bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (base == (char *)MAP_FAILED) return false;
  Carver cv(base, l.bytes);
  l.ws = carve(cv, p, p.n, p.batch);
  const MsmWorkspace &w = l.ws;
  const void *ptrs[] = {w.dig, w.negmask, w.blockhist, w.count, w.start, w.tiles, w.sorted, w.buckets, w.rec_pt, w.items, w.piece_base, w.heavy_items,
                        w.heavy_buckets, w.chunk_sums, w.heavy_count, w.tail_part, w.red, w.winsum, w.out_aff, w.heavy_slot};
  l.offs.clear();
  for (const void *q : ptrs) l.offs.push_back((size_t)((const char *)q - base));
  const bool same = cv.off == l.bytes;
  munmap(base, l.bytes);
  return same;
}

static const uint64_t GRID_X = 0x7FFFFFFFull, GRID_Y = 65535, LDS_MAX = 160 * 1024;

static int check_small(const MsmSmallPlan &s, size_t n) {
  REQUIRE(s.len * s.S >= n && s.len <= n && (s.S == 1 || s.len <= MSM_SMALL_MAX));
  REQUIRE(s.lds <= 64 * 1024);                              // k_msm_small gets no hipFuncSetAttribute
  REQUIRE((uint64_t)s.W <= GRID_X && s.S <= GRID_Y && (1 << (s.c - 1)) <= 256);
  return 0;
}

static int check_relations(const MsmPlan &p, const Layout &l) {
  const uint64_t n = p.n;
  // sort
  const uint64_t per = (((n + p.CH - 1) / p.CH) + 7u) & ~(uint64_t)7;
  REQUIRE(p.CH >= 1 && per % 8 == 0 && per * p.CH >= n && l.ws.stride % 8 == 0 && l.ws.stride >= n);
  REQUIRE(p.Q == 0 || (p.M % p.Q == 0 && (p.M / p.Q) % 4 == 0));
  const uint64_t lane_steps = (per + (uint64_t)p.hist_threads * 8 - 1) / ((uint64_t)p.hist_threads * 8);
  REQUIRE(!p.one_read || (p.Q && lane_steps <= (uint64_t)SCATTER_AHEAD));
  // LDS
  REQUIRE(sort_lds_bytes(p) <= LDS_MAX);
  if (p.Q) {
    REQUIRE(ranges_lds_bytes(p) <= LDS_MAX && 2 * ranges_lds_bytes(p) > LDS_MAX && ranges_lds_bytes(p) >= sort_lds_bytes(p) / p.Q);
    REQUIRE(2 * sort_lds_bytes(p) > LDS_MAX);               // k_scatter_one_read: one workgroup per CU too
    REQUIRE(p.hist_threads == 1024 && p.batch == 1 && !p.flat);
  }
  // accumulate and reduce
  REQUIRE(p.L >= 1 && p.G * (uint64_t)p.L >= p.total_max);
  REQUIRE(!p.fq29 || p.sized);
  if (p.marg) {
    const MargGeom &g = p.mg;
    REQUIRE(!p.RG && g.LO * g.HI == p.M && g.PR * g.SR == g.LO && g.PC * g.SC == g.HI);
    REQUIRE(g.PR >= 1 && g.PR <= 64 && g.PC >= 1 && g.PC <= 64 && (g.PR & (g.PR - 1)) == 0 && (g.PC & (g.PC - 1)) == 0);
    REQUIRE(g.TR >= 1 && g.TC <= 16 && g.TR * 16 == g.HI && g.TC * 16 == g.LO && g.TR <= 16);
    REQUIRE((uint64_t)g.row_tiles * 64 >= (uint64_t)g.HI * g.PR && (uint64_t)g.col_tiles * 64 >= (uint64_t)g.LO * g.PC);
  } else if (p.RG) {
    REQUIRE((p.RG & (p.RG - 1)) == 0 && p.RG <= std::min(8, p.M));
  } else {
    REQUIRE(p.Lw >= 1 && p.WPW >= 1 && p.WPW <= 64 && (uint64_t)p.WPW * 64 * p.Lw >= (uint64_t)p.M);
  }
  // grids: x, y of every launch of the general pipeline
  const uint64_t gx[] = {(p.batch * n + 255) / 256, p.NB, (p.FB + 255) / 256, (uint64_t)p.ntiles, p.Q ? ranged_grid(p) : 0, (l.ws.items_max + 255) / 256,
                         (p.G + 255) / 256, (p.NS * (uint64_t)p.RG + 63) / 64, (uint64_t)p.mg.row_tiles + p.mg.col_tiles, (uint64_t)(p.mg.TR + p.mg.TC), p.NS,
                         (p.batch + 63) / 64};
  for (uint64_t x : gx) REQUIRE(x <= GRID_X);
  REQUIRE((uint64_t)p.CH <= GRID_Y && (uint64_t)p.WPW <= GRID_Y && (!p.marg || p.NS <= GRID_Y));
  REQUIRE((uint64_t)p.ntiles * SCAN_TILE >= p.FB);
  return 0;
}

// ---- part 3: bucket-count vectors.  A bucket set holds at most `budget` entries (n per digit row: a scalar leaves at most one entry per
// window; a flat plan's set takes all W rows).  Every kind of vector fills the buckets of a set in order while that budget lasts.
struct Counts {
  const MsmPlan &p; uint64_t budget;
  explicit Counts(const MsmPlan &pl) : p(pl), budget(pl.flat ? (uint64_t)pl.W * pl.n : pl.n) {}
  template <class F> void each(int kind, uint64_t v, uint64_t seed, F f) const {   // f(count) for every bucket, in bucket order
    std::mt19937_64 rng(seed);
    for (uint64_t s = 0; s < p.NS; s++) {
      uint64_t left = budget;
      for (int m = 0; m < p.M; m++) {
        uint64_t c;
        if (kind == 0) c = m == 0 ? left : 0;                                    // everything in one bucket
        else if (kind == 1) c = std::min(left, v);                               // v per bucket
        else if (kind == 2) c = std::min(left, m == 0 ? (uint64_t)1 : v);        // one entry, then v per bucket: every run starts one past a slice boundary
        else { const unsigned k = rng() % 16; c = std::min(left, k < 8 ? rng() % 4 : k < 14 ? rng() % 300 : k < 15 ? rng() % 5000 : left); }
        left -= c;
        f((uint32_t)c);
      }
    }
  }
};

static int replay(const MsmPlan &p, const Layout &l, int kind, uint64_t v, uint64_t seed) {
  const MsmWorkspace &w = l.ws;
  uint64_t start = 0, items = 0, slots = 0, chunk_items = 0, multi = 0, top_slot = 0;
  Counts(p).each(kind, v, seed, [&](uint32_t cnt) {
    if (!cnt) return;
    if (p.sized) {                                          // k_order
      const uint32_t full = cnt / ACC_CAP, rem = cnt % ACC_CAP;
      items += full + (rem ? 1 : 0);
      if (cnt > ACC_CAP) {
        const uint32_t np = full + (rem ? 1u : 0u), nch = (np + HEAVY_CHUNK - 1) / HEAVY_CHUNK;
        slots += np; chunk_items += nch; multi += nch > 1;
      }
    } else {                                                // k_acc_points' slots, k_merge
      const uint64_t g0 = start / (uint32_t)p.L, g1 = (start + cnt - 1) / (uint32_t)p.L;
      if (g0 != g1) {
        const uint32_t np = (uint32_t)(g1 - g0 + 1);
        top_slot = std::max(top_slot, 2 * g1 + 1);          // partial_ptr: tail slot 2 g0 + 1, head slots 2 (g0 + t) and k_acc_points' own 2 g + 1
        if (np > (uint32_t)MERGE_SERIAL_MAX + 1) { const uint32_t nch = (np + HEAVY_CHUNK - 1) / HEAVY_CHUNK; chunk_items += nch; multi += nch > 1; }
      }
    }
    start += cnt;
  });
  REQUIRE(start <= p.total_max);
  REQUIRE(chunk_items <= w.hmax && multi <= w.hmax);        // heavy_items / heavy_slot / chunk_sums, heavy_buckets
  if (p.sized) { REQUIRE(items <= w.items_max && slots <= partial_slots(p)); }
  else REQUIRE(top_slot < partial_slots(p) || !top_slot);
  return 0;
}

static int check_capacities(const MsmPlan &p, const Layout &l) {
  const uint64_t L = (uint64_t)p.L;
  if (replay(p, l, 0, 0, 0)) return 1;
  for (uint64_t v : {(uint64_t)1, (uint64_t)ACC_CAP, (uint64_t)ACC_CAP + 1, (uint64_t)2 * ACC_CAP - 1, (uint64_t)HEAVY_CHUNK * ACC_CAP + 1})
    if (replay(p, l, 1, v, 0)) return 1;
  // every bucket on exactly MERGE_SERIAL_MAX + 2 lanes: (MERGE_SERIAL_MAX + 1) L entries from one past a slice boundary; and the same with
  // HEAVY_CHUNK lanes more, so that every bucket has two chunks
  for (uint64_t v : {(uint64_t)(MERGE_SERIAL_MAX + 1) * L, (uint64_t)(MERGE_SERIAL_MAX + 1) * L + 1, (uint64_t)(HEAVY_CHUNK - 1) * L, (uint64_t)HEAVY_CHUNK * L})
    if (replay(p, l, 2, v, 0)) return 1;
  for (uint64_t seed = 1; seed <= 3; seed++) if (replay(p, l, 3, 0, 20261019 + seed)) return 1;
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { printf("usage: msm_plan_check tests/golden/msm_plans.txt\n"); return 2; }
  std::ifstream in(argv[1]);
  std::string line;
  int lines = 0, small = 0, replayed = 0;
  std::set<std::tuple<uint64_t, uint64_t, uint64_t, int, int, int, int>> seen;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    g_line = line;
    std::istringstream is(line);
    size_t n, batch, table_stride; int window_bits, flat, route, no_balance, no_small;
    MsmTune t; t.num_cus = 256;
    is >> n >> batch >> window_bits >> flat >> table_stride >> t.sort_ranges >> t.hist_ch >> t.scatter_one_read >> t.acc_sized >> t.acc_fq29 >> t.marg_s >> no_balance >>
        no_small >> t.lw >> t.rg >> t.lacc >> route;
    REQUIRE(!is.fail() && flat == (table_stride != 0));
    t.no_balance = no_balance != 0; t.no_small = no_small != 0;
    std::ostringstream os;
    os << n << ' ' << batch << ' ' << window_bits << ' ' << flat << ' ' << table_stride << ' ' << t.sort_ranges << ' ' << t.hist_ch << ' ' << t.scatter_one_read << ' '
       << t.acc_sized << ' ' << t.acc_fq29 << ' ' << t.marg_s << ' ' << no_balance << ' ' << no_small << ' ' << t.lw << ' ' << t.rg << ' ' << t.lacc << ' ';
    REQUIRE((route == 1) == msm_small_route(n, batch, window_bits, table_stride, false, t));
    if (route == 1) {
      const MsmSmallPlan s = make_small_plan(n, t);
      Carver cv(nullptr, 0);
      carve_small(cv, s);
      os << 1 << ' ' << s.c << ' ' << s.W << ' ' << s.acnt << ' ' << s.top << ' ' << s.len << ' ' << s.S << ' ' << s.lds << ' ' << cv.off;
      REQUIRE(os.str() == line);
      if (check_small(s, n)) return 1;
      small++; lines++;
      continue;
    }
    const int c = window_bits ? window_bits : choose_window(n, batch, t);
    const MsmPlan p = make_plan(n, batch, c, flat != 0, t);
    Layout l;
    REQUIRE(layout(p, l));
    const MargGeom &g = p.mg;
    os << 0 << ' ' << p.c << ' ' << p.W << ' ' << p.acnt << ' ' << p.M << ' ' << p.CH << ' ' << p.hist_threads << ' ' << p.Lw << ' ' << p.WPW << ' ' << p.top << ' ' << (int)p.flat
       << ' ' << p.Wc << ' ' << p.NB << ' ' << p.NS << ' ' << p.FB << ' ' << p.total_max << ' ' << p.L << ' ' << p.G << ' ' << p.RG << ' ' << (int)p.marg << ' ' << g.a << ' '
       << g.LO << ' ' << g.HI << ' ' << g.PR << ' ' << g.PC << ' ' << g.SR << ' ' << g.SC << ' ' << g.row_tiles << ' ' << g.col_tiles << ' ' << g.TR << ' ' << g.TC << ' '
       << p.ntiles << ' ' << p.Q << ' ' << (int)p.one_read << ' ' << (int)p.sized << ' ' << (int)p.fq29 << ' ' << l.bytes;
    for (size_t o : l.offs) os << ' ' << o;
    if (os.str() != line) { printf("FAILED: the plan differs from the recorded one\n  recorded:   %s\n  recomputed: %s\n", line.c_str(), os.str().c_str()); return 1; }
    // the limits msm_run_ex checks before it plans or launches
    REQUIRE(c >= 2 && c <= 16 && p.FB < (1ull << 32) - 1 && p.total_max < (1ull << 32) - 1);
    if (check_relations(p, l)) return 1;
    // the replay walks every bucket: plans of up to 2^20 buckets, one of each shape
    if (p.FB <= (1u << 20) && seen.insert(std::make_tuple(p.FB, p.total_max, (uint64_t)p.n, p.L, p.M, (int)p.sized, (int)p.flat)).second) {
      if (check_capacities(p, l)) return 1;
      replayed++;
    }
    lines++;
  }
  if (lines < 100) { printf("FAILED: only %d fixture lines read from %s\n", lines, argv[1]); return 1; }
  printf("%d plans ok (%d small), %d replayed\n", lines, small, replayed);
  return 0;
}
