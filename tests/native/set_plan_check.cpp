// set_plan_check.cpp — the host's share of the set commitments (csrc/rpset_plan.hpp) replayed without a GPU.  Nodes are their names (level, index), so
// no hash is needed: the replay walks an append exactly as k_rp_set_leaf and k_rp_set_tree (csrc/rpset.hip.h) index it — tile by tile, lane by lane,
// level by level, through a model of the 256-node LDS buffer — over a full store and over a frontier with its two scratch buffers, and checks that
//   every node the definition gives the set of n + m rows, and no other, is created, exactly once, from its own two children;
//   every read finds a node that exists: LDS slots written by this tile at the level below, the store below a level's node count, the frontier slot
//   of a peak of n, the scratch buffers inside tops_nodes;
//   after the merge the frontier holds the peaks of n + m, and chains of appends give what one append gives;
//   locate and path_slot agree with a plain walk over the peaks for every leaf of every n < 2^11 and sampled n beyond, and h + p + 1 <= bit_length (n)
//   for every n < 2^14; the level arrays only grow and hold what is asked of them;
//   grow_levels is all or nothing: with an allocation, a copy or the table upload failing at every possible call, the store, what it holds and
//   the table the kernels would read are as before, nothing leaks, nothing live is freed, and the same growth succeeds afterwards.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <set>
#include <string.h>
#include <random>
#include <utility>
#include <vector>
#include "rpset_plan.hpp"

using namespace bppp_set;
typedef std::pair<uint32_t, uint64_t> Node;                     // (level, index)
static const Node NONE(~0u, 0);

#define CHECK(c)                                                                          \
  do {                                                                                    \
    if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); }          \
  } while (0)

struct Model {
  bool keep;
  uint64_t n = 0;
  std::vector<std::vector<Node>> lvl;                           // a full store: lvl[k] sized by grow ()
  std::vector<Node> front;                                      // a frontier: MAX_LEVELS slots
  Model(bool k) : keep(k), lvl(FULL_LEVELS), front(MAX_LEVELS, NONE) {}
};

static void append(Model &S, uint64_t m) {
  if (!m) return;
  const uint64_t n = S.n, N = n + m;
  CHECK(N <= (S.keep ? FULL_MAX_N : FRONTIER_MAX_N));
  if (S.keep)
    for (uint32_t k = 0; k < FULL_LEVELS; k++) {
      const uint64_t c = grow(S.lvl[k].size(), level_nodes(N, k));
      CHECK(c >= level_nodes(N, k) && c >= S.lvl[k].size());
      S.lvl[k].resize(c, NONE);
    }
  std::vector<Node> leaves(S.keep ? 0 : m, NONE), tops[2], front_new(MAX_LEVELS, NONE);
  tops[0].assign(S.keep ? 0 : tops_nodes(m, 0), NONE); tops[1].assign(S.keep ? 0 : tops_nodes(m, 1), NONE);
  // made[k][j - (n >> k)]: node (k, j) was created; the index is in range exactly when is_new (n, N, k, j)
  std::vector<std::vector<bool>> made(MAX_LEVELS);
  for (uint32_t k = 0; k < MAX_LEVELS; k++) made[k].assign(shr(N, k) - shr(n, k), false);
  uint64_t nmade = 0;
  auto make_once = [&](const Node &v) {
    CHECK(v.first < MAX_LEVELS && v.second >= shr(n, v.first) && v.second - shr(n, v.first) < made[v.first].size());
    CHECK(!made[v.first][v.second - shr(n, v.first)]);
    made[v.first][v.second - shr(n, v.first)] = true;
    nmade++;
  };
  for (uint64_t t = 0; t < m; t++) {                            // k_rp_set_leaf
    if (S.keep) { CHECK(n + t < S.lvl[0].size()); S.lvl[0][n + t] = Node(0, n + t); } else leaves[t] = Node(0, n + t);
    make_once(Node(0, n + t));
  }
  auto front_put = [&](uint32_t lev, uint64_t idx, Node v) { if (has_peak(N, lev) && idx == peak_index(N, lev)) front_new[lev] = v; };
  const std::vector<Pass> passes = append_passes(n, m);
  CHECK(!passes.empty() && passes.size() <= (bit_length(N) + TILE_BITS - 1) / TILE_BITS);
  const std::vector<Node> *in = &leaves;
  for (size_t q = 0; q < passes.size(); q++) {
    const Pass &P = passes[q];
    CHECK(P.L == TILE_BITS * q && P.tiles >= 1);
    std::vector<Node> &out = tops[q & 1];
    const uint64_t in_base = n >> P.L, out_base = shr(n, P.L + TILE_BITS);
    for (uint64_t g = 0; g < P.tiles; g++) {                    // k_rp_set_tree, workgroup g
      const uint64_t tile = P.tile0 + g;
      std::vector<Node> lds(TILE, NONE);
      for (uint32_t j = 0; j < TILE; j++) {
        const uint64_t idx = (tile << TILE_BITS) + j;
        if (!is_new(n, N, P.L, idx)) continue;
        Node v;
        if (S.keep) { CHECK(idx < S.lvl[P.L].size()); v = S.lvl[P.L][idx]; } else { CHECK(idx - in_base < in->size()); v = (*in)[idx - in_base]; }
        CHECK(v == Node(P.L, idx));
        lds[j] = v;
        if (!S.keep && P.L == 0) front_put(P.L, idx, v);
      }
      for (uint32_t k = 1; k <= TILE_BITS; k++) {
        const uint32_t lev = P.L + k;
        if (shr(N, lev) <= shr(n, lev)) break;
        std::vector<Node> next(TILE, NONE);
        for (uint32_t j = 0; j < (TILE >> k); j++) {
          const uint64_t idx = (tile << (TILE_BITS - k)) + j;
          if (!is_new(n, N, lev, idx)) continue;
          const uint64_t left = 2 * idx;
          Node a;
          if (left >= shr(n, lev - 1)) a = lds[2 * j];
          else {
            CHECK(has_peak(n, lev - 1) && left == peak_index(n, lev - 1));
            if (S.keep) { CHECK(left < level_nodes(n, lev - 1)); a = S.lvl[lev - 1][left]; } else a = S.front[lev - 1];
          }
          const Node b = lds[2 * j + 1];
          CHECK(a == Node(lev - 1, left) && b == Node(lev - 1, left + 1));
          next[j] = Node(lev, idx);
          make_once(next[j]);
          if (S.keep) { CHECK(lev < FULL_LEVELS && idx < S.lvl[lev].size()); S.lvl[lev][idx] = next[j]; }
          else {
            front_put(lev, idx, next[j]);
            if (k == TILE_BITS) { CHECK(idx - out_base < out.size()); out[idx - out_base] = next[j]; }
          }
        }
        for (uint32_t j = 0; j < (TILE >> k); j++) if (!(next[j] == NONE)) lds[j] = next[j];      // a lane that makes nothing leaves its slot
      }
    }
    in = &out;
  }
  uint64_t want = 0;                                            // exactly the nodes of the definition
  for (uint32_t k = 0; k < 64; k++) want += shr(N, k) - shr(n, k);
  CHECK(nmade == want);
  if (!S.keep)
    for (uint32_t k = 0; k < MAX_LEVELS; k++) if (peak_is_new(n, N, k)) { CHECK(!(front_new[k] == NONE)); S.front[k] = front_new[k]; }
  S.n = N;
  for (uint32_t k = 0; k < MAX_LEVELS; k++) {
    if (!has_peak(N, k)) continue;
    const Node pk(k, peak_index(N, k));
    CHECK(S.keep ? S.lvl[k][pk.second] == pk : S.front[k] == pk);
  }
  if (S.keep) for (uint32_t k = 0; k < FULL_LEVELS; k++) for (uint64_t j = 0; j < level_nodes(N, k); j++) CHECK(S.lvl[k][j] == Node(k, j));
}

static void check_paths(uint64_t n, uint64_t i) {
  // the plain walk: the peaks from the highest down
  uint32_t h = 0, p = 0, m = 0;
  uint64_t start = 0;
  bool found = false;
  for (int k = 63; k >= 0; k--) {
    if (!((n >> k) & 1)) continue;
    if (!found) { if (i < start + ((uint64_t)1 << k)) { h = (uint32_t)k; p = m; found = true; } else start += (uint64_t)1 << k; }
    m++;
  }
  const Locate L = locate(n, i);
  CHECK(found && L.h == h && L.p == p && L.m == m && L.used == h + p + (p + 1 < m ? 1 : 0));
  const uint32_t len = bit_length(n);
  CHECK(L.used <= len && path_bytes(n) == 32 * (size_t)len);
  uint32_t nonzero = 0, next_peak = p;
  for (uint32_t s = 0; s < len; s++) {
    const Slot sl = path_slot(n, i, L, s);
    if (sl.kind == SLOT_ZERO) { CHECK(s >= L.used); continue; }
    CHECK(s == nonzero && s < L.used);
    nonzero++;
    if (sl.kind == SLOT_SIBLING) CHECK(s < h && sl.level == s && sl.index == ((i >> s) ^ 1) && sl.index < level_nodes(n, s) && (sl.index >> (h - s)) == (i >> h));
    else if (sl.kind == SLOT_RIGHT_BAG) CHECK(s == h && p + 1 < m && sl.peak == p + 1);
    else { CHECK(next_peak >= 1 && sl.peak == next_peak - 1 && has_peak(n, sl.level) && sl.index == peak_index(n, sl.level) && peak_level(n, sl.peak) == sl.level); next_peak--; }
  }
  CHECK(nonzero == L.used && next_peak == 0);
}

// ---- the growth of the level arrays with an allocator, a copy and a table upload that fail on demand: whichever call fails, the store, its
// capacities, what the arrays hold and the published table are as before, nothing leaks and nothing live was freed (the arrays are real
// allocations, so the sanitizer sees a read through a stale table)
struct StubOps {
  int fail_alloc = -1, fail_copy = -1, fail_publish = -1, allocs = 0, copies = 0, publishes = 0;
  std::set<void *> live;
  uint32_t *table[LEVEL_SLOTS] = {};
  void *alloc(size_t bytes) { if (allocs++ == fail_alloc) return nullptr; void *p = malloc(bytes); CHECK(p); memset(p, 0xDD, bytes); live.insert(p); return p; }
  void release(void *p) { CHECK(live.erase(p) == 1); free(p); }
  bool copy(void *dst, const void *src, size_t bytes) { if (copies++ == fail_copy) return false; memcpy(dst, src, bytes); return true; }
  bool publish(uint32_t *const *t) { if (publishes++ == fail_publish) return false; for (uint32_t k = 0; k < LEVEL_SLOTS; k++) table[k] = t[k]; return true; }
};
static void fill(LevelStore &S, uint64_t from, uint64_t to) {      // node (k, j) holds 8 words of k * 2^24 + j, for the rows [from, to)
  for (uint32_t k = 0; k < FULL_LEVELS; k++) for (uint64_t j = level_nodes(from, k); j < level_nodes(to, k); j++) for (int q = 0; q < 8; q++) S.lvl[k][j * 8 + q] = (k << 24) + (uint32_t)j;
}
static void holds(const StubOps &ops, const LevelStore &S, uint64_t n) {
  std::set<void *> mine;
  for (uint32_t k = 0; k < LEVEL_SLOTS; k++) {
    CHECK(ops.table[k] == S.lvl[k] && (S.lvl[k] != nullptr) == (S.cap[k] != 0));
    if (S.lvl[k]) mine.insert(S.lvl[k]);
    if (k < FULL_LEVELS) { CHECK(S.cap[k] >= level_nodes(n, k)); for (uint64_t j = 0; j < level_nodes(n, k); j++) for (int q = 0; q < 8; q++) CHECK(ops.table[k][j * 8 + q] == (k << 24) + (uint32_t)j); }
  }
  CHECK(mine == ops.live);
}
static void check_growth() {
  int failed[3] = {0, 0, 0};
  const uint64_t steps[][2] = {{0, 1}, {0, 1000}, {1000, 70000}, {70000, 70001}, {70001, 300000}};
  for (int kind = 0; kind < 3; kind++)
    for (const auto &st : steps) {
      // how many calls of each kind the step makes when nothing fails
      int calls = 0;
      for (int f = -1; f < (f == -1 ? 0 : calls) || f == -1; f++) {
        StubOps ops;
        LevelStore S;
        CHECK(grow_levels(S, 0, st[0], ops) == GROW_OK);
        fill(S, 0, st[0]);
        holds(ops, S, st[0]);
        const LevelStore before = S;
        const int a0 = ops.allocs, c0 = ops.copies, p0 = ops.publishes;
        if (f >= 0) (kind == 0 ? ops.fail_alloc : kind == 1 ? ops.fail_copy : ops.fail_publish) = (kind == 0 ? a0 : kind == 1 ? c0 : p0) + f;
        const GrowResult r = grow_levels(S, st[0], st[1], ops);
        if (f < 0) {
          CHECK(r == GROW_OK);
          calls = kind == 0 ? ops.allocs - a0 : kind == 1 ? ops.copies - c0 : ops.publishes - p0;
          fill(S, st[0], st[1]);
          holds(ops, S, st[1]);
          for (uint32_t k = 0; k < FULL_LEVELS; k++) CHECK(S.cap[k] >= before.cap[k] && (S.cap[k] == before.cap[k]) == (S.lvl[k] == before.lvl[k]));
          CHECK(grow_levels(S, st[1], st[1], ops) == GROW_OK && ops.allocs - a0 == (kind == 0 ? calls : ops.allocs - a0));      // nothing to grow: no call
        } else {
          CHECK(r == (kind == 0 ? GROW_ALLOC_FAILED : kind == 1 ? GROW_COPY_FAILED : GROW_PUBLISH_FAILED));
          failed[kind]++;
          for (uint32_t k = 0; k < LEVEL_SLOTS; k++) CHECK(S.lvl[k] == before.lvl[k] && S.cap[k] == before.cap[k]);
          holds(ops, S, st[0]);
          ops.fail_alloc = ops.fail_copy = ops.fail_publish = -1;                   // and the set goes on: the same growth succeeds afterwards
          CHECK(grow_levels(S, st[0], st[1], ops) == GROW_OK);
          fill(S, st[0], st[1]);
          holds(ops, S, st[1]);
        }
        for (uint32_t k = 0; k < LEVEL_SLOTS; k++) if (S.lvl[k]) ops.release(S.lvl[k]);
        CHECK(ops.live.empty());
        if (f == -1 && calls == 0) break;
      }
    }
  CHECK(failed[0] >= 30 && failed[1] >= 10 && failed[2] == 5);      // every allocation, every copy and every upload of the five steps failed once
}

int main() {
  check_growth();
  std::mt19937_64 rnd(7);
  const uint64_t n0s[] = {0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 70000};
  const uint64_t ms[] = {1, 2, 3, 255, 256, 257, 700, 65536, 65537};
  for (int keep = 0; keep < 2; keep++) {
    for (uint64_t n0 : n0s)
      for (uint64_t m : ms) {
        Model S(keep != 0);
        append(S, n0);                                           // one append from empty, then the append under test
        append(S, m);
      }
    for (int chain = 0; chain < 6; chain++) {                    // chains of appends of 0 .. 600 rows
      Model S(keep != 0);
      for (int c = 0; c < 40; c++) append(S, rnd() % 601);
    }
  }
  {                                                              // far up: a frontier near 2^62, a full store at its last row
    Model S(false);
    S.n = ((uint64_t)1 << 62) - 3;
    for (uint32_t k = 0; k < MAX_LEVELS; k++) if (has_peak(S.n, k)) S.front[k] = Node(k, peak_index(S.n, k));
    append(S, 1); append(S, 1); append(S, 1); append(S, 700);
    CHECK(append_passes(FRONTIER_MAX_N - 1, 1).size() == 1 && append_passes(((uint64_t)1 << 62) - 1, 1).size() == 8);
  }
  for (uint64_t n = 1; n < (1u << 14); n++) {
    uint32_t worst = 0;
    for (uint32_t p = 0; p < popcount(n); p++) { const uint32_t u = peak_level(n, p) + p + 1; worst = u > worst ? u : worst; }
    CHECK(worst <= bit_length(n));
    if (n < (1u << 11)) for (uint64_t i = 0; i < n; i++) check_paths(n, i);
    else for (int r = 0; r < 8; r++) check_paths(n, rnd() % n);
  }
  for (int r = 0; r < 20000; r++) { const uint64_t n = (rnd() >> (rnd() % 63)) % FRONTIER_MAX_N + 1; check_paths(n, rnd() % n); check_paths(n, n - 1); check_paths(n, 0); }
  CHECK(bit_length(0) == 0 && path_bytes(0) == 0 && leaf_blocks(1) == 1 && leaf_blocks(23) == 1 && leaf_blocks(24) == 2 && leaf_blocks(87) == 2 && leaf_blocks(88) == 3 &&
        leaf_blocks(8192) == 129);
  printf("replays ok\n");
  return 0;
}
