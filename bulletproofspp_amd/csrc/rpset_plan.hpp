// rpset_plan.hpp — the index arithmetic of the set commitments (csrc/rpset.hip, include/bppp.h: "set commitments"): which nodes a Merkle mountain
// range of n rows has, which of them an append of m rows creates, where a leaf's path lies and how the level arrays grow.  No HIP and no hashing:
// the kernels of csrc/rpset.hip.h and the host code of csrc/rpset.hip call the functions below, and tests/native/set_plan_check.cpp replays them
// without a GPU.
//   node (k, j)   covers leaves [j 2^k, (j + 1) 2^k); it exists once (j + 1) 2^k <= n, i.e. j < n >> k
//   peaks of n    for every set bit k of n, from the highest down: node (k, (n >> k) - 1); P_0 .. P_{m-1}
//   an append of m rows onto n creates node (k, j) exactly when j is in [n >> k, (n + m) >> k)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__)
#define BPPP_SET_HD __host__ __device__ inline
#else
#define BPPP_SET_HD inline
#endif

namespace bppp_set {

static constexpr uint32_t TILE_BITS = 8, TILE = 1u << TILE_BITS;     // levels fused by one launch of the tree kernel; nodes of a tile's bottom level
static constexpr uint32_t MAX_ROW_BYTES = 8192;
static constexpr uint32_t FULL_LEVELS = 31;                          // a full store holds n < 2^31 rows: levels 0 .. 30
static constexpr uint32_t MAX_LEVELS = 64;                           // a frontier holds n < 2^63: slots 0 .. 62, the array is 64 wide
static constexpr uint64_t FULL_MAX_N = ((uint64_t)1 << 31) - 1, FRONTIER_MAX_N = ((uint64_t)1 << 63) - 1;

BPPP_SET_HD uint64_t shr(uint64_t x, uint32_t s) { return s >= 64 ? 0 : x >> s; }
BPPP_SET_HD uint32_t bit_length(uint64_t n) { return n ? 64u - (uint32_t)__builtin_clzll((unsigned long long)n) : 0u; }
BPPP_SET_HD uint32_t popcount(uint64_t n) { return (uint32_t)__builtin_popcountll((unsigned long long)n); }
BPPP_SET_HD bool has_peak(uint64_t n, uint32_t k) { return k < 64 && ((n >> k) & 1); }
BPPP_SET_HD uint64_t peak_index(uint64_t n, uint32_t k) { return (n >> k) - 1; }                  // of a level k with has_peak (n, k)
// node (k, j) is created by the append that takes the set from n to N rows
BPPP_SET_HD bool is_new(uint64_t n, uint64_t N, uint32_t k, uint64_t j) { return j >= shr(n, k) && j < shr(N, k); }
// the append from n to N makes a new peak at level k (else a peak of N at that level is the peak n had there)
BPPP_SET_HD bool peak_is_new(uint64_t n, uint64_t N, uint32_t k) { return has_peak(N, k) && shr(N, k) > shr(n, k); }
// compressions of a leaf: the message Dl || row with its padding
BPPP_SET_HD uint32_t leaf_blocks(uint32_t row_bytes) { return (32 + row_bytes + 9 + 63) / 64; }
BPPP_SET_HD size_t path_bytes(uint64_t n) { return (size_t)32 * bit_length(n); }

// where leaf i of n rows (i < n) stands: its peak P_p of height h, the peaks m of n, and the hashes its path uses
struct Locate { uint32_t h, p, m, used; };
BPPP_SET_HD Locate locate(uint64_t n, uint64_t i) {
  // i < n: at the highest bit where they differ n has a one, and the peaks above it are full of leaves below i
  Locate L{bit_length(i ^ n) - 1, 0, popcount(n), 0};
  L.p = popcount(shr(n, L.h + 1));
  L.used = L.h + (L.p + 1 < L.m ? 1u : 0u) + L.p;
  return L;
}
// the level of peak P_p of n (p < popcount (n))
BPPP_SET_HD uint32_t peak_level(uint64_t n, uint32_t p) {
  for (int k = 63; k >= 0; k--) if ((n >> k) & 1) { if (!p) return (uint32_t)k; p--; }
  return 0;
}
// what slot s of the path of leaf i holds
enum SlotKind : uint32_t { SLOT_SIBLING = 0, SLOT_RIGHT_BAG = 1, SLOT_PEAK = 2, SLOT_ZERO = 3 };
struct Slot { uint32_t kind, level; uint64_t index; uint32_t peak; };      // SIBLING: node (level, index); RIGHT_BAG: the bag of P_peak ..; PEAK: P_peak
BPPP_SET_HD Slot path_slot(uint64_t n, uint64_t i, const Locate &L, uint32_t s) {
  Slot S{SLOT_ZERO, 0, 0, 0};
  if (s < L.h) { S.kind = SLOT_SIBLING; S.level = s; S.index = (i >> s) ^ 1; return S; }
  uint32_t r = s - L.h;
  if (L.p + 1 < L.m) { if (!r) { S.kind = SLOT_RIGHT_BAG; S.peak = L.p + 1; return S; } r--; }
  if (r < L.p) { S.kind = SLOT_PEAK; S.peak = L.p - 1 - r; S.level = peak_level(n, S.peak); S.index = peak_index(n, S.level); }
  return S;
}

// ---- an append of m >= 1 rows onto n: one launch of the tree kernel per pass.  Pass q fuses the levels 8q + 1 .. 8q + 8 over the tiles of level 8q
// that hold a new node; it runs iff level 8q has a new node, so an append costs 1 (leaves) + passes launches, passes <= ceil (bit_length (n + m) / 8)
struct Pass { uint32_t L; uint64_t tile0, tiles; };
inline std::vector<Pass> append_passes(uint64_t n, uint64_t m) {
  std::vector<Pass> out;
  const uint64_t N = n + m;
  for (uint32_t L = 0; L < 64; L += TILE_BITS) {
    const uint64_t a = n >> L, b = N >> L;
    if (b <= a) break;
    out.push_back(Pass{L, a >> TILE_BITS, ((b - 1) >> TILE_BITS) - (a >> TILE_BITS) + 1});
  }
  return out;
}
// frontier-only: the tops of pass q (the new nodes of level 8 (q + 1), at most (m >> 8 (q + 1)) + 1) go to scratch buffer q & 1, which the next pass reads;
// the nodes each of the two buffers holds
inline uint64_t tops_nodes(uint64_t m, uint32_t which) { return (m >> (TILE_BITS * (which + 1))) + 2; }
// the nodes of level k a set of n rows has, and the grow-only capacity of its level array: at least `need`, at least twice what it was
inline uint64_t level_nodes(uint64_t n, uint32_t k) { return shr(n, k); }
inline uint64_t grow(uint64_t cap, uint64_t need) {
  if (need <= cap) return cap;
  uint64_t c = cap * 2 > need ? cap * 2 : need;
  return c < 64 ? 64 : c;
}

// ---- the level arrays of a full store and their growth, all or nothing.  The kernels reach the arrays through a table of their addresses in HBM, so the
// arrays, their capacities and that table have to change together.  grow_levels makes the store hold N rows where it holds n:
//   1. every array that must grow is allocated; if one allocation fails, the new ones are freed and nothing else has happened;
//   2. what the old arrays hold is copied; if a copy fails, the same;
//   3. the table of the new addresses is published; if that fails, the old table is published again and the new arrays are freed;
//   4. only now the old arrays are freed and the store takes the new ones.
// So a failure at any step leaves the store, and the table the kernels see, as they were.  Between steps 1 and 4 an array that grows is alive
// twice: its old capacity (below `need`) beside its new one (below 2 `need`), transiently up to three times the level's nodes.
// Ops (csrc/rpset.hip: HIP; tests/native/set_plan_check.cpp: a stub that fails on demand):
//   void *alloc (size_t bytes)  nullptr on failure;  void release (void *);  bool copy (void *dst, const void *src, size_t bytes);
//   bool publish (uint32_t *const table[32])
static constexpr uint32_t LEVEL_SLOTS = 32;
struct LevelStore { uint32_t *lvl[LEVEL_SLOTS] = {}; uint64_t cap[LEVEL_SLOTS] = {}; };
enum GrowResult { GROW_OK = 0, GROW_ALLOC_FAILED = 1, GROW_COPY_FAILED = 2, GROW_PUBLISH_FAILED = 3 };
template <class Ops> GrowResult grow_levels(LevelStore &S, uint64_t n, uint64_t N, Ops &ops) {
  uint32_t *fresh[LEVEL_SLOTS] = {};
  uint64_t fresh_cap[LEVEL_SLOTS] = {};
  bool any = false;
  auto undo = [&]() { for (uint32_t k = 0; k < LEVEL_SLOTS; k++) if (fresh[k]) ops.release(fresh[k]); };
  for (uint32_t k = 0; k < FULL_LEVELS; k++) {
    const uint64_t need = level_nodes(N, k);
    if (need <= S.cap[k]) continue;
    fresh_cap[k] = grow(S.cap[k], need);
    fresh[k] = (uint32_t *)ops.alloc((size_t)fresh_cap[k] * 32);
    if (!fresh[k]) { undo(); return GROW_ALLOC_FAILED; }
    any = true;
  }
  if (!any) return GROW_OK;
  for (uint32_t k = 0; k < FULL_LEVELS; k++) {
    const uint64_t have = level_nodes(n, k);
    if (fresh[k] && have && !ops.copy(fresh[k], S.lvl[k], (size_t)have * 32)) { undo(); return GROW_COPY_FAILED; }
  }
  uint32_t *table[LEVEL_SLOTS];
  for (uint32_t k = 0; k < LEVEL_SLOTS; k++) table[k] = fresh[k] ? fresh[k] : S.lvl[k];
  if (!ops.publish(table)) { ops.publish(S.lvl); undo(); return GROW_PUBLISH_FAILED; }
  for (uint32_t k = 0; k < LEVEL_SLOTS; k++) {
    if (!fresh[k]) continue;
    if (S.lvl[k]) ops.release(S.lvl[k]);
    S.lvl[k] = fresh[k]; S.cap[k] = fresh_cap[k];
  }
  return GROW_OK;
}

}  // namespace bppp_set
