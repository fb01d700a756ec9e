// rptally_plan.hpp — the host's plan of a tally (csrc/rptally.hip): which sums one pass over the workspace holds, and the workgroup items
// that sum the long ones, level by level.  Plain C++ over a VALIDATED sum_start (non-decreasing from 0), so that a native check
// (tests/native/tally_plan_check.cpp) can replay a plan without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace bppp_tally {

static constexpr uint32_t FINAL = 0x80000000u;     // an item's destination: bit 31 = the sum itself, else a partial point

// one workgroup's work: sources [x, y) — entries at level 0, partial points of the level before later — summed into destination z (sum
// `z & ~FINAL` of the pass when FINAL is set, else partial point z of this level's buffer); w: the sum of the pass it belongs to.
// Laid out as the kernel's uint4.
struct Item { uint32_t x, y, z, w; };

// the first sum of every pass, then nsums: a pass holds at most E sums and, unless it is one sum alone, at most E entries
inline std::vector<size_t> chunk_bounds(const uint32_t *start, size_t nsums, size_t E) {
  E = std::max<size_t>(1, E);
  std::vector<size_t> b{0};
  size_t t0 = 0;
  for (size_t t = 0; t < nsums; t++)
    if (t > t0 && (t - t0 >= E || (size_t)start[t + 1] - start[t0] > E)) { b.push_back(t); t0 = t; }
  b.push_back(nsums);
  return b;
}

// the items of the sums of [t0, t1) that are longer than smax (the others are one lane's work), in pieces of at most P >= 2 sources:
// level k reads entries (k = 0) or buffer (k - 1) & 1 and writes buffer k & 1; npart[b]: the points buffer b must hold
struct Levels { std::vector<std::vector<Item>> lv; size_t npart[2] = {0, 0}, nitems = 0; };
inline Levels plan_levels(const uint32_t *start, size_t t0, size_t t1, uint32_t smax, uint32_t P) {
  P = std::max<uint32_t>(2, P);
  struct Range { uint32_t b, e, slot; };
  Levels L;
  std::vector<Range> cur;
  for (size_t t = t0; t < t1; t++) if (start[t + 1] - start[t] > smax) cur.push_back({start[t], start[t + 1], (uint32_t)(t - t0)});
  for (int k = 0; !cur.empty(); k++) {
    std::vector<Item> items;
    std::vector<Range> next;
    uint32_t np = 0;
    for (const Range &r : cur) {
      if (r.e - r.b <= P) { items.push_back({r.b, r.e, FINAL | r.slot, r.slot}); continue; }
      const uint32_t first = np;
      for (uint32_t b = r.b; b < r.e; b += std::min(P, r.e - b)) items.push_back({b, b + std::min(P, r.e - b), np++, r.slot});
      next.push_back({first, np, r.slot});
    }
    L.npart[k & 1] = std::max<size_t>(L.npart[k & 1], np);
    L.nitems += items.size();
    L.lv.push_back(std::move(items));
    cur.swap(next);
  }
  return L;
}

}  // namespace bppp_tally
