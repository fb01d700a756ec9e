// tally_plan_check.cpp — the host's plan of a tally (csrc/rptally_plan.hpp) replayed without a GPU: over random CSR jobs and thresholds,
// every pass and every level is executed on 64-bit integers in place of points (lane route for the short sums, items for the long ones,
// two partial buffers of exactly the planned sizes) and must leave in every sum's slot, written exactly once, the signed sum of its
// entries.  Built with the sanitizers by tests/test_tally_plan_host.py, so an index past a planned buffer is a failure too.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>
#include "rptally_plan.hpp"

using namespace bppp_tally;

#define REQUIRE(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int replay(const std::vector<uint32_t> &start, const std::vector<uint32_t> &entries, const std::vector<uint64_t> &val, uint32_t smax, uint32_t P, size_t E) {
  const size_t nsums = start.size() - 1;
  const std::vector<size_t> cb = chunk_bounds(start.data(), nsums, E);
  REQUIRE(cb.front() == 0 && cb.back() == nsums);
  auto term = [&](uint32_t e) { const uint64_t v = val[e & ~FINAL]; return (e >> 31) ? (uint64_t)0 - v : v; };
  size_t seen = 0;
  for (size_t c = 0; c + 1 < cb.size(); c++) {
    const size_t t0 = cb[c], t1 = cb[c + 1], ns = t1 - t0;
    REQUIRE(ns >= 1 && ns <= std::max<size_t>(1, E) && t0 == seen);
    REQUIRE(ns == 1 || (size_t)start[t1] - start[t0] <= std::max<size_t>(1, E));
    seen = t1;
    std::vector<uint64_t> sums(ns, 0);
    std::vector<int> written(ns, 0);
    for (size_t t = 0; t < ns; t++) {                      // route 0
      const uint32_t b = start[t0 + t], e = start[t0 + t + 1];
      if (e - b > smax) continue;
      for (uint32_t p = b; p < e; p++) sums[t] += term(entries[p]);
      written[t]++;
    }
    const Levels L = plan_levels(start.data(), t0, t1, smax, P);
    std::vector<uint64_t> part[2] = {std::vector<uint64_t>(L.npart[0]), std::vector<uint64_t>(L.npart[1])};
    size_t nitems = 0;
    for (size_t k = 0; k < L.lv.size(); k++) {
      REQUIRE(!L.lv[k].empty());
      std::vector<int> dst_written(part[k & 1].size(), 0);
      for (const Item &it : L.lv[k]) {
        REQUIRE(it.x < it.y && it.y - it.x <= std::max<uint32_t>(2, P) && it.w < ns);
        uint64_t acc = 0;
        for (uint32_t p = it.x; p < it.y; p++) acc += k ? part[(k + 1) & 1].at(p) : term(entries.at(p));
        if (it.z & FINAL) { REQUIRE((it.z & ~FINAL) == it.w); sums.at(it.w) = acc; written.at(it.w)++; }
        else { part[k & 1].at(it.z) = acc; dst_written.at(it.z)++; }
      }
      nitems += L.lv[k].size();
    }
    REQUIRE(nitems == L.nitems);
    for (size_t t = 0; t < ns; t++) {
      uint64_t want = 0;
      for (uint32_t p = start[t0 + t]; p < start[t0 + t + 1]; p++) want += term(entries[p]);
      REQUIRE(written[t] == 1 && sums[t] == want);
    }
  }
  return 0;
}

int main() {
  std::mt19937_64 rng(20260101);
  int jobs = 0;
  for (int round = 0; round < 100; round++) {
    const size_t nsums = 1 + rng() % 40, total = 1 + rng() % 50;
    std::vector<uint32_t> start{0}, entries;
    for (size_t t = 0; t < nsums; t++) {
      const unsigned kind = rng() % 8;
      const size_t len = kind == 0 ? 0 : kind < 5 ? rng() % 6 : kind < 7 ? rng() % 40 : rng() % 700;
      for (size_t i = 0; i < len; i++) entries.push_back((uint32_t)(rng() % total) | ((rng() & 1) ? FINAL : 0u));
      start.push_back((uint32_t)entries.size());
    }
    std::vector<uint64_t> val(total);
    for (auto &v : val) v = rng();
    const uint32_t smaxs[] = {0, 1, 3, 16}, pieces[] = {2, 3, 5, 64, 4096};
    const size_t passes[] = {1, 2, 7, 100, (size_t)1 << 22};
    for (uint32_t smax : smaxs) for (uint32_t P : pieces) for (size_t E : passes) { if (replay(start, entries, val, smax, P, E)) return 1; jobs++; }
  }
  printf("%d replays ok\n", jobs);
  return 0;
}
