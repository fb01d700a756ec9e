// scan_keys_check.cpp — the host's share of the many-key scan (csrc/rpscan_keys_plan.hpp) replayed without a GPU, over seeded random jobs:
//   geometry   the passes, tiles and open chunks are walked as csrc/rpscan_keys.hip walks them: every (row, key) pair is visited exactly once, and
//              the highest index each kernel touches — in the worst case, every pair a survivor — is written into vectors of exactly the carved
//              sizes, within the budgets the header states (rows a pass, pairs a tile)
//   merge      hits arrive tile by tile in shuffled order; the merged lists equal a sorted reference cut at cap, for cap below, at and above
//              the hit count, and the slots each pass reports are the ones its kept hits occupy
//   recoding   the two halves put together again from their signed window digits, by additions and doublings mod n alone, give the scalar mod n,
//              and the digits are a width-4 wNAF
// Built with the address and undefined-behaviour sanitizers by tests/test_scan_keys_plan_host.py, so an index past a carved array fails too.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <random>
#include <vector>
#include "rpscan_keys_plan.hpp"

using namespace bppp;
using bppp_host::U256;

#define REQUIRE(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static const size_t TAB_WORDS = 64, ACC_WORDS = 40;

static int replay_geometry(size_t flat, size_t nr, size_t rows, size_t nkeys) {
  const ScanKeysGeom G = scan_keys_geometry(flat, nr, rows, nkeys);
  const size_t per = std::max<size_t>(1, flat / nr);
  REQUIRE(G.rows_pass >= 1 && G.kt >= 1 && G.open_chunk >= 1);
  REQUIRE(G.rows_pass <= std::max<size_t>(1, per / SCAN_KEYS_ROW_SHARE) && G.rows_pass <= std::max<size_t>(1, rows));
  REQUIRE(G.kt <= SCAN_KEYS_TILE_MAX && G.kt <= nkeys && G.rows_pass * G.kt <= std::max(per, G.rows_pass));
  REQUIRE(G.open_chunk * nr <= std::max(per, nr));
  const ScanKeysCarve Z = scan_keys_carve(G, nr, TAB_WORDS, ACC_WORDS);
  std::vector<uint32_t> R(Z.R), status(Z.status), tab(Z.tab), keys(Z.keys), acc(Z.acc), P(Z.P), count(Z.count), surv_row(Z.surv_row), surv_key(Z.surv_key), ss(Z.ss), in_sc(Z.in_sc),
      flag(Z.flag), dec(Z.dec), rec(Z.rec), verdict(Z.verdict);
  std::vector<uint8_t> visited(rows * nkeys, 0);
  for (size_t o = 0; o < rows; o += G.rows_pass) {
    const size_t n = std::min(G.rows_pass, rows - o), blocks = (n + 63) / 64;
    R[(n - 1) * 16 + 15] = 1; status[n - 1] = 1;
    tab[(blocks - 1) * TAB_WORDS * 64 + (TAB_WORDS - 1) * 64 + 63] = 1;       // the last lane's column of the last block, were the block full
    for (size_t k0 = 0; k0 < nkeys; k0 += G.kt) {
      const size_t kt = std::min(G.kt, nkeys - k0), pairs = n * kt;
      keys[(kt - 1) * SCAN_KEY_WORDS + SCAN_KEY_WORDS - 1] = 1;
      acc[((kt - 1) * n + n - 1) * ACC_WORDS + ACC_WORDS - 1] = 1;
      P[((kt - 1) * n + n - 1) * 16 + 15] = 1;
      count[0] = (uint32_t)pairs;
      for (size_t b = 0; b < n; b++) for (size_t k = 0; k < kt; k++) visited[(o + b) * nkeys + k0 + k]++;
      // every pair survives
      surv_row[pairs - 1] = 1; surv_key[pairs - 1] = 1; ss[(pairs - 1) * 8 + 7] = 1;
      size_t judged = 0;
      for (size_t c0 = 0; c0 < pairs; c0 += G.open_chunk) {
        const size_t c = std::min(G.open_chunk, pairs - c0), m = c * nr;
        in_sc[(m - 1) * 24 + 23] = 1; flag[m - 1] = 1; dec[(m - 1) * 16 + 15] = 1; rec[(m - 1) * 16 + 15] = 1;
        REQUIRE(ss.size() >= (c0 + c) * 8 && surv_row.size() >= c0 + c);
        verdict[c0 + c - 1] = 1;
        judged += c;
      }
      REQUIRE(judged == pairs);
    }
  }
  for (size_t i = 0; i < visited.size(); i++) REQUIRE(visited[i] == 1);
  return 0;
}

static int replay_merge(std::mt19937_64 &rng, size_t rows, size_t nkeys, size_t rows_pass, size_t kt, double density, int cap_mode) {
  std::vector<std::pair<uint32_t, uint32_t>> all;           // (row, key), the reference
  std::vector<uint8_t> own(rows * nkeys);
  for (auto &x : own) x = (rng() % 1000) < density * 1000;
  for (size_t i = 0; i < rows; i++) for (size_t k = 0; k < nkeys; k++) if (own[i * nkeys + k]) all.push_back({(uint32_t)i, (uint32_t)k});
  const size_t total = all.size();
  const size_t cap = cap_mode == 0 ? 0 : cap_mode == 1 ? total / 2 : cap_mode == 2 ? (total ? total - 1 : 0) : cap_mode == 3 ? total : total + 3;
  std::vector<uint32_t> hit_key(cap, 0xA5A5A5A5u), hit_row(cap, 0xA5A5A5A5u), slot_ss(cap, 0);
  size_t nhits = 0;
  for (size_t o = 0; o < rows; o += rows_pass) {
    const size_t n = std::min(rows_pass, rows - o);
    std::vector<ScanHit> pass;
    for (size_t k0 = 0; k0 < nkeys; k0 += kt) {
      std::vector<ScanHit> tile;
      for (size_t b = 0; b < n; b++)
        for (size_t k = k0; k < std::min(nkeys, k0 + kt); k++)
          if (own[(o + b) * nkeys + k]) { ScanHit h; h.row = (uint32_t)(o + b); h.key = (uint32_t)k; for (int w = 0; w < 8; w++) h.ss[w] = (uint32_t)(h.row * 131 + h.key * 7 + w); tile.push_back(h); }
      std::shuffle(tile.begin(), tile.end(), rng);         // survivor order is free
      pass.insert(pass.end(), tile.begin(), tile.end());
    }
    const size_t before = nhits, arrived = pass.size();
    const size_t first = scan_keys_merge_pass(pass, cap, nhits, cap ? hit_key.data() : nullptr, cap ? hit_row.data() : nullptr);
    REQUIRE(nhits == before + arrived && first == std::min(before, cap) && pass.size() == std::min(arrived, cap - first));
    for (size_t j = 0; j < pass.size(); j++) {
      REQUIRE(first + j < cap && hit_row[first + j] == pass[j].row && hit_key[first + j] == pass[j].key);
      slot_ss[first + j] = pass[j].ss[0];
    }
  }
  REQUIRE(nhits == total);
  for (size_t h = 0; h < cap; h++) {
    if (h < total) REQUIRE(hit_row[h] == all[h].first && hit_key[h] == all[h].second && slot_ss[h] == all[h].first * 131 + all[h].second * 7);
    else REQUIRE(hit_row[h] == 0xA5A5A5A5u && hit_key[h] == 0xA5A5A5A5u);      // the tail is the caller's to zero: the merge leaves it alone
  }
  return 0;
}

// (2 a) mod n and (a + b) mod n for a, b < n, by the raw additions alone
static U256 addmod(const U256 &a, const U256 &b) {
  U256 s, t;
  const uint64_t c = bppp_host::add_raw(s, a, b);
  if (c || bppp_host::cmp(s, bppp_host::FR().m) >= 0) { bppp_host::sub_raw(t, s, bppp_host::FR().m); return t; }
  return s;
}
static int replay_recode(const uint64_t x[4]) {
  static const uint64_t LAMBDA[4] = {0xDF02967C1B23BD72ULL, 0x122E22EA20816678ULL, 0xA5261C028812645AULL, 0x5363AD4CC05C30E0ULL};
  ScanKeyRec W;
  REQUIRE(scan_keys_recode(x, W));
  REQUIRE(W.nbits <= 4 * SCAN_KEY_DIGIT_WORDS);
  for (uint32_t i = 0; i < SCAN_KEY_WORDS - SCAN_KEY_DIGIT_WORDS - 1; i++) REQUIRE(W.zero[i] == 0);
  auto byte_at = [&](uint32_t i) { return (W.d[i >> 2] >> (8 * (i & 3))) & 0xFFu; };
  for (uint32_t i = W.nbits; i < 4 * SCAN_KEY_DIGIT_WORDS; i++) REQUIRE(byte_at(i) == 0);
  if (W.nbits) REQUIRE(byte_at(W.nbits - 1) != 0);
  // a1 mod n and a2 lambda mod n, position by position from the highest down: h += digit * unit, by additions of the unit alone
  const U256 one = U256::one(), lam = U256::load(LAMBDA);
  U256 h1 = U256::zero(), h2 = U256::zero(), t;
  int last[2] = {-100, -100};
  for (int i = (int)W.nbits - 1; i >= 0; i--) {
    h1 = addmod(h1, h1); h2 = addmod(h2, h2);
    for (int half = 0; half < 2; half++) {
      const uint32_t nb = (byte_at((uint32_t)i) >> (4 * half)) & 15u;
      if (!nb) continue;
      const uint32_t mag = 2 * (nb & 7u) - 1;
      REQUIRE((nb & 7u) >= 1 && (nb & 7u) <= 4);                    // odd digits of magnitude at most 7
      REQUIRE(last[half] == -100 || last[half] - i >= 4);          // no two non-zero digits within four places
      last[half] = i;
      U256 unit = half ? lam : one;
      if (nb & 8u) { bppp_host::sub_raw(t, bppp_host::FR().m, unit); unit = t; }
      U256 &h = half ? h2 : h1;
      for (uint32_t r = 0; r < mag; r++) h = addmod(h, unit);
    }
  }
  U256 want = U256::load(x);
  if (!bppp_host::sub_raw(t, want, bppp_host::FR().m)) want = t;
  REQUIRE(addmod(h1, h2) == want);
  return 0;
}

int main() {
  std::mt19937_64 rng(20261020);
  // geometry: the defaults on a few shapes, then small random jobs under small flat chunks
  const size_t fixed[][4] = {{(size_t)1 << 22, 1, 1, 1}, {(size_t)1 << 22, 1, 300, 40}, {(size_t)1 << 22, 3, 257, 33}, {3 * 16 * 64, 3, 257, 33}, {1, 3, 5, 3}, {48, 3, 65, 17}};
  for (const auto &f : fixed) if (replay_geometry(f[0], f[1], f[2], f[3])) return 1;
  for (int it = 0; it < 400; it++) {
    const size_t nr = 1 + rng() % 4, flat = 1 + rng() % (nr * 16 * 40), rows = 1 + rng() % 300, nkeys = 1 + rng() % 40;
    if (replay_geometry(flat, nr, rows, nkeys)) { printf("geometry job: flat %zu nr %zu rows %zu keys %zu\n", flat, nr, rows, nkeys); return 1; }
  }
  {                                                          // the shapes the GPU tests rely on
    const ScanKeysGeom d = scan_keys_geometry((size_t)1 << 22, 3, 257, (size_t)1 << 20), s = scan_keys_geometry(3 * 16 * 64, 3, 257, 33);
    REQUIRE(d.rows_pass == 257 && d.kt == SCAN_KEYS_TILE_MAX && s.rows_pass == 64 && s.kt == 16 && s.open_chunk == 64);
  }
  for (int it = 0; it < 300; it++) {
    const size_t rows = 1 + rng() % 120, nkeys = 1 + rng() % 20, rows_pass = 1 + rng() % 40, kt = 1 + rng() % 8;
    const double density = (it % 3 == 0) ? 1.0 : (it % 3 == 1) ? 0.3 : 0.02;
    if (replay_merge(rng, rows, nkeys, rows_pass, kt, density, it % 5)) { printf("merge job %d\n", it); return 1; }
  }
  const uint64_t named[][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, 0, 0, 0}, {~0ULL, ~0ULL, ~0ULL, ~0ULL}, {0, 0, 0, 1ULL << 63},
                               {0xBFD25E8CD0364141ULL, 0xBAAEDCE6AF48A03BULL, 0xFFFFFFFFFFFFFFFEULL, ~0ULL},      // n
                               {0xBFD25E8CD0364140ULL, 0xBAAEDCE6AF48A03BULL, 0xFFFFFFFFFFFFFFFEULL, ~0ULL},      // n - 1
                               {0xBFD25E8CD0364142ULL, 0xBAAEDCE6AF48A03BULL, 0xFFFFFFFFFFFFFFFEULL, ~0ULL},      // n + 1
                               {0xDF02967C1B23BD72ULL, 0x122E22EA20816678ULL, 0xA5261C028812645AULL, 0x5363AD4CC05C30E0ULL}};   // lambda
  for (const auto &x : named) if (replay_recode(x)) return 1;
  for (int it = 0; it < 2000; it++) {
    const uint64_t x[4] = {rng(), rng(), rng(), rng()};
    if (replay_recode(x)) { printf("scalar %016llx%016llx%016llx%016llx\n", (unsigned long long)x[3], (unsigned long long)x[2], (unsigned long long)x[1], (unsigned long long)x[0]); return 1; }
  }
  printf("replays ok\n");
  return 0;
}
