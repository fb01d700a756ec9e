// rpscan_keys_plan.hpp — the host's share of the many-key scan (bppp_rp_scan_keys, csrc/rpscan_keys.hip): the recoding of a view secret for the
// multi-key walk, the geometry of the passes, and the merge of a pass's hits into the call's (row, key) order.  Plain C++, no HIP: the test
// library calls it and tests/native/scan_keys_check.cpp replays it under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "hosteis.hpp"

namespace bppp {

// ---- the recoded key: a mod n = a1 + a2 lambda (decompose_eis, as scan_recode of csrc/rpseal.hip.h splits it), each half as a width-4 signed sliding window (wNAF: digits 0, +-1, +-3, +-5, +-7, no two non-zero
// digits within four places), the half's sign folded into its digits.  Position i holds a byte at bits 8 (i & 3) .. of d[i >> 2]: the low nibble
// is the digit of a1, the high one of a2; a nibble is 0 for the digit 0, else (|digit| + 1) / 2 in its low three bits and 8 for a negative digit.
// nbits positions, walked from nbits - 1 down; 132 positions hold every split (a 129-bit magnitude has at most 130 digits).
static constexpr uint32_t SCAN_KEY_DIGIT_WORDS = 33, SCAN_KEY_WORDS = 36;
struct ScanKeyRec { uint32_t d[SCAN_KEY_DIGIT_WORDS]; uint32_t nbits; uint32_t zero[SCAN_KEY_WORDS - SCAN_KEY_DIGIT_WORDS - 1]; };
static_assert(sizeof(ScanKeyRec) == 4 * SCAN_KEY_WORDS, "a key record is 36 words");
// the wNAF of the magnitude m (three limbs), negated if neg: digits from position 0 up; returns their number (at most 4 * SCAN_KEY_DIGIT_WORDS)
inline int scan_keys_wnaf4(const uint64_t m[3], bool neg, int8_t *out) {
  uint64_t k[3] = {m[0], m[1], m[2]};
  int n = 0;
  while (k[0] | k[1] | k[2]) {
    int d = 0;
    if (k[0] & 1) {
      d = (int)(k[0] & 15);
      if (d > 8) d -= 16;
      if (d > 0) { const uint64_t o = k[0]; k[0] -= (uint64_t)d; if (k[0] > o) { if (k[1]-- == 0) k[2]--; } }
      else { const uint64_t o = k[0]; k[0] += (uint64_t)(-d); if (k[0] < o) { if (++k[1] == 0) k[2]++; } }
    }
    out[n++] = (int8_t)(neg ? -d : d);
    k[0] = (k[0] >> 1) | (k[1] << 63); k[1] = (k[1] >> 1) | (k[2] << 63); k[2] >>= 1;
  }
  return n;
}
inline bool scan_keys_recode(const uint64_t scalar[4], ScanKeyRec &W) {
  using namespace bppp_host;
  U256 x = U256::load(scalar), t;
  if (!sub_raw(t, x, FR().m)) x = t;
  const bppp_eis::Eis e = bppp_eis::decompose_eis(x);
  memset(&W, 0, sizeof W);
  if (std::max(e.a.bits(), e.b.bits()) > 130) return false;
  int8_t d1[4 * SCAN_KEY_DIGIT_WORDS + 4] = {0}, d2[4 * SCAN_KEY_DIGIT_WORDS + 4] = {0};
  const int n = std::max(scan_keys_wnaf4(e.a.m, e.a.neg, d1), scan_keys_wnaf4(e.b.m, e.b.neg, d2));
  W.nbits = (uint32_t)n;
  auto nib = [](int d) -> uint32_t { return d == 0 ? 0u : (uint32_t)(((d < 0 ? -d : d) + 1) / 2) | (d < 0 ? 8u : 0u); };
  for (int i = 0; i < n; i++) W.d[i >> 2] |= (nib(d1[i]) | (nib(d2[i]) << 4)) << (8 * (i & 3));
  return true;
}

// ---- the geometry of a call.  Rows are the outer loop (a pass: its seals lifted and its tables made once for every key), tiles of kt keys the
// inner one (one walk launch a tile), and a tile's survivors are opened open_chunk at a time.  All three come from the handle's flat chunk F
// (items of one pass over the workspace, csrc/rp_internal.hpp) and nranges: a pass holds at most F / nranges / 16 rows and a tile at most
// F / nranges (row, key) pairs, so the accumulators of a tile are bounded as the one-key scan's workspace is.
static constexpr size_t SCAN_KEYS_TILE_MAX = 16, SCAN_KEYS_ROW_SHARE = 16;
struct ScanKeysGeom { size_t rows_pass, kt, open_chunk; };
inline ScanKeysGeom scan_keys_geometry(size_t flat_chunk, size_t nr, size_t rows, size_t nkeys) {
  const size_t per = std::max<size_t>(1, flat_chunk / std::max<size_t>(1, nr));
  ScanKeysGeom g;
  g.rows_pass = std::max<size_t>(1, std::min(rows, per / SCAN_KEYS_ROW_SHARE));
  g.kt = std::max<size_t>(1, std::min({nkeys, SCAN_KEYS_TILE_MAX, per / g.rows_pass}));
  g.open_chunk = g.rows_pass;
  return g;
}
// the 32-bit words of every array carved for that geometry.  tab: the walk's tables, word-major in blocks of 64 lanes (tab_words a lane);
// acc, P, surv_*, ss, verdict hold a whole tile — every pair may survive —; in_sc, flag, dec, rec one open chunk.
struct ScanKeysCarve { size_t R, status, tab, keys, acc, P, count, surv_row, surv_key, ss, in_sc, flag, dec, rec, verdict; };
inline ScanKeysCarve scan_keys_carve(const ScanKeysGeom &g, size_t nr, size_t tab_words, size_t acc_words, size_t key_words = SCAN_KEY_WORDS) {
  const size_t C = g.rows_pass, pairs = C * g.kt, S = g.open_chunk;
  ScanKeysCarve c;
  c.R = C * 16; c.status = C; c.tab = (C + 63) / 64 * 64 * tab_words; c.keys = g.kt * key_words; c.acc = pairs * acc_words; c.P = pairs * 16; c.count = 4;
  c.surv_row = pairs; c.surv_key = pairs; c.ss = pairs * 8; c.verdict = pairs;
  c.in_sc = S * nr * 24; c.flag = S * nr; c.dec = S * nr * 16; c.rec = S * nr * 16;
  return c;
}

// ---- hits.  A pass's owned (row, key) pairs arrive tile by tile in no order; the call lists them by (row, key) ascending, and rows only grow
// from pass to pass, so sorting each pass and appending is the call's order.  merge_pass appends the pass's hits to the lists while slots are
// left (cap), counts every one of them in nhits, and returns in `pass` the sorted hits with those past the cap cut off: hit j of what is left
// belongs in slot first_slot + j, and its opening is made from its ss.
struct ScanHit { uint32_t row, key; uint32_t ss[8]; };
inline size_t scan_keys_merge_pass(std::vector<ScanHit> &pass, size_t cap, size_t &nhits, uint32_t *hit_key, uint32_t *hit_row) {
  std::sort(pass.begin(), pass.end(), [](const ScanHit &a, const ScanHit &b) { return a.row != b.row ? a.row < b.row : a.key < b.key; });
  const size_t first_slot = std::min(nhits, cap), keep = std::min(pass.size(), cap - first_slot);
  for (size_t j = 0; j < keep; j++) { hit_row[first_slot + j] = pass[j].row; hit_key[first_slot + j] = pass[j].key; }
  nhits += pass.size();
  pass.resize(keep);
  return first_slot;
}

}  // namespace bppp
