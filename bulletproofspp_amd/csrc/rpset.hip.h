// rpset.hip.h — the kernels of the set commitments (csrc/rpset.hip launches them; include/bppp.h states every message; csrc/rpset_plan.hpp has the
// index arithmetic, shared with the host).  A node is eight big-endian words, as sha256_compress leaves a digest; bytes are made at the outputs.
//   k_rp_set_leaf          one lane a row: SHA-256 (Dl || row) by a run-time loop of leaf_blocks (row_bytes) compressions over bytewise loads
//   k_rp_set_tree          a workgroup per aligned tile of 256 nodes of level L: the eight levels above through LDS; every new node goes to the store
//                          (or, on a frontier-only set, the tile's top to the next pass and a new peak to the frontier); an old left node comes from
//                          the store (or the frontier)
//   k_rp_set_front_merge   frontier-only: the new peaks over the old ones, after the passes that read the old ones
//   k_rp_set_bags          one lane: the peaks P_0 .., their right-bags bag (P_p ..) and the root; the peaks and the root as bytes where asked
//   k_rp_set_paths         one lane per (query, slot): 32 bytes of a path from the store, the right-bags or the peaks
//   k_rp_set_verify        one lane a query: the verdict of one path against a root
// Every kernel is bounds-checked on its own index, no loop bound comes from memory, stores are ordinary vector stores and there is no atomic.
#pragma once
#include "rpexcess_shared.hip.h"
#include "rpset_plan.hpp"

namespace bppp {
namespace set {

using bppp_set::TILE;
using bppp_set::TILE_BITS;

// the four domains of a set, by value in every launch
struct SetDomains { ExDomain leaf, node, bag, root; };
// where the nodes of a set live: a full store's level arrays (lvl[k][j][8], a table in HBM) or a frontier's slots (front[k][8], the peak of level k)
struct SetNodes { uint32_t *const *lvl; uint32_t *front; uint32_t keep; };

BPPP_DI const uint32_t *peak_ptr(const SetNodes &S, uint64_t n, uint32_t k) { return S.keep ? S.lvl[k] + bppp_set::peak_index(n, k) * 8 : S.front + k * 8; }

// st = SHA-256 (d || a || b): 96 bytes, the shape of a node and of a bag step
BPPP_DI void hash_pair(const ExDomain &d, const uint32_t *a, const uint32_t *b, uint32_t st[8]) {
  ex_digest<2>(96, [&](uint32_t k) -> uint32_t { return k < 32 ? ex_dom_byte(d, k) : k < 64 ? ex_word_byte(a, k - 32) : ex_word_byte(b, k - 64); }, st);
}
// st = SHA-256 (Dr || le64 (n) || le32 (row_bytes) || acc): 76 bytes
BPPP_DI void hash_root(const ExDomain &dr, uint64_t n, uint32_t row_bytes, const uint32_t *acc, uint32_t st[8]) {
  ex_digest<2>(32 + 8 + 4 + 32, [&](uint32_t k) -> uint32_t {
    if (k < 32) return ex_dom_byte(dr, k);
    if (k < 40) return (uint32_t)(n >> (8 * (k - 32)));
    if (k < 44) return row_bytes >> (8 * (k - 40));
    return ex_word_byte(acc, k - 44);
  }, st);
}
// st = SHA-256 (Dl || row): the block count is a run-time value, the words of a block are built with constant indices
BPPP_DI void hash_leaf(const ExDomain &dl, const uint8_t *__restrict__ row, uint32_t row_bytes, uint32_t st[8]) {
  const uint32_t nbytes = 32 + row_bytes, nblk = bppp_set::leaf_blocks(row_bytes);
  sha256_init(st);
  for (uint32_t blk = 0; blk < nblk; blk++) {
    uint32_t w[16];
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) {
      uint32_t word = 0;
#pragma unroll
      for (uint32_t r = 0; r < 4; r++) {
        const uint32_t k = 64 * blk + 4 * q + r;
        const uint32_t byte = k < 32 ? ex_dom_byte(dl, k) : k < nbytes ? (uint32_t)row[k - 32] : k == nbytes ? 0x80u : 0u;
        word = (word << 8) | byte;
      }
      w[q] = word;
    }
    if (blk == nblk - 1) w[15] = nbytes * 8;
    sha256_compress(st, w);
  }
}

// leaf i0 + t of the set: rows [m][row_bytes] -> out[t][8] (a full store: level 0 at row n + t; a frontier-only set: the scratch of the append)
__global__ void __launch_bounds__(64) k_rp_set_leaf(uint32_t m, uint32_t row_bytes, ExDomain dl, const uint8_t *__restrict__ rows, uint32_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  uint32_t st[8];
  hash_leaf(dl, rows + (size_t)t * row_bytes, row_bytes, st);
  for (int q = 0; q < 8; q++) out[(size_t)t * 8 + q] = st[q];
}

// One pass of an append from n to N rows over the levels L .. L + 8.  Workgroup g: tile tile0 + g, the nodes [tile 256, (tile + 1) 256) of level L and
// everything above them up to one node of level L + 8.  The tile is aligned, so its pairs are the pairs of the whole level.  Node j of level k is made
// exactly when bppp_set::is_new (n, N, k, j).  Its right child is then new too and sits in LDS; its left child is new (LDS) or is the peak n has at
// level k - 1 (the store, or the frontier).
//   a full store     level L is read from lvl[L], every new node of levels L + 1 .. L + 8 is written to its level array
//   frontier-only    level L is read from in[(j - in_base)][8] (the leaves, or the tops of the pass before), the tile's top goes to out[(j - out_base)][8],
//                    and a node that is a peak of N goes to front_new; `S.front` is only read, so no workgroup reads what another writes
// The loop count and every barrier are the same in all lanes.
struct TreePass { uint64_t n, N, tile0; uint32_t L; const uint32_t *in; uint64_t in_base; uint32_t *out; uint64_t out_base; uint32_t *front_new; };

BPPP_DI void front_put(const TreePass &A, uint32_t lev, uint64_t idx, const uint32_t *w) {
  if (bppp_set::has_peak(A.N, lev) && idx == bppp_set::peak_index(A.N, lev)) for (int q = 0; q < 8; q++) A.front_new[lev * 8 + q] = w[q];
}

__global__ void __launch_bounds__(TILE) k_rp_set_tree(TreePass A, SetNodes S, ExDomain dn) {
  __shared__ uint32_t lds[TILE * 8];
  const uint64_t tile = A.tile0 + blockIdx.x;
  const uint32_t j = threadIdx.x;
  {
    const uint64_t idx = (tile << TILE_BITS) + j;
    if (bppp_set::is_new(A.n, A.N, A.L, idx)) {
      const uint32_t *src = S.keep ? S.lvl[A.L] + idx * 8 : A.in + (idx - A.in_base) * 8;
      uint32_t w[8];
      for (int q = 0; q < 8; q++) w[q] = src[q];
      for (int q = 0; q < 8; q++) lds[j * 8 + q] = w[q];
      if (!S.keep && A.L == 0) front_put(A, A.L, idx, w);     // a leaf that is a peak; the bottom of a later pass was put by the pass before, as its top
    }
  }
  __syncthreads();
  for (uint32_t k = 1; k <= TILE_BITS; k++) {
    const uint32_t lev = A.L + k;
    if (bppp_set::shr(A.N, lev) <= bppp_set::shr(A.n, lev)) break;      // no new node at this level or above: the same in every lane
    const uint64_t idx = (tile << (TILE_BITS - k)) + j;
    const bool make = j < (TILE >> k) && bppp_set::is_new(A.n, A.N, lev, idx);
    uint32_t st[8];
    if (make) {
      uint32_t a[8], b[8];
      const uint64_t left = 2 * idx;
      if (left >= bppp_set::shr(A.n, lev - 1)) {
        for (int q = 0; q < 8; q++) a[q] = lds[2 * j * 8 + q];
      } else {                                                           // the peak n has at level lev - 1
        const uint32_t *old = S.keep ? S.lvl[lev - 1] + left * 8 : S.front + (lev - 1) * 8;
        for (int q = 0; q < 8; q++) a[q] = old[q];
      }
      for (int q = 0; q < 8; q++) b[q] = lds[(2 * j + 1) * 8 + q];
      hash_pair(dn, a, b, st);
    }
    __syncthreads();
    if (make) {
      for (int q = 0; q < 8; q++) lds[j * 8 + q] = st[q];
      if (S.keep) {
        uint32_t *dst = S.lvl[lev] + idx * 8;
        for (int q = 0; q < 8; q++) dst[q] = st[q];
      } else {
        front_put(A, lev, idx, st);
        if (k == TILE_BITS) for (int q = 0; q < 8; q++) A.out[(idx - A.out_base) * 8 + q] = st[q];
      }
    }
    __syncthreads();
  }
}

// front[k] = front_new[k] for the levels of `mask`
__global__ void __launch_bounds__(64) k_rp_set_front_merge(uint64_t mask, const uint32_t *__restrict__ front_new, uint32_t *__restrict__ front) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= bppp_set::MAX_LEVELS * 8) return;
  if ((mask >> (t >> 3)) & 1) front[t] = front_new[t];
}

// One lane.  pk [m][8] = P_0 .. P_{m-1}; rbag [m][8]: rbag[p] = bag (P_p, ..., P_{m-1}), so rbag[0] is the bag; root8 [8] = the root (each may be NULL:
// the root call wants no scratch).  peaks_out [m][8] and root_out [8] (may be NULL): the same as bytes, a word holding four bytes in memory order.
__global__ void __launch_bounds__(64) k_rp_set_bags(uint64_t n, uint32_t row_bytes, SetNodes S, ExDomain db, ExDomain dr, uint32_t *__restrict__ pk, uint32_t *__restrict__ rbag,
                                                    uint32_t *__restrict__ peaks_out, uint32_t *__restrict__ root_out) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t m = bppp_set::popcount(n);
  uint32_t p = m;
  for (uint32_t k = 0; k < 64; k++) {                   // from the lowest level up: P_{m-1} first
    if (!bppp_set::has_peak(n, k)) continue;
    p--;
    uint32_t P[8], st[8];
    const uint32_t *src = peak_ptr(S, n, k);
    for (int q = 0; q < 8; q++) P[q] = src[q];
    if (p == m - 1) { for (int q = 0; q < 8; q++) acc[q] = P[q]; }
    else { hash_pair(db, P, acc, st); for (int q = 0; q < 8; q++) acc[q] = st[q]; }
    for (int q = 0; q < 8; q++) {
      if (pk) pk[p * 8 + q] = P[q];
      if (rbag) rbag[p * 8 + q] = acc[q];
      if (peaks_out) peaks_out[p * 8 + q] = __builtin_bswap32(P[q]);
    }
  }
  if (!root_out) return;
  uint32_t st[8];
  hash_root(dr, n, row_bytes, acc, st);
  for (int q = 0; q < 8; q++) root_out[q] = __builtin_bswap32(st[q]);
}

// lane t: slot t % L of query t / L, L = bit_length (n) >= 1; idx[q] < n was checked by the caller.  A full store only.
__global__ void __launch_bounds__(64) k_rp_set_paths(uint64_t nq, uint64_t n, uint32_t L, SetNodes S, const uint32_t *__restrict__ pk, const uint32_t *__restrict__ rbag,
                                                     const uint64_t *__restrict__ idx, uint32_t *__restrict__ paths) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t qy = t / L;
  if (qy >= nq) return;
  const uint32_t s = (uint32_t)(t % L);
  const uint64_t i = idx[qy];
  if (i >= n) return;
  const bppp_set::Locate W = bppp_set::locate(n, i);
  const bppp_set::Slot sl = bppp_set::path_slot(n, i, W, s);
  const uint32_t *src = sl.kind == bppp_set::SLOT_SIBLING ? S.lvl[sl.level] + sl.index * 8 : sl.kind == bppp_set::SLOT_RIGHT_BAG ? rbag + sl.peak * 8
                        : sl.kind == bppp_set::SLOT_PEAK ? pk + sl.peak * 8 : nullptr;
  for (int q = 0; q < 8; q++) paths[t * 8 + q] = src ? __builtin_bswap32(src[q]) : 0u;
}

// the verdict of query t: idx[t], rows[t][row_bytes], paths[t][32 L] against `root` of n rows.  The first that applies: BAD_INDEX, BAD_PADDING,
// MISMATCH, OK; any[0] is raised by a query that is not OK (every lane that stores there stores the same word)
__global__ void __launch_bounds__(64) k_rp_set_verify(uint64_t nq, uint64_t n, uint32_t row_bytes, uint32_t L, SetDomains D, ExDomain root, const uint64_t *__restrict__ idx,
                                                      const uint8_t *__restrict__ rows, const uint8_t *__restrict__ paths, uint32_t *__restrict__ status, uint32_t *__restrict__ any) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nq) return;
  const uint64_t i = idx[t];
  uint32_t verdict = BPPP_RP_SET_OK;
  if (i >= n) verdict = BPPP_RP_SET_BAD_INDEX;
  else {
    const bppp_set::Locate W = bppp_set::locate(n, i);
    const uint8_t *path = paths + (size_t)t * 32 * L;
    uint32_t tail = 0;                                   // W.used <= L (csrc/rpset_plan.hpp); both loops are bounded by L all the same
    for (uint32_t o = 0; o < 32 * L; o++) if (o >= 32 * W.used) tail |= path[o];
    if (tail) verdict = BPPP_RP_SET_BAD_PADDING;
    else {
      uint32_t acc[8], sib[8], st[8];
      hash_leaf(D.leaf, rows + (size_t)t * row_bytes, row_bytes, acc);
      for (uint32_t s = 0; s < L; s++) {
        if (s >= W.used) break;
        for (int q = 0; q < 8; q++) {
          const uint8_t *b = path + 32 * s + 4 * q;
          sib[q] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
        }
        if (s < W.h) { if ((i >> s) & 1) hash_pair(D.node, sib, acc, st); else hash_pair(D.node, acc, sib, st); }
        else if (s == W.h && W.p + 1 < W.m) hash_pair(D.bag, acc, sib, st);       // the peaks to the right, bagged
        else hash_pair(D.bag, sib, acc, st);                                      // a peak to the left
        for (int q = 0; q < 8; q++) acc[q] = st[q];
      }
      hash_root(D.root, n, row_bytes, acc, st);
      uint32_t diff = 0;
      for (int q = 0; q < 8; q++) diff |= st[q] ^ root.w[q];
      if (diff) verdict = BPPP_RP_SET_MISMATCH;
    }
  }
  if (status) status[t] = verdict;
  if (verdict != BPPP_RP_SET_OK) any[0] = 1u;
}

}  // namespace set
}  // namespace bppp
