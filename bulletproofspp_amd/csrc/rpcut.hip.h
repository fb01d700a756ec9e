// rpcut.hip.h — the kernels of cut-through (csrc/rpcut.hip, bppp_rp_cut_through* of include/bppp.h): the entries of a tally job matched by the
// 33-byte identity of the commitment they reference, the matched pairs dropped, the pool and the entries compacted, the claims added up.
//   k_cut_ident        per entry: put (x mod p) as 8 words (the tally's load, csrc/rplift.hip.h), the file's sign bit, the salted SipHash-2-4 of both
//   k_cut_insert       open-addressed table of 32-bit slots, linear probing, atomicCAS: the winner of a slot labels the group, a loser compares
//                      the whole identity against it and joins or walks on.  The hash routes; equality is decided on the 33 bytes
//   k_cut_lead         the lowest job position of every group (atomicMin): labels that do not depend on who won
//   k_cut_first        flag = "this entry is the first of its group"; its scan numbers the groups densely in order of first appearance
//   k_cut_key          key = 2 * group + subtracted
//   k_cut_hist / k_cut_scatter   stable LSD counting sort of the job positions on the key, 8 bits a pass: one wavefront a tile of 1024 positions,
//                      digit counts in LDS, ranks inside a round from ballots, rounds in job order
//   k_cut_bounds       the first and the last sorted position of every key, written by the lanes that see the key change
//   k_cut_status       rank within (group, sign) = sorted position - first position of the key; m = min of the group's two counts; the verdict
//   k_cut_rowflags / k_cut_rowmap / k_cut_entries / k_cut_gather   the two ordered compactions and the gather of the surviving rows
//   k_cut_scan_tile / k_cut_scan_add     exclusive scan of 32-bit counts, any length, by levels of 2048
//   k_cut_claims       the three claim columns added mod n, one partial a workgroup, then one workgroup over the partials
// Within one launch a lane learns about another workgroup only from the value an atomic returns (k_cut_insert); every array written with plain
// stores is read by later launches only.  Every kernel is bounds-checked on its own index and takes its loop bounds from arguments, never from
// device data.  Included by csrc/rpcut.hip alone.
#pragma once
#include "fe.hip.h"
#include "rplift.hip.h"
#include "rpwords.hip.h"

namespace bppp {

static constexpr uint32_t CUT_NONE = 0xFFFFFFFFu;
static constexpr uint32_t CUT_SUB = 0x80000000u;           // bit 31 of an entry: subtracted
static constexpr uint32_t CUT_SORT_ROUNDS = 16, CUT_SORT_TILE = 64 * CUT_SORT_ROUNDS;   // positions per wavefront of the sort kernels
static constexpr uint32_t CUT_SCAN_PER = 8, CUT_SCAN_TILE = 256 * CUT_SCAN_PER;         // counts per workgroup of the scan
static constexpr uint32_t CUT_CLAIM_BLOCKS = 256;          // partial sums of the claims

// ---- SipHash-2-4 of the 36-byte message  x (8 words, least significant first) || sign, under the call's key
BPPP_DI uint64_t cut_rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }
BPPP_DI void cut_sipround(uint64_t &v0, uint64_t &v1, uint64_t &v2, uint64_t &v3) {
  v0 += v1; v1 = cut_rotl(v1, 13); v1 ^= v0; v0 = cut_rotl(v0, 32);
  v2 += v3; v3 = cut_rotl(v3, 16); v3 ^= v2;
  v0 += v3; v3 = cut_rotl(v3, 21); v3 ^= v0;
  v2 += v1; v1 = cut_rotl(v1, 17); v1 ^= v2; v2 = cut_rotl(v2, 32);
}
BPPP_DI uint64_t cut_hash(const fe &x, uint32_t sign, uint64_t k0, uint64_t k1) {
  uint64_t v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull, v2 = k0 ^ 0x6c7967656e657261ull, v3 = k1 ^ 0x7465646279746573ull;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint64_t m = i < 4 ? ((uint64_t)x.v[2 * i] | ((uint64_t)x.v[2 * i + 1] << 32)) : (((uint64_t)36 << 56) | sign);
    v3 ^= m;
    cut_sipround(v0, v1, v2, v3); cut_sipround(v0, v1, v2, v3);
    v0 ^= m;
  }
  v2 ^= 0xff;
  for (int i = 0; i < 4; i++) cut_sipround(v0, v1, v2, v3);
  return v0 ^ v1 ^ v2 ^ v3;
}

// ---- entry e -> idw[e][8] = x mod p of the commitment it references, hs[e] = the routing hash with the file's sign bit in bit 0 (same: every hash
// zero, the test hook's one chain).  entries has passed k_rp_tally_validate: every index is below rows * nr.
__global__ void __launch_bounds__(256) k_cut_ident(uint32_t nnz, uint32_t nr, uint32_t coms_bytes, const uint32_t *__restrict__ entries, const uint8_t *__restrict__ coms,
                                                   uint64_t k0, uint64_t k1, uint32_t same, uint32_t *__restrict__ idw, uint64_t *__restrict__ hs) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const uint32_t j = entries[e] & ~CUT_SUB, r = j / nr, i = j - r * nr;
  const uint8_t *file = coms + (size_t)r * coms_bytes;
  const uint32_t sign = (file[i >> 3] >> (i & 7)) & 1u;
  const fe x = load_field_be<0>(file + (nr + 7) / 8 + (size_t)i * 32);
  fe_store(idw + e * 8, x);
  const uint64_t h = same ? 0 : cut_hash(x, sign, k0, k1);
  hs[e] = (h & ~(uint64_t)1) | sign;
}

// a word that other workgroups change by atomics in this launch, read by an atomic load at agent scope (never from this CU's L1).  Thousands of
// entries of ONE identity meet in one word: loads of it are served side by side, read-modify-writes one after another, so the kernels below look
// first and skip the read-modify-write that could not change the word any more
BPPP_DI uint32_t cut_peek(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- the table: tab [mask + 1] starts as CUT_NONE everywhere.  Entry e walks from its hash; at an empty slot its CAS wins and e labels the slot;
// at a taken slot it compares hs (hash and sign bit) and the 8 words of x with the winner's, which an EARLIER launch wrote: equal -> it joins.
// mask + 1 >= nnz, so a walk of mask + 1 steps meets its group or an empty slot; err[0] is raised if it did not (never: a broken table).
__global__ void __launch_bounds__(256) k_cut_insert(uint32_t nnz, uint32_t mask, const uint32_t *__restrict__ idw, const uint64_t *__restrict__ hs, uint32_t *tab,
                                                    uint32_t *__restrict__ slot, uint32_t *__restrict__ err) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const uint64_t h = hs[e];
  uint32_t mine[8];
#pragma unroll
  for (int k = 0; k < 8; k++) mine[k] = idw[e * 8 + k];
  uint32_t s = (uint32_t)(h >> 1) & mask, found = CUT_NONE;
  for (uint64_t step = 0; step <= mask; step++) {
    uint32_t v = cut_peek(tab + s);              // a taken slot never changes again: only an empty one needs the CAS
    if (v == CUT_NONE) v = atomicCAS(tab + s, CUT_NONE, (uint32_t)e);
    if (v == CUT_NONE || v == (uint32_t)e) { found = s; break; }
    if (v < nnz && hs[v] == h) {
      uint32_t d = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) d |= idw[(size_t)v * 8 + k] ^ mine[k];
      if (!d) { found = s; break; }
    }
    s = (s + 1) & mask;
  }
  if (found == CUT_NONE) { atomicOr(err, 1u); found = 0; }
  slot[e] = found;
}

// ---- win[e] = the label of e's slot; lead[label] = the lowest position of the group (lead starts as CUT_NONE)
__global__ void __launch_bounds__(256) k_cut_lead(uint32_t nnz, uint32_t mask, const uint32_t *__restrict__ tab, const uint32_t *__restrict__ slot, uint32_t *__restrict__ win,
                                                  uint32_t *lead) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  uint32_t w = tab[slot[e] & mask];
  if (w >= nnz) w = (uint32_t)e;               // never: the slot of an inserted entry is taken
  win[e] = w;
  if (cut_peek(lead + w) > (uint32_t)e) atomicMin(lead + w, (uint32_t)e);      // the word only falls: one that is not above e stays so
}
// ldr[e] = the first position of e's group, flag[e] = e is that position
__global__ void __launch_bounds__(256) k_cut_first(uint32_t nnz, const uint32_t *__restrict__ win, const uint32_t *__restrict__ lead, uint32_t *__restrict__ ldr,
                                                   uint32_t *__restrict__ flag) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  uint32_t l = lead[win[e]];
  if (l > e) l = (uint32_t)e;                  // never
  ldr[e] = l;
  flag[e] = l == e ? 1u : 0u;
}
// key[e] = 2 * (dense number of e's group) + subtracted
__global__ void __launch_bounds__(256) k_cut_key(uint32_t nnz, const uint32_t *__restrict__ entries, const uint32_t *__restrict__ ldr, const uint32_t *__restrict__ gpos,
                                                 uint32_t *__restrict__ key) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  uint32_t g = gpos[ldr[e]];
  if (g >= nnz) g = 0;                         // never: there are at most nnz groups
  key[e] = 2 * g + (entries[e] >> 31);
}

// ---- one pass of the sort.  Position i of the pass's order is entry in[i] (in NULL: i itself, the first pass); wavefront b owns positions
// [b * CUT_SORT_TILE, ...).  hist[d * nb + b] = how many of them carry digit d: scanned digit-major, hoff[d * nb + b] is where b's first such
// position goes, behind every lower digit and behind the same digit of every earlier wavefront.
__global__ void __launch_bounds__(64) k_cut_hist(uint32_t n, uint32_t shift, const uint32_t *__restrict__ key, const uint32_t *__restrict__ in, uint32_t nb,
                                                 uint32_t *__restrict__ hist) {
  __shared__ uint32_t cnt[256];
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  if (b >= nb) return;
  for (uint32_t d = lane; d < 256; d += 64) cnt[d] = 0;
  __syncthreads();
  for (uint32_t r = 0; r < CUT_SORT_ROUNDS; r++) {
    const uint64_t i = (uint64_t)b * CUT_SORT_TILE + r * 64 + lane;
    if (i >= n) continue;
    uint32_t e = in ? in[i] : (uint32_t)i;
    if (e >= n) e = 0;                         // never: in is a permutation of [0, n)
    atomicAdd(&cnt[(key[e] >> shift) & 255u], 1u);
  }
  __syncthreads();
  for (uint32_t d = lane; d < 256; d += 64) hist[(size_t)d * nb + b] = cnt[d];
}
// the lanes of a round that carry the same digit find each other by ballots; the rank inside the round is the number of lower lanes among them, and
// the highest of them moves the digit's counter on.  Rounds follow each other in job order, so equal keys keep their order: the sort is stable.
__global__ void __launch_bounds__(64) k_cut_scatter(uint32_t n, uint32_t shift, const uint32_t *__restrict__ key, const uint32_t *__restrict__ in, uint32_t nb,
                                                    const uint32_t *__restrict__ hoff, uint32_t *__restrict__ out) {
  __shared__ uint32_t cnt[256];
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  if (b >= nb) return;
  for (uint32_t d = lane; d < 256; d += 64) cnt[d] = hoff[(size_t)d * nb + b];
  __syncthreads();
  for (uint32_t r = 0; r < CUT_SORT_ROUNDS; r++) {
    const uint64_t i = (uint64_t)b * CUT_SORT_TILE + r * 64 + lane;
    const bool valid = i < n;
    uint32_t e = 0, d = 0;
    if (valid) {
      e = in ? in[i] : (uint32_t)i;
      if (e >= n) e = 0;                       // never
      d = (key[e] >> shift) & 255u;
    }
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (uint32_t bit = 0; bit < 8; bit++) {
      const bool set = ((d >> bit) & 1u) != 0;
      const uint64_t bm = __ballot(valid && set);
      peers &= set ? bm : ~bm;
    }
    const uint32_t base = valid ? cnt[d] : 0u;
    __syncthreads();
    if (valid) {
      const uint64_t to = (uint64_t)base + (uint32_t)__popcll(peers & (((uint64_t)1 << lane) - 1));
      if (to < n) out[to] = e;                 // always: the offsets come from the counts of these very digits
      if (lane == 63u - (uint32_t)__clzll((long long)peers)) cnt[d] = base + (uint32_t)__popcll(peers);
    }
    __syncthreads();
  }
}

// ---- sorted position q holds entry perm[q]; the positions of one key are contiguous and in job order.  k_cut_bounds: the first of them writes
// startk[key] = q and the last endk[key] = q + 1 (both start as zero, so a key without entries has the count 0): one writer a word, no atomics.
__global__ void __launch_bounds__(256) k_cut_bounds(uint32_t nnz, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ key, uint32_t *__restrict__ startk,
                                                    uint32_t *__restrict__ endk) {
  const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nnz) return;
  const uint32_t e = perm[q], k = key[e < nnz ? e : 0];
  if (q == 0 || key[perm[q - 1] < nnz ? perm[q - 1] : 0] != k) startk[k] = (uint32_t)q;
  if (q + 1 == nnz || key[perm[q + 1] < nnz ? perm[q + 1] : 0] != k) endk[k] = (uint32_t)q + 1;
}
// With rank = q - startk[key] and m = min of the group's two
// counts: rank < m is cut, rank == m is the first survivor, rank > m survives behind it (only the longer side has any).  A survivor marks its row:
// bit 1 = referenced by a surviving ADDED entry, bit 0 = by a surviving subtracted one.  tot[0] += cut, tot[1] += kept again.
__global__ void __launch_bounds__(256) k_cut_status(uint32_t nnz, uint32_t nr, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ key,
                                                    const uint32_t *__restrict__ startk, const uint32_t *__restrict__ endk, const uint32_t *__restrict__ entries,
                                                    uint32_t *__restrict__ status, uint32_t *__restrict__ keep, uint32_t *rowmark, uint32_t *tot) {
  const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t st = BPPP_RP_CUT_KEPT;
  const bool valid = q < nnz;
  if (valid) {
    uint32_t e = perm[q];
    if (e >= nnz) e = 0;                       // never
    const uint32_t k = key[e], rank = (uint32_t)q - startk[k], m = min(endk[k] - startk[k], endk[k ^ 1u] - startk[k ^ 1u]), ent = entries[e];
    st = rank < m ? BPPP_RP_CUT_SPENT : rank == m ? BPPP_RP_CUT_KEPT : BPPP_RP_CUT_KEPT_AGAIN;
    status[e] = st;
    keep[e] = st != BPPP_RP_CUT_SPENT ? 1u : 0u;
    if (st != BPPP_RP_CUT_SPENT) {
      uint32_t *mark = rowmark + (ent & ~CUT_SUB) / nr;
      const uint32_t bit = (ent >> 31) ? 1u : 2u;
      if (!(cut_peek(mark) & bit)) atomicOr(mark, bit);        // the bits only rise
    }
  }
  const uint64_t cut = __ballot(valid && st == BPPP_RP_CUT_SPENT), again = __ballot(valid && st == BPPP_RP_CUT_KEPT_AGAIN);
  if ((threadIdx.x & 63u) == 0) {
    if (cut) atomicAdd(tot, (uint32_t)__popcll(cut));
    if (again) atomicAdd(tot + 1, (uint32_t)__popcll(again));
  }
}

// ---- rows: F[r] = row r holds a new output (a surviving added entry references it), F[rows + r] = it survives without one.  The scan of F as ONE
// array of 2 rows counts puts the second group behind the first: P[r] / P[rows + r] is the row's new index.
__global__ void __launch_bounds__(256) k_cut_rowflags(uint32_t rows, const uint32_t *__restrict__ rowmark, uint32_t *__restrict__ F) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const uint32_t m = rowmark[r];
  F[r] = (m & 2u) ? 1u : 0u;
  F[(size_t)rows + r] = (m && !(m & 2u)) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_cut_rowmap(uint32_t rows, const uint32_t *__restrict__ rowmark, const uint32_t *__restrict__ P, uint32_t *__restrict__ row_map,
                                                    uint32_t *__restrict__ rowinv) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const uint32_t m = rowmark[r];
  uint32_t k = CUT_NONE;
  if (m) {
    k = (m & 2u) ? P[r] : P[(size_t)rows + r];
    if (k < rows) row_map[k] = (uint32_t)r; else k = CUT_NONE;      // always below rows: at most rows flags are set
  }
  rowinv[r] = k;
}
// surviving entry e goes to slot epos[e] with its sign and its index re-based to the new pool
__global__ void __launch_bounds__(256) k_cut_entries(uint32_t nnz, uint32_t nr, uint32_t rows, const uint32_t *__restrict__ entries, const uint32_t *__restrict__ keep,
                                                     const uint32_t *__restrict__ epos, const uint32_t *__restrict__ rowinv, uint32_t *__restrict__ out) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz || !keep[e]) return;
  const uint32_t ent = entries[e], j = ent & ~CUT_SUB, r = j / nr, k = rowinv[r], to = epos[e];
  if (k >= rows || to >= nnz) return;          // never: a survivor's row was marked, and there are at most nnz survivors
  out[to] = (ent & CUT_SUB) | (k * nr + (j - r * nr));
}
// the new pool, 16 bytes of it a lane: byte p of it is byte p % cb of old row row_map[p / cb]; dst is 16-byte aligned, the last chunk may be short
__global__ void __launch_bounds__(256) k_cut_gather(uint64_t total, uint32_t cb, uint32_t rows, const uint32_t *__restrict__ row_map, const uint8_t *__restrict__ src,
                                                    uint8_t *__restrict__ dst) {
  const uint64_t o = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  if (o >= total) return;
  const uint32_t n = total - o < 16 ? (uint32_t)(total - o) : 16u;
  uint64_t k = o / cb;
  uint32_t off = (uint32_t)(o - k * cb);
  uint32_t r = row_map[k];
  if (r >= rows) r = 0;                        // never
  uint32_t w[4] = {0, 0, 0, 0};
  for (uint32_t t = 0; t < n; t++) {
    w[t >> 2] |= (uint32_t)src[(size_t)r * cb + off] << (8 * (t & 3));
    if (++off == cb && t + 1 < n) {
      off = 0; k++;
      r = row_map[k];
      if (r >= rows) r = 0;
    }
  }
  if (n == 16) *(uint4 *)(dst + o) = make_uint4(w[0], w[1], w[2], w[3]);
  else for (uint32_t t = 0; t < n; t++) dst[o + t] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
}
// what the host reads back in one copy: new_rows, out_rows, new_nnz, cut, kept again
__global__ void k_cut_counts(uint32_t nnz, uint32_t rows, const uint32_t *__restrict__ epos, const uint32_t *__restrict__ P, const uint32_t *__restrict__ tot,
                             uint32_t *__restrict__ res) {
  if (threadIdx.x || blockIdx.x) return;
  res[0] = P[2 * (size_t)rows]; res[1] = P[rows]; res[2] = epos[nnz]; res[3] = tot[0]; res[4] = tot[1];
}

// ---- exclusive scan of in [n] into out [n + 1] (out[n] = the total; the element behind the end counts as zero).  A workgroup scans CUT_SCAN_TILE
// elements and writes its total to tsum[b]; with more than one workgroup the totals are scanned the same way and k_cut_scan_add adds them back.
__global__ void __launch_bounds__(256) k_cut_scan_tile(uint64_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t *__restrict__ tsum) {
  __shared__ uint32_t wsum[4];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * CUT_SCAN_TILE + (uint64_t)t * CUT_SCAN_PER;
  uint32_t v[CUT_SCAN_PER], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < CUT_SCAN_PER; k++) { v[k] = base + k < n ? in[base + k] : 0u; sum += v[k]; }
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if ((int)lane >= d) inc += o; }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t pre = inc - sum;
  for (uint32_t k = 0; k < w; k++) pre += wsum[k];
#pragma unroll
  for (uint32_t k = 0; k < CUT_SCAN_PER; k++) { if (base + k <= n) out[base + k] = pre; pre += v[k]; }
  if (t == 255) tsum[blockIdx.x] = pre;
}
__global__ void __launch_bounds__(256) k_cut_scan_add(uint64_t n, const uint32_t *__restrict__ tsc, uint32_t *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i <= n) out[i] += tsc[i / CUT_SCAN_TILE];
}

// ---- the claims.  cut_block_sum: the three running sums of a workgroup's 256 lanes added mod n into lane 0's (a tree of cross-lane moves, then the
// four wavefronts over LDS).  Addition mod n is exact, so the order of the tree does not show in the result.
BPPP_DI fe cut_fe_shfl_down(const fe &a, int d) { fe r; for (int k = 0; k < 8; k++) r.v[k] = __shfl_down(a.v[k], d); return r; }
BPPP_DI void cut_block_sum(fe acc[3], uint32_t *sh /* [4][24] */) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  for (int d = 32; d >= 1; d >>= 1)
    for (int s = 0; s < 3; s++) acc[s] = fe_add<1>(acc[s], cut_fe_shfl_down(acc[s], d));
  if (lane == 0) for (int s = 0; s < 3; s++) fe_store(sh + w * 24 + s * 8, acc[s]);
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t k = 1; k < 4; k++)
      for (int s = 0; s < 3; s++) acc[s] = fe_add<1>(acc[s], fe_load(sh + k * 24 + s * 8));
}
// part[b] = the sums over the claims this workgroup strides through: the amount reduced as a two's-complement integer (wi_smod_n), the type (zero
// on a binary handle) and the offset as given; one of those >= n lowers flag[0] to its sum
__global__ void __launch_bounds__(256) k_cut_claims(uint32_t nsums, uint32_t binary, const uint32_t *__restrict__ amounts, const uint32_t *__restrict__ types,
                                                    const uint32_t *__restrict__ offsets, uint32_t *__restrict__ part, uint32_t *flag) {
  __shared__ uint32_t sh[4 * 24];
  fe acc[3] = {fe_zero(), fe_zero(), fe_zero()};
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < nsums; t += (uint64_t)gridDim.x * 256) {
    const fe v[3] = {wi_smod_n(fe_load(amounts + t * 8)), binary ? fe_zero() : fe_load(types + t * 8), fe_load(offsets + t * 8)};
    if (!wi_canonical(v[1]) || !wi_canonical(v[2])) { atomicMin(flag, (uint32_t)t); continue; }
    for (int s = 0; s < 3; s++) acc[s] = fe_add<1>(acc[s], v[s]);
  }
  cut_block_sum(acc, sh);
  if (threadIdx.x == 0) for (int s = 0; s < 3; s++) fe_store(part + (size_t)blockIdx.x * 24 + s * 8, acc[s]);
}
// out [3][8] = the sum of the partials; the amount as bppp_rp_tally_claims writes it: a below 2^255, else a - n in two's complement
__global__ void __launch_bounds__(256) k_cut_claims_fin(uint32_t nparts, const uint32_t *__restrict__ part, uint32_t *__restrict__ out) {
  __shared__ uint32_t sh[4 * 24];
  fe acc[3] = {fe_zero(), fe_zero(), fe_zero()};
  for (uint32_t b = threadIdx.x; b < nparts; b += 256)
    for (int s = 0; s < 3; s++) acc[s] = fe_add<1>(acc[s], fe_load(part + (size_t)b * 24 + s * 8));
  cut_block_sum(acc, sh);
  if (threadIdx.x) return;
  fe a = acc[0];
  if (wi_neg(a)) raw_sub(a, acc[0], fr_modulus());
  fe_store(out, a); fe_store(out + 8, acc[1]); fe_store(out + 16, acc[2]);
}

}  // namespace bppp
