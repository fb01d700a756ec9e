// msm.hip — signed-digit Pippenger multi-scalar multiplication for gfx950.
//
// Replaces FastInnerProduct.innerProduct (src/Commitment.hs:325-335) reached through `commit`
// (src/Commitment.hs:416-417).  The reference is a 256-row bit-serial Straus loop; this is a
// different algorithm that yields the same group element:
//
//   1. k_digits      reduceScalar's sign fold (Commitment.hs:276-279, :366) + signed c-bit window
//                    recode (the format of recode.hip.h); coalesced 32-B scalar loads, u16 digits out.
//   2. k_hist / k_count_tiles / k_scan_apply / k_scatter, k_scatter_ranges
//                    counting sort of (window, |digit|) keys: the bucket histogram and cursors are
//                    staged in LDS (<= 128 KiB per workgroup), so HBM sees only coalesced streams.
//   3. k_acc_points / k_merge / k_merge_heavy
//                    load-balanced bucket accumulation: every lane owns exactly L consecutive
//                    sorted entries (4 bytes each: sign | point index; the bucket of a position follows from the
//                    bucket offsets start[], it is not stored), sums runs of one bucket in an XYZZ register
//                    accumulator with mixed adds and stores complete buckets; a bucket that
//                    straddles lanes is finished by k_merge (one lane per bucket) or, when it spans
//                    many lanes (skewed scalars), by one wavefront in k_merge_heavy.  Batches, registered bases and one
//                    MSM with windows under 16 bits.
//   3'. k_order / k_acc_points_sized / k_merge_heavy<true>
//                    one MSM over arbitrary points with 16-bit windows (MsmTune::acc_sized): a lane sums one whole
//                    bucket (or a piece of <= 128 entries of a larger one), the buckets dispatched in descending order
//                    of size so that the lanes of a wavefront run equally long: no boundary logic in the loop, no
//                    partial sums unless the scalars are skewed.  k_acc_points_sized29 (MsmTune::acc_fq29, the default) is the same
//                    kernel with the accumulator in 9 x 29-bit limbs (fq29.hip.h): 81 partial products per multiplication, not 100.
//                    k_acc_points_sized29_fast (MsmTune::acc_fast, the default) is that kernel on an addition that tests nothing, with one
//                    zero test of ZZ per item and the redo of a flagged item by the complete loop.
//   4. k_reduce_marg / k_reduce_tail_quad
//                    sum_m m*B_m per window by MARGINAL SUMS (m = LO*hi + lo: plain row and column sums, every lane busy,
//                    then two short weighted sums); k_reduce1/2 (per-lane running sums + wavefront suffix scans) for windows
//                    under 256 buckets, k_reduce_groups for thousands of small windows.
//   5. window combine: Horner over <= 65 window sums — on the host for one MSM (a 256-doubling
//                    dependency chain), in k_window_combine for batches.
//
// The plan of a call (window layout, chunk counts, kernel forms, reduction geometry) and the layout of its workspace are plain host code in
// msm_plan.hpp; this file holds the kernels and, at the end, the stages that launch them.
//
// Integer / carry-chain work on the VALU; nothing here is a dense contraction, so no MFMA.
#include <algorithm>
#include <vector>
#include "ctx.hpp"
#include "ec.hip.h"
#include "ec29.hip.h"
#include "ec_quad.hip.h"
#include "hostcurve.hpp"
#include "hostmath.hpp"
#include "recode.hip.h"

namespace bppp {

static_assert(MSM_XYZZ_WORDS == XYZZ_WORDS, "msm_plan.hpp sizes the workspace by the stored point of ec.hip.h");
static_assert(sizeof(MsmPair) == sizeof(uint2) && sizeof(MsmQuad) == sizeof(uint4) && alignof(MsmQuad) == alignof(uint4), "the workspace's pairs and quadruples are the kernels' uint2 / uint4");

// ------------------------------------------------------------------------------------------------
// 1. digits
// Window widths: the first `acnt` windows are c bits wide, the others c - 1 (balanced windows, make_plan; acnt = W: all c).  A digit of a
// narrow window is stored re-biased by 2^(c-2), so that every consumer reads  stored - 2^(c-1)  as the signed digit whatever the width.
// top >= 0 (a plan without carry window, window_layout): K leaves row `top`, the last one, unbiased and its digit d in [0, 2^(cw-1)] is stored
// NEGATED, as 2^(c-1) - d: magnitude, bucket and zero test are those of every other row, and the scatter flips the sign of that row's entries.
__global__ void __launch_bounds__(256) k_digits(const uint32_t *__restrict__ scalars, uint64_t total, uint32_t n, uint32_t stride, int c,
                                                int W, int acnt, int top, RecodeK K, uint16_t *__restrict__ dig,
                                                unsigned long long *__restrict__ negmask, uint32_t *__restrict__ zero, uint32_t nzero,
                                                uint32_t *__restrict__ zero2, uint32_t nzero2) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // the call's counters (heavy_count, k_reduce_tail_quad's tickets, the scan's tile sums): this is the first kernel of the call
  for (uint64_t j = i; j < nzero; j += (uint64_t)gridDim.x * blockDim.x) zero[j] = 0u;
  for (uint64_t j = i; j < nzero2; j += (uint64_t)gridDim.x * blockDim.x) zero2[j] = 0u;
  bool valid = i < total;
  bool neg = false;
  if (valid) {
    uint32_t sp[9];
    neg = recode_fold(fe_load(scalars + 8 * i), K, sp);
    uint32_t inst = (uint32_t)(i / n), j = (uint32_t)(i % n);
    size_t base = (size_t)inst * W * stride + j;
    for (int w = 0; w < W; w++) {
      const int cw = w < acnt ? c : c - 1;
      const uint32_t bias = w < acnt ? 0u : (1u << (c - 2));
      const uint32_t f = recode_next(sp, cw);
      dig[base + (size_t)w * stride] = (uint16_t)(w == top ? (1u << (c - 1)) - f : f + bias);
    }
  }
  unsigned long long m = __ballot(valid && neg);
  if ((threadIdx.x & 63) == 0 && (i - (i & 63)) < total) negmask[i >> 6] = m;
}

// ------------------------------------------------------------------------------------------------
// 2. counting sort by (instance, window, |digit|)
// Both sort kernels read 8 consecutive u16 digits per lane with ONE 16-byte load (n is padded to a multiple of 8 in the
// digit buffer's row stride), so each lane has 8 independent LDS atomics / stores in flight instead of a dependent
// load -> atomic -> store chain per entry (the scattered stores are latency-, not bandwidth-bound).
// h16 (MsmPlan::hist16: a ranged scatter's plan, no chunk longer than 65535 terms, so no count above that): the counts leave as 16-bit values,
// eight per lane in one 16-byte store, in the same [row][chunk][bucket] order — half the bytes, in the front half of the allocation.
__global__ void k_hist(const uint16_t *__restrict__ dig, uint32_t n, uint32_t stride, int c, int CH, uint32_t *__restrict__ blockhist, int h16) {
  extern __shared__ uint32_t lh[];
  const int M = 1 << (c - 1);
  const uint32_t nbw = blockIdx.x, ch = blockIdx.y;
  for (int t = threadIdx.x; t < M; t += blockDim.x) lh[t] = 0;
  __syncthreads();
  uint32_t per = (((n + CH - 1) / CH) + 7u) & ~7u, lo = ch * per, hi = min(n, lo + per);
  const uint16_t *d = dig + (size_t)nbw * stride;
  // the digits of the next step are loaded before this step's are counted (a second register set, as marg_serial_sum's buckets): a lane
  // has two loads in flight, not one.  Every load, the first and the ones ahead, is guarded by its own j < hi.
  const uint32_t step = blockDim.x * 8;
  uint32_t j0 = lo + threadIdx.x * 8;
  uint4 pk = make_uint4(0u, 0u, 0u, 0u);
  if (j0 < hi) pk = *reinterpret_cast<const uint4 *>(d + j0);
  while (j0 < hi) {
    const uint32_t jn = j0 + step;
    uint4 pkn = pk;
    if (jn < hi) pkn = *reinterpret_cast<const uint4 *>(d + jn);
    uint32_t w[4] = {pk.x, pk.y, pk.z, pk.w};
#pragma unroll
    for (int k = 0; k < 8; k++) {
      int v = (int)((w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu) - M;
      if (j0 + k < hi && v) atomicAdd(&lh[(v < 0 ? -v : v) - 1], 1u);
    }
    pk = pkn; j0 = jn;
  }
  __syncthreads();
  if (h16) {                                                // M is 2^15 (a ranged scatter's plan): rows of 64 KiB, 16-byte aligned
    uint4 *out16 = reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(blockhist) + ((size_t)nbw * CH + ch) * M);
    const uint4 *l4 = reinterpret_cast<const uint4 *>(lh);
    for (int t = threadIdx.x; t < M / 8; t += blockDim.x) {
      const uint4 a = l4[2 * t], b = l4[2 * t + 1];
      out16[t] = make_uint4(a.x | (a.y << 16), a.z | (a.w << 16), b.x | (b.y << 16), b.z | (b.w << 16));
    }
    return;
  }
  uint32_t *out = blockhist + ((size_t)nbw * CH + ch) * M;
  for (int t = threadIdx.x; t < M; t += blockDim.x) out[t] = lh[t];
}

// Exclusive scan over the bucket totals in two launches.  k_count_tiles, one lane per flat bucket: exclusive prefix over the chunks (in
// place) and the bucket total `count`; a workgroup adds its 256 totals to the sum of its tile of SCAN_TILE buckets (tile_sums is zero at
// launch: k_digits).  k_scan_apply, one workgroup per tile: its offset is the sum of the tile sums before it — a few hundred words that
// every workgroup adds up for itself, which is cheaper than a launch of one workgroup that scans them — then a block-level scan of the tile.
// Those reads grow as ntiles^2 / 2 words: 9 K at 2^20 terms (136 tiles), 0.8 M at the largest batched shapes in use (~1300 tiles).  A plan
// may reach 2^32 buckets only on paper — the bucket array alone is 160 B each, so 288 GB of HBM hold under 2^31 / 4096 = 2^19 tiles, and
// anything near that is seconds of accumulation; at 2^27 buckets (21 GB, 32 K tiles) it is 2 GB of L2 reads, about a millisecond.
__global__ void __launch_bounds__(256) k_count_tiles(uint32_t *__restrict__ blockhist, int M, int CH, uint64_t FB, uint32_t *__restrict__ count,
                                                     uint32_t *__restrict__ tile_sums) {
  __shared__ uint32_t ws[4];
  const uint64_t fb = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t s = 0;
  if (fb < FB) {
    const uint64_t nbw = fb / M, mb = fb % M;
    for (int ch = 0; ch < CH; ch++) {
      const size_t at = ((size_t)nbw * CH + ch) * M + mb;
      const uint32_t t = blockhist[at];
      blockhist[at] = s;
      s += t;
    }
    count[fb] = s;
  }
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(tile_sums + blockIdx.x / (SCAN_TILE / 256), ws[0] + ws[1] + ws[2] + ws[3]);
}
// k_count_tiles on the 16-bit counts of k_hist (MsmPlan::hist16).  A lane takes TWO neighbouring buckets, one 32-bit word per chunk, so a
// wavefront's requests stay 256 bytes wide, and a workgroup 512 buckets; M and FB are even, so both buckets lie in one window.  The exclusive
// prefix goes back in place modulo 2^16: exact for a bucket of fewer than 65536 entries, and the scatters rebuild the prefixes of a larger one
// from the wraps of its stored sequence (scatter_load_cursors16).  count[] and the tile sums are 32-bit, as k_count_tiles'.  The loads of
// eight chunks are requested before the first prefix is stored (a load after a store to the same array would wait for it).
__global__ void __launch_bounds__(256) k_count_tiles16(uint32_t *__restrict__ blockhist, int M, int CH, uint64_t FB, uint32_t *__restrict__ count,
                                                       uint32_t *__restrict__ tile_sums) {
  __shared__ uint32_t ws[4];
  const uint64_t fb = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  uint32_t s0 = 0, s1 = 0;
  if (fb < FB) {
    const uint64_t nbw = fb / M, mb = fb % M;
    uint32_t *p = blockhist + ((size_t)nbw * CH * M + mb) / 2;        // the word that holds the two counts of chunk 0
    const size_t row = (size_t)M / 2;                                 // words per chunk row
    for (int ch0 = 0; ch0 < CH; ch0 += 8) {
      uint32_t t[8];
#pragma unroll
      for (int k = 0; k < 8; k++) t[k] = ch0 + k < CH ? p[(size_t)(ch0 + k) * row] : 0u;
#pragma unroll
      for (int k = 0; k < 8; k++)
        if (ch0 + k < CH) {
          p[(size_t)(ch0 + k) * row] = (s0 & 0xFFFFu) | (s1 << 16);
          s0 += t[k] & 0xFFFFu; s1 += t[k] >> 16;
        }
    }
    *reinterpret_cast<uint2 *>(count + fb) = make_uint2(s0, s1);
  }
  uint32_t s = s0 + s1;
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(tile_sums + blockIdx.x / (SCAN_TILE / 512), ws[0] + ws[1] + ws[2] + ws[3]);
}
// An ITEM of the sized accumulation (section 3'): a bucket of at most ACC_CAP entries, or a piece of ACC_CAP entries (the last one: the rest) of
// a larger one.  size_hist (the sized route only, else null; zero at launch: k_digits) counts the items by size: the tile's histogram in LDS,
// then one global atomic per non-empty bin.  Bin size - 1 is the word (size - 1) * ACC_LINE: a bin has a 128-byte line to itself, so that the
// atomics of different bins do not queue on one line.  (SCAN_TILE, ACC_CAP, ACC_LINE: msm_plan.hpp)
__global__ void __launch_bounds__(256) k_scan_apply(const uint32_t *__restrict__ in, uint64_t n, const uint32_t *__restrict__ tile_sums,
                                                    uint32_t *__restrict__ out, uint32_t *__restrict__ size_hist) {
  // the tile's offset, then a block-level exclusive scan of the tile (16 per thread); the last lane of the last tile writes the total out[n]
  __shared__ uint32_t wsum[4], wpre[4];
  __shared__ uint32_t lh[ACC_CAP];
  if (size_hist && threadIdx.x < ACC_CAP) lh[threadIdx.x] = 0;
  uint32_t pre = 0;
  for (uint32_t i = threadIdx.x; i < blockIdx.x; i += 256) pre += tile_sums[i];
  for (int d = 32; d >= 1; d >>= 1) pre += __shfl_down(pre, d, 64);
  if ((threadIdx.x & 63) == 0) wpre[threadIdx.x >> 6] = pre;
  uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * 16;
  uint32_t v[16], s = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) { v[k] = (base + k < n) ? in[base + k] : 0; s += v[k]; }
  uint32_t inc = s;
  for (int d = 1; d < 64; d <<= 1) { uint32_t t = __shfl_up(inc, d, 64); if ((int)(threadIdx.x & 63) >= d) inc += t; }
  if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
  __syncthreads();
  if (size_hist) {
#pragma unroll
    for (int k = 0; k < 16; k++) {
      if (v[k] >= ACC_CAP) atomicAdd(&lh[ACC_CAP - 1], v[k] / ACC_CAP);
      if (v[k] % ACC_CAP) atomicAdd(&lh[v[k] % ACC_CAP - 1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < ACC_CAP && lh[threadIdx.x]) atomicAdd(size_hist + threadIdx.x * ACC_LINE, lh[threadIdx.x]);
  }
  uint32_t woff = 0;
  for (int w = 0; w < (int)(threadIdx.x >> 6); w++) woff += wsum[w];
  uint32_t run = wpre[0] + wpre[1] + wpre[2] + wpre[3] + woff + inc - s;
#pragma unroll
  for (int k = 0; k < 16; k++) { if (base + k < n) out[base + k] = run; run += v[k]; }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) out[n] = run;
}

__global__ void k_scatter(const uint16_t *__restrict__ dig, const unsigned long long *__restrict__ negmask, uint32_t n, uint32_t stride, int c,
                          int CH, int W, const uint32_t *__restrict__ blockhist, const uint32_t *__restrict__ start,
                          uint32_t *__restrict__ sorted, uint32_t flat_stride, int top) {
  extern __shared__ uint32_t lh[];
  const int M = 1 << (c - 1);
  const uint32_t nbw = blockIdx.x, ch = blockIdx.y;
  const uint32_t flip = (int)(nbw % W) == top ? 1u : 0u;     // row `top` holds its digits negated (k_digits)
  const uint32_t *bh = blockhist + ((size_t)nbw * CH + ch) * M;
  // flat_stride != 0: the windows of an instance share one bucket set and the entry indexes the table row of its window
  const uint32_t *st = start + (size_t)(flat_stride ? nbw / W : nbw) * M;
  const uint32_t idx_base = flat_stride ? (nbw % W) * flat_stride : 0u;
  // cursors: four pairs of loads are in flight before the first of them is added into LDS
  for (int t0 = threadIdx.x; t0 < M; t0 += 4 * (int)blockDim.x) {
    uint32_t a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { const int t = t0 + i * (int)blockDim.x; a[i] = t < M ? st[t] : 0u; b[i] = t < M ? bh[t] : 0u; }
#pragma unroll
    for (int i = 0; i < 4; i++) { const int t = t0 + i * (int)blockDim.x; if (t < M) lh[t] = a[i] + b[i]; }
  }
  __syncthreads();
  uint32_t per = (((n + CH - 1) / CH) + 7u) & ~7u, lo = ch * per, hi = min(n, lo + per);
  const uint16_t *d = dig + (size_t)nbw * stride;
  const uint64_t inst0 = (uint64_t)(nbw / W) * n;
  // the next step's digits and sign words are loaded before this step's entries are placed (k_hist); each load is guarded by its own j < hi
  const uint32_t step = blockDim.x * 8;
  uint32_t j0 = lo + threadIdx.x * 8;
  uint4 pk = make_uint4(0u, 0u, 0u, 0u);
  // sign bits of the 8 scalars: they may straddle two 64-bit words when inst*n is not a multiple of 8
  unsigned long long m0 = 0ull, m1 = 0ull;
  if (j0 < hi) {
    pk = *reinterpret_cast<const uint4 *>(d + j0);
    m0 = negmask[(inst0 + j0) >> 6]; m1 = negmask[(inst0 + j0 + 7) >> 6];
  }
  while (j0 < hi) {
    const uint32_t jn = j0 + step;
    uint4 pkn = pk;
    unsigned long long m0n = m0, m1n = m1;
    if (jn < hi) {
      pkn = *reinterpret_cast<const uint4 *>(d + jn);
      m0n = negmask[(inst0 + jn) >> 6]; m1n = negmask[(inst0 + jn + 7) >> 6];
    }
    uint32_t w[4] = {pk.x, pk.y, pk.z, pk.w};
    const uint64_t flat0 = inst0 + j0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      int v = (int)((w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu) - M;
      if (j0 + k < hi && v) {
        uint32_t mb = (v < 0 ? -v : v) - 1;
        uint64_t flat = flat0 + k;
        unsigned long long mw = ((flat >> 6) == (flat0 >> 6)) ? m0 : m1;
        uint32_t sneg = (uint32_t)((mw >> (flat & 63)) & 1ull);
        uint32_t sg = (v < 0 ? 1u : 0u) ^ sneg ^ flip;
        uint32_t pos = atomicAdd(&lh[mb], 1u);
        sorted[pos] = (sg << 31) | (idx_base + j0 + k);   // 4 bytes: the bucket is implied by start[] (position -> bucket), not stored
      }
    }
    pk = pkn; m0 = m0n; m1 = m1n; j0 = jn;
  }
}

// The scatter of ONE MSM with wide windows (M * 4 > 80 KiB; make_plan, MsmPlan::Q), by bucket range, in the form for chunks of ANY length;
// a plan whose chunks fit a lane's registers takes k_scatter_one_read below instead (MsmPlan::one_read).  k_scatter's stores are its whole cost:
// a bucket's ~n / M entries (one 128-byte line at 2^20 terms) arrive from CH workgroups that sit on all 8 XCDs, so every 4-byte store leaves an
// L2 as a request of its own.  Here a workgroup is (window w, range q of Q, chunk ch): it reads its chunk of the window's digit row as
// k_scatter does, keeps only the cursors of the M / Q buckets of its range in LDS and places only their entries, at the positions k_scatter
// would use (the order inside a (bucket, chunk) may differ).  The 1-D grid puts the chunks of one (w, q) unit on blocks b = s (mod 8), the
// observed XCD affinity: an XCD works through its units one after another and the unit's slice of `sorted` (n * 4 / Q bytes) can stay in its
// 4-MiB L2 until the lines are full.  That is placement for speed only — any dispatch order and any block -> XCD map give the same `sorted`
// positions; no workgroup waits for another.  The digit row is read Q times, once per range (non-temporal: it should not push the output lines
// out): a quarter of this launch's traffic at Q = 4, which is what k_scatter_one_read saves where the chunk is short enough.
// ONE workgroup per CU (the launch asks for more than half of a CU's LDS, ranges_lds_bytes): a unit's chunks then fill the XCD and one unit is live per
// L2.  With two workgroups per CU (64 VGPRs allow it) two units are live, the lines leave the L2 half full (WRITE_SIZE 109 -> 215 MB at 2^20
// terms) and the kernel is slower, loads ahead or not.  So the latency of a workgroup's chain is hidden inside the lane instead:
// the digits and sign bytes of its first SCATTER_AHEAD steps are requested BEFORE the cursors, all cursor loads before the first LDS write, and
// a step's registers are refilled with the step SCATTER_AHEAD further on as soon as its entries are placed.  The test j < hi that guarded the
// single load per step now selects the ADDRESS: a lane whose step lies past the chunk's end reads the first 16 bytes of the row (and mask byte 0),
// which every row has, and drops them.  A load under a branch would do, but its result then meets the other path's value in a register copy, and
// the compiler waits for the load right there.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// The three steps that k_scatter_ranges and k_scatter_one_read share (SCATTER_AHEAD: msm_plan.hpp).
// Prefetch: the digit packs and sign bytes of the lane's steps j0, j0 + step, ... of the row d; a step past the chunk's end reads the row's
// first 16 bytes (and mask byte 0), dropped at the placement.
BPPP_DI void scatter_prefetch(const uint16_t *__restrict__ d, const uint8_t *__restrict__ sgn, uint32_t j0, uint32_t step, uint32_t hi,
                              u32x4 (&pk)[SCATTER_AHEAD], uint32_t (&sneg8)[SCATTER_AHEAD]) {
#pragma unroll
  for (int i = 0; i < SCATTER_AHEAD; i++) {
    const uint32_t j = j0 + (uint32_t)i * step, ja = j < hi ? j : 0u;
    pk[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(d + ja)); sneg8[i] = sgn[ja >> 3];
  }
}
// Cursors of the buckets [r0, r0 + count) of a (window, chunk) into lh[0, count): bh_row and st_row are the chunk's histogram row and the
// window's start row.  Four buckets per load (r0 and count are multiples of 4 and the arrays 16-byte aligned), four pairs of loads per lane
// and round of the loop, all in flight before the first sum is written to LDS.
BPPP_DI void scatter_load_cursors(const uint32_t *__restrict__ bh_row, const uint32_t *__restrict__ st_row, uint32_t r0, uint32_t count, uint32_t *lh) {
  const uint4 *bh = reinterpret_cast<const uint4 *>(bh_row + r0);
  const uint4 *st = reinterpret_cast<const uint4 *>(st_row + r0);
  const uint32_t nq = count >> 2;
  for (uint32_t t0 = threadIdx.x; t0 < nq; t0 += 4 * blockDim.x) {
    uint4 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t t = t0 + i * blockDim.x;
      a[i] = b[i] = make_uint4(0u, 0u, 0u, 0u);
      if (t < nq) { a[i] = st[t]; b[i] = bh[t]; }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t t = t0 + i * blockDim.x;
      if (t < nq) { lh[4 * t] = a[i].x + b[i].x; lh[4 * t + 1] = a[i].y + b[i].y; lh[4 * t + 2] = a[i].z + b[i].z; lh[4 * t + 3] = a[i].w + b[i].w; }
    }
  }
}
// The cursors from the 16-bit prefixes of k_count_tiles16 (MsmPlan::hist16).  bh_row is the row of chunk ch of the window's CH rows of M values,
// so chunk k's is bh_row - (ch - k) * M.  Eight buckets per 16-byte load of prefixes (r0 and count are multiples of 8), beside two loads of their
// starts and the one start after them; a cursor is start[b] + the stored prefix.  A bucket of 65536 entries or more (start[b + 1] - start[b]) has
// prefixes that wrapped.  Every chunk adds fewer than 65536 entries to it, so a stored prefix is below the one of the chunk before exactly when
// it wrapped once more: the lane walks the bucket's stored values of chunks 1 .. ch (chunk 0 stores 0) and adds 65536 per decrease.  With
// evenly spread digits no bucket is that large; n equal scalars have one per window.
BPPP_DI uint32_t scatter_wraps(const uint16_t *__restrict__ at, uint32_t ch, uint32_t M) {
  const uint16_t *p = at - (size_t)ch * M;
  uint32_t wraps = 0, prev = 0;
  for (uint32_t k = 1; k <= ch; k++) { const uint32_t v = p[(size_t)k * M]; wraps += v < prev ? 1u : 0u; prev = v; }
  return wraps;
}
BPPP_DI void scatter_load_cursors16(const uint16_t *__restrict__ bh_row, uint32_t ch, uint32_t M, const uint32_t *__restrict__ st_row, uint32_t r0, uint32_t count,
                                    uint32_t *lh) {
  const uint4 *bh = reinterpret_cast<const uint4 *>(bh_row + r0);
  const uint4 *st = reinterpret_cast<const uint4 *>(st_row + r0);
  uint4 *lh4 = reinterpret_cast<uint4 *>(lh);
  const uint32_t no = count >> 3;
  for (uint32_t t0 = threadIdx.x; t0 < no; t0 += 4 * blockDim.x) {
    uint4 a0[4], a1[4], b[4];
    uint32_t a2[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t t = t0 + i * blockDim.x;
      a0[i] = a1[i] = b[i] = make_uint4(0u, 0u, 0u, 0u); a2[i] = 0u;
      if (t < no) { a0[i] = st[2 * t]; a1[i] = st[2 * t + 1]; a2[i] = st_row[r0 + 8 * t + 8]; b[i] = bh[t]; }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t t = t0 + i * blockDim.x;
      if (t < no) {
        const uint32_t s[9] = {a0[i].x, a0[i].y, a0[i].z, a0[i].w, a1[i].x, a1[i].y, a1[i].z, a1[i].w, a2[i]};
        uint32_t pre[8] = {b[i].x & 0xFFFFu, b[i].x >> 16, b[i].y & 0xFFFFu, b[i].y >> 16, b[i].z & 0xFFFFu, b[i].z >> 16, b[i].w & 0xFFFFu, b[i].w >> 16};
#pragma unroll
        for (int k = 0; k < 8; k++)
          if (s[k + 1] - s[k] >= 65536u) pre[k] += scatter_wraps(bh_row + r0 + 8 * t + k, ch, M) << 16;
        lh4[2 * t] = make_uint4(s[0] + pre[0], s[1] + pre[1], s[2] + pre[2], s[3] + pre[3]);
        lh4[2 * t + 1] = make_uint4(s[4] + pre[4], s[5] + pre[5], s[6] + pre[6], s[7] + pre[7]);
      }
    }
  }
}
// Placement: the entries of the pack of step j (digits pkv, sign byte sn) whose bucket lies in [r0, r0 + Mq); lh[b - b0] is bucket b's cursor
// (b0 = r0 where LDS holds the range alone, 0 where it holds the window).
BPPP_DI void scatter_place(const u32x4 pkv, uint32_t sn, uint32_t j, uint32_t hi, uint32_t M, uint32_t r0, uint32_t Mq, uint32_t flip, uint32_t *lh, uint32_t b0,
                           uint32_t *__restrict__ sorted) {
  const uint32_t w[4] = {pkv.x, pkv.y, pkv.z, pkv.w};
#pragma unroll
  for (int e = 0; e < 8; e++) {
    int v = (int)((w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu) - (int)M;
    uint32_t mb = (uint32_t)(v < 0 ? -v : v) - 1u;            // v == 0: wraps past every range
    if (j + e < hi && v && mb - r0 < Mq) {
      uint32_t sg = (v < 0 ? 1u : 0u) ^ ((sn >> e) & 1u) ^ flip;
      uint32_t pos = atomicAdd(&lh[mb - b0], 1u);
      sorted[pos] = (sg << 31) | (j + e);
    }
  }
}
__global__ void __launch_bounds__(1024) k_scatter_ranges(const uint16_t *__restrict__ dig, const unsigned long long *__restrict__ negmask, uint32_t n,
                                                         uint32_t stride, int c, int CH, int Q, uint32_t U, int top,
                                                         const uint32_t *__restrict__ blockhist, const uint32_t *__restrict__ start,
                                                         uint32_t *__restrict__ sorted, int h16) {
  extern __shared__ uint32_t lh[];
  const uint32_t M = 1u << (c - 1), Mq = M / (uint32_t)Q;
  const uint32_t s = blockIdx.x & 7u, k = blockIdx.x >> 3, u = (k / (uint32_t)CH) * 8u + s, ch = k % (uint32_t)CH;
  if (u >= U) return;                                       // the grid is padded to 8 slots x whole units
  const uint32_t nbw = u / (uint32_t)Q, r0 = (u % (uint32_t)Q) * Mq;
  const uint32_t flip = (int)nbw == top ? 1u : 0u;          // row `top` holds its digits negated (k_digits)
  uint32_t per = (((n + CH - 1) / CH) + 7u) & ~7u, lo = ch * per, hi = min(n, lo + per);
  const uint16_t *d = dig + (size_t)nbw * stride;
  // one instance and j a multiple of 8: the sign bits of a step's 8 scalars are ONE BYTE of negmask (bit j of the mask is bit j & 7 of
  // byte j >> 3: the words are little-endian)
  const uint8_t *sgn = reinterpret_cast<const uint8_t *>(negmask);
  const uint32_t step = blockDim.x * 8;
  uint32_t j0 = lo + threadIdx.x * 8;
  u32x4 pk[SCATTER_AHEAD];
  uint32_t sneg8[SCATTER_AHEAD];
  scatter_prefetch(d, sgn, j0, step, hi, pk, sneg8);
  // cursors of the range (M = 2^15, Q <= 4: r0 and Mq are multiples of 4): all of a lane's loads (Mq / 4096 pairs, two at Q = 4) are in
  // flight before the first sum is written to LDS; h16 (MsmPlan::hist16): from 16-bit prefixes, eight buckets per load
  if (h16) scatter_load_cursors16(reinterpret_cast<const uint16_t *>(blockhist) + ((size_t)nbw * CH + ch) * M, ch, M, start + (size_t)nbw * M, r0, Mq, lh);
  else scatter_load_cursors(blockhist + ((size_t)nbw * CH + ch) * M, start + (size_t)nbw * M, r0, Mq, lh);
  __syncthreads();
  for (; j0 < hi; j0 += SCATTER_AHEAD * step) {
#pragma unroll
    for (int i = 0; i < SCATTER_AHEAD; i++) {
      const uint32_t j = j0 + (uint32_t)i * step;
      if (j < hi) {
        const u32x4 pkv = pk[i];
        const uint32_t sn = sneg8[i];
        const uint32_t jn = j + SCATTER_AHEAD * step, ja = jn < hi ? jn : 0u;
        pk[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(d + ja)); sneg8[i] = sgn[ja >> 3];
        scatter_place(pkv, sn, j, hi, M, r0, Mq, flip, lh, r0, sorted);
      }
    }
  }
}

// The ranged scatter with a chunk's digits read ONCE (make_plan, MsmPlan::one_read: every chunk fits the SCATTER_AHEAD steps a lane holds in
// registers).  A workgroup is (window w, chunk ch): it requests its digit packs and sign bytes as k_scatter_ranges does, before the cursors,
// loads the cursors of all M buckets into LDS (M * 4 bytes, 128 KiB: one workgroup per CU, as k_scatter), and after ONE barrier places range 0,
// then range 1, ... from the same registers, each pass taking only the entries whose bucket lies in its range.  The (window, range) -> XCD
// placement of k_scatter_ranges is kept in time instead of in space: the 1-D grid puts the CH chunks of a window on blocks b = s (mod 8), so
// an XCD works through its windows one after another, its workgroups walk the ranges together and the live slice of `sorted` per L2 is one
// range of one window (n * 4 / Q bytes).  Placement for speed only: every entry lands where k_scatter puts it (the order inside a (bucket,
// chunk) may differ), whatever the dispatch order; no workgroup waits for another.  The barrier after every pass is for speed too: it keeps
// the 16 wavefronts of a workgroup, and with them the 32 workgroups of an XCD, on one range.  Without it they drift apart, all Q slices are
// live at once and the lines leave the L2 a fraction full (WRITE_SIZE 66 -> 405 MB at 2^20 terms, sort stage 0.163 -> 0.183 ms).
__global__ void __launch_bounds__(1024) k_scatter_one_read(const uint16_t *__restrict__ dig, const unsigned long long *__restrict__ negmask, uint32_t n,
                                                           uint32_t stride, int c, int CH, int Q, uint32_t W, int top,
                                                           const uint32_t *__restrict__ blockhist, const uint32_t *__restrict__ start,
                                                           uint32_t *__restrict__ sorted, int h16) {
  extern __shared__ uint32_t lh[];
  const uint32_t M = 1u << (c - 1);
  const uint32_t s = blockIdx.x & 7u, k = blockIdx.x >> 3, nbw = (k / (uint32_t)CH) * 8u + s, ch = k % (uint32_t)CH;
  if (nbw >= W) return;                                     // the grid is padded to 8 slots x whole windows
  const uint32_t flip = (int)nbw == top ? 1u : 0u;          // row `top` holds its digits negated (k_digits)
  uint32_t per = (((n + CH - 1) / CH) + 7u) & ~7u, lo = ch * per, hi = min(n, lo + per);
  const uint16_t *d = dig + (size_t)nbw * stride;
  const uint8_t *sgn = reinterpret_cast<const uint8_t *>(negmask);   // one byte per step (k_scatter_ranges)
  const uint32_t step = blockDim.x * 8, j0 = lo + threadIdx.x * 8;
  u32x4 pk[SCATTER_AHEAD];
  uint32_t sneg8[SCATTER_AHEAD];
  scatter_prefetch(d, sgn, j0, step, hi, pk, sneg8);
  // cursors of the whole window (M is a multiple of 8), from 32-bit or (h16, MsmPlan::hist16) 16-bit prefixes
  if (h16) scatter_load_cursors16(reinterpret_cast<const uint16_t *>(blockhist) + ((size_t)nbw * CH + ch) * M, ch, M, start + (size_t)nbw * M, 0u, M, lh);
  else scatter_load_cursors(blockhist + ((size_t)nbw * CH + ch) * M, start + (size_t)nbw * M, 0u, M, lh);
  __syncthreads();
  const uint32_t Mq = M / (uint32_t)Q;
  for (uint32_t r0 = 0; r0 < M; r0 += Mq) {
#pragma unroll
    for (int i = 0; i < SCATTER_AHEAD; i++) {
      const uint32_t j = j0 + (uint32_t)i * step;
      if (j < hi) scatter_place(pk[i], sneg8[i], j, hi, M, r0, Mq, flip, lh, 0u, sorted);
    }
    __syncthreads();                                        // the workgroup's wavefronts move to the next range together (see above)
  }
}

// ------------------------------------------------------------------------------------------------
// 3. load-balanced accumulation
// Lane g owns sorted positions [g*L, (g+1)*L).  A bucket b = [start[b], start[b]+count[b]) that lies
// inside one lane is summed and stored there.  A bucket spanning lanes g0 < g1 leaves partial sums:
//   lane g0 (run starts inside the lane)      -> tail slot 2*g0+1
//   lanes g0 < g <= g1 (run continues from g-1) -> head slot 2*g
// which k_merge (one lane per bucket, short spans) or k_merge_heavy (one wavefront per bucket)
// add up.  Slots are addressed from start/count alone: no keys are stored, no compaction needed.
__global__ void __launch_bounds__(256) k_acc_points(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ start, uint32_t FB,
                                                    const uint32_t *__restrict__ points, uint32_t n, uint32_t WM, int shared_pts,
                                                    int L, uint64_t G, uint32_t *__restrict__ buckets, uint32_t *__restrict__ rec_pt) {
  uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const uint32_t total = start[FB];
  const uint64_t pos0 = g * (uint64_t)L;
  if (pos0 >= total) return;
  const uint32_t pos1 = (uint32_t)min((uint64_t)total, pos0 + L);
  // the bucket that holds position pos0: the largest fb with start[fb] <= pos0 (it is non-empty: start[fb + 1] > pos0)
  uint32_t lo = 0, hi = FB - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (start[mid] <= (uint32_t)pos0) lo = mid; else hi = mid - 1;
  }
  uint32_t cur = lo, end = start[cur + 1];
  const bool from_prev = start[cur] < (uint32_t)pos0;         // the first run continues one that began in an earlier lane
  bool first = true;
  uint32_t e = sorted[pos0];
  xyzz acc = xyzz_inf();
  for (uint32_t p = (uint32_t)pos0; p < pos1; p++) {
    const uint32_t e_next = (p + 1 < pos1) ? sorted[p + 1] : 0u;
    if (p == end) {
      // the finished run ends inside this lane: head partial if it came from the previous lane, else complete
      if (first && from_prev) xyzz_store(rec_pt + (2 * g) * XYZZ_WORDS, acc);
      else xyzz_store(buckets + (size_t)cur * XYZZ_WORDS, acc);
      first = false; acc = xyzz_inf();
      cur++; end = start[cur + 1];
      if (end <= p) {                                         // an empty bucket — there may be thousands in a row (the unused half of a narrow
        uint32_t lo2 = cur + 1, hi2 = FB - 1;                 // window, an empty carry window): bisect for the bucket that holds p
        while (lo2 < hi2) {
          const uint32_t mid = lo2 + (hi2 - lo2 + 1) / 2;
          if (start[mid] <= p) lo2 = mid; else hi2 = mid - 1;
        }
        cur = lo2; end = start[cur + 1];
      }
    }
    const uint32_t idx = e & 0x7FFFFFFFu;
    const bool sg = (e >> 31) & 1u;
    // shared_pts: 1 = one point array for every instance, 0 = one per instance, d >= 2 = one per d consecutive instances
    size_t pidx = shared_pts == 1 ? (size_t)idx : (size_t)((cur / WM) / (shared_pts ? shared_pts : 1)) * n + idx;
    aff P = aff_cneg(aff_load(points + pidx * 16), sg);
    xyzz_madd(acc, P);
    e = e_next;
  }
  const bool hi_part = first && from_prev, ti = end > pos1;   // the last run goes on in the next lane
  if (hi_part) xyzz_store(rec_pt + (2 * g) * XYZZ_WORDS, acc);
  else if (ti) xyzz_store(rec_pt + (2 * g + 1) * XYZZ_WORDS, acc);
  else xyzz_store(buckets + (size_t)cur * XYZZ_WORDS, acc);
}

// partial t of a bucket whose first lane is g0: t = 0 is g0's tail slot, t >= 1 the head slot of lane g0+t
BPPP_DI const uint32_t *partial_ptr(const uint32_t *rec_pt, uint64_t g0, uint64_t t) {
  return rec_pt + (t == 0 ? 2 * g0 + 1 : 2 * (g0 + t)) * XYZZ_WORDS;
}
// hand bucket fb with np partial sums to k_merge_heavy, HEAVY_CHUNK partials per wavefront: its (bucket, chunk) items are drawn from ctr[0]
// and, when there are several, the bucket gets an entry of heavy_buckets (drawn from ctr[1]) on which the chunks draw their tickets
BPPP_DI void heavy_register(uint32_t fb, uint32_t np, uint2 *heavy_items, uint32_t *heavy_slot, uint4 *heavy_buckets, uint32_t *ctr) {
  const uint32_t nch = (np + HEAVY_CHUNK - 1) / HEAVY_CHUNK;
  uint32_t base = atomicAdd(&ctr[0], nch), hb = 0;
  if (nch > 1) { hb = atomicAdd(&ctr[1], 1u); heavy_buckets[hb] = make_uint4(fb, base, nch, 0u); }   // .w: the chunks' ticket
  for (uint32_t j = 0; j < nch; j++) { heavy_items[base + j] = make_uint2(fb, j); heavy_slot[base + j] = hb; }
}

__global__ void __launch_bounds__(256) k_merge(const uint32_t *__restrict__ start, const uint32_t *__restrict__ count, uint64_t FB, int L,
                                               const uint32_t *__restrict__ rec_pt, uint32_t *__restrict__ buckets,
                                               uint2 *__restrict__ heavy_items, uint32_t *__restrict__ heavy_slot, uint4 *__restrict__ heavy_buckets,
                                               uint32_t *__restrict__ heavy_count) {
  uint64_t fb = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (fb >= FB) return;
  uint32_t cnt = count[fb];
  // the bucket array is not cleared between calls: an empty bucket is marked here, every other one is written by k_acc_points, below
  // or by k_merge_heavy before a reduction reads it
  if (!cnt) { xyzz_store(buckets + fb * XYZZ_WORDS, xyzz_inf()); return; }
  uint32_t s = start[fb];
  uint64_t g0 = s / (uint32_t)L, g1 = (uint64_t)(s + cnt - 1) / (uint32_t)L;
  if (g0 == g1) return;                       // summed and stored by its lane
  uint32_t np = (uint32_t)(g1 - g0 + 1);      // number of partial sums
  if (np > MERGE_SERIAL_MAX + 1) {
    // skewed scalars / a narrow top window: hand the bucket to wavefronts
    heavy_register((uint32_t)fb, np, heavy_items, heavy_slot, heavy_buckets, heavy_count);
    return;
  }
  xyzz acc = xyzz_load(partial_ptr(rec_pt, g0, 0));
  for (uint32_t t = 1; t < np; t++) {
    xyzz p = xyzz_load(partial_ptr(rec_pt, g0, t));
    xyzz_add(acc, p);
  }
  xyzz_store(buckets + fb * XYZZ_WORDS, acc);
}

// one wavefront per (heavy bucket, chunk): lanes stride over the chunk's partials, then a shuffle tree.  A bucket of more than one chunk
// collects its chunk sums in chunk_sums; each chunk draws a ticket on the bucket's heavy_buckets entry (.w, zero from k_merge) and the
// wavefront that arrives last adds them up.  Launched as 2048 single-wavefront workgroups, and the shape matters beyond this kernel:
// with 512 workgroups of four wavefronts in its place the k_reduce_marg launch that follows (69 632 single-wavefront workgroups at 2^20
// terms) ran 0.216 ms instead of 0.158 (measured both ways, same data).
// SIZED (the join of k_acc_points_sized's pieces, section 3'): the partials of bucket fb are its ceil(count / ACC_CAP) piece sums, consecutive in
// rec_pt from slot piece_base[fb] on.
template <bool SIZED>
__global__ void __launch_bounds__(64) k_merge_heavy(const uint32_t *__restrict__ start, const uint32_t *__restrict__ count, int L,
                                                     const uint32_t *__restrict__ rec_pt, const uint32_t *__restrict__ piece_base, uint32_t *__restrict__ buckets,
                                                     const uint2 *__restrict__ heavy_items, const uint32_t *__restrict__ heavy_slot, uint4 *heavy_buckets,
                                                     const uint32_t *__restrict__ heavy_count, uint32_t *chunk_sums) {
  const uint32_t nitems = heavy_count[0], lane = threadIdx.x;
  for (uint32_t h = blockIdx.x; h < nitems; h += gridDim.x) {
    uint2 it = heavy_items[h];
    uint32_t fb = it.x, cnt = count[fb], np;
    uint64_t g0 = 0;
    const uint32_t *pieces = nullptr;
    if (SIZED) { np = (cnt + ACC_CAP - 1) / ACC_CAP; pieces = rec_pt + (size_t)piece_base[fb] * XYZZ_WORDS; }
    else {
      const uint32_t s = start[fb];
      g0 = s / (uint32_t)L;
      np = (uint32_t)((uint64_t)(s + cnt - 1) / (uint32_t)L - g0 + 1);
    }
    uint32_t t0 = it.y * HEAVY_CHUNK, t1 = min(np, t0 + HEAVY_CHUNK);
    xyzz acc = xyzz_inf();
    for (uint32_t t = t0 + lane; t < t1; t += 64) {
      xyzz p = xyzz_load(SIZED ? pieces + (size_t)t * XYZZ_WORDS : partial_ptr(rec_pt, g0, t));
      xyzz_add_chain(acc, p);
    }
    for (int d = 32; d >= 1; d >>= 1) {
      xyzz o = xyzz_shfl_down(acc, d);
      if ((int)lane + d < 64) xyzz_add_chain(acc, o);
    }
    if (np <= HEAVY_CHUNK) {
      if (lane == 0) xyzz_store(buckets + (size_t)fb * XYZZ_WORDS, acc);
      continue;
    }
    // more than one chunk: publish this chunk's sum (agent-scope release before the ticket), the last arriver acquires and adds them
    const uint32_t nch = (np + HEAVY_CHUNK - 1) / HEAVY_CHUNK;
    uint32_t last = 0;
    if (lane == 0) {
      xyzz_store(chunk_sums + (size_t)h * XYZZ_WORDS, acc);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      last = __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(heavy_buckets + heavy_slot[h]) + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nch - 1;
    }
    last = (uint32_t)__shfl((int)last, 0, 64);
    if (!last) continue;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t base = h - it.y;                        // the bucket's chunks are consecutive items
    acc = xyzz_inf();
    for (uint32_t j = lane; j < nch; j += 64) {
      xyzz p = xyzz_load(chunk_sums + (size_t)(base + j) * XYZZ_WORDS);
      xyzz_add_chain(acc, p);
    }
    for (int d = 32; d >= 1; d >>= 1) {
      xyzz o = xyzz_shfl_down(acc, d);
      if ((int)lane + d < 64) xyzz_add_chain(acc, o);
    }
    if (lane == 0) xyzz_store(buckets + (size_t)fb * XYZZ_WORDS, acc);
  }
}

// ------------------------------------------------------------------------------------------------
// 3'. accumulation by whole buckets, ordered by size (one MSM over arbitrary points; MsmTune::acc_sized)
// The slices of section 3 cross a bucket boundary in nearly every iteration of some lane of a wavefront (store, clear, next bucket: executed by
// all under divergence), spend a whole addition slot on the copy that starts each run and leave half of the buckets in two partial sums.
// Here a lane takes one ITEM (k_count_tiles) and the items are dispatched in descending order of size, so the lanes of a wavefront run the
// same number of additions: the loop has no boundary, the first entry is loaded into the accumulator (one addition less per item), and a
// bucket that is one item — every bucket unless the scalars are skewed — is stored once and finished.
//
// k_order, one workgroup per tile of SCAN_TILE buckets (16 per lane): every workgroup derives the class offsets (largest size first) from the
// size histogram, counts its own items per class in LDS, draws its share of each class with one global atomic (cursors, laid out like the
// histogram, zero at launch: k_digits) and writes items[] = (bucket, piece).  The order inside a class is arbitrary: the sums are group
// elements.  It also marks the empty buckets (the bucket array is not cleared between calls) and lists the buckets of several pieces for
// k_merge_heavy<true>, which adds their piece sums: the pieces' slots (piece_base[bucket], drawn from ctr[2]) and the (bucket, chunk) items
// of that kernel.  ctr[3]: the number of items.
__global__ void __launch_bounds__(256) k_order(const uint32_t *__restrict__ count, uint64_t FB, const uint32_t *__restrict__ size_hist,
                                               uint32_t *__restrict__ cursors, uint2 *__restrict__ items, uint32_t *__restrict__ piece_base,
                                               uint32_t *__restrict__ buckets, uint2 *__restrict__ heavy_items, uint32_t *__restrict__ heavy_slot,
                                               uint4 *__restrict__ heavy_buckets, uint32_t *__restrict__ ctr) {
  __shared__ uint32_t off[ACC_CAP], lc[ACC_CAP], lb[ACC_CAP];
  const uint32_t t = threadIdx.x;
  if (t < ACC_CAP) { lc[t] = 0; lb[t] = size_hist[t * ACC_LINE]; }
  __syncthreads();
  if (t < ACC_CAP) {
    uint32_t s = 0;
    for (uint32_t u = t + 1; u < ACC_CAP; u++) s += lb[u];
    off[t] = s;                                               // items of a larger size
    if (t == 0 && blockIdx.x == 0) ctr[3] = s + lb[0];
  }
  const uint64_t fb0 = (uint64_t)blockIdx.x * SCAN_TILE + t;
  uint32_t cnt[16], rr[16], rf[16];                           // the ranks of the bucket's short item (bin rem - 1) and of its full pieces (the last bin)
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint64_t fb = fb0 + (uint64_t)k * 256;
    cnt[k] = fb < FB ? count[fb] : 0u;
    rr[k] = cnt[k] % ACC_CAP ? atomicAdd(&lc[cnt[k] % ACC_CAP - 1], 1u) : 0u;
    rf[k] = cnt[k] >= ACC_CAP ? atomicAdd(&lc[ACC_CAP - 1], cnt[k] / ACC_CAP) : 0u;
  }
  __syncthreads();                                            // lc complete, lb read by all
  if (t < ACC_CAP) lb[t] = lc[t] ? atomicAdd(cursors + t * ACC_LINE, lc[t]) : 0u;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint64_t fb = fb0 + (uint64_t)k * 256;
    if (fb >= FB) continue;
    const uint32_t full = cnt[k] / ACC_CAP, rem = cnt[k] % ACC_CAP;
    if (!cnt[k]) { xyzz_store(buckets + fb * XYZZ_WORDS, xyzz_inf()); continue; }
    for (uint32_t j = 0; j < full; j++) items[off[ACC_CAP - 1] + lb[ACC_CAP - 1] + rf[k] + j] = make_uint2((uint32_t)fb, j);
    if (rem) items[off[rem - 1] + lb[rem - 1] + rr[k]] = make_uint2((uint32_t)fb, full);
    if (cnt[k] <= ACC_CAP) continue;
    const uint32_t np = full + (rem ? 1u : 0u);
    piece_base[fb] = atomicAdd(&ctr[2], np);
    heavy_register((uint32_t)fb, np, heavy_items, heavy_slot, heavy_buckets, ctr);
  }
}

// The point arithmetic of the sized accumulation: the entry's point with its sign folded in, the accumulator started from it, the mixed
// addition, and the sum in the 40-word layout that k_merge_heavy<true> and the bucket reduction read.
struct AccFq26 {                                   // 10 x 26-bit limbs (ec.hip.h)
  typedef aff point; typedef xyzz sum;
  static BPPP_DI aff load(const uint32_t *p) { return aff_load(p); }
  static BPPP_DI aff cneg(const aff &P, bool neg) { return aff_cneg(P, neg); }
  static BPPP_DI xyzz first(const aff &P) { return xyzz_from_aff(P); }
  static BPPP_DI void madd(xyzz &acc, const aff &P) { xyzz_madd(acc, P); }
  static BPPP_DI xyzz stored(const xyzz &acc) { return acc; }
};
// 9 x 29-bit limbs (fq29.hip.h, ec29.hip.h; MsmTune::acc_fq29): 81 partial products per field multiplication instead of 100.  The sum is
// converted once, at the store (every limb below 2^26).
struct AccFq29 {
  typedef aff29 point; typedef xyzz29 sum;
  static BPPP_DI aff29 load(const uint32_t *p) { return aff29_load(p); }
  static BPPP_DI aff29 cneg(const aff29 &P, bool neg) { return aff29_cneg(P, neg); }
  static BPPP_DI xyzz29 first(const aff29 &P) { return xyzz29_from_aff(P); }
  static BPPP_DI void madd(xyzz29 &acc, const aff29 &P) { xyzz29_madd(acc, P); }
  static BPPP_DI xyzz stored(const xyzz29 &acc) { return xyzz29_to_xyzz(acc); }
};
// one item per lane: the same 4-byte entries, sign fold and complete mixed addition as k_acc_points.  A lane whose item is shorter than the
// wavefront's longest leaves the loop early (execution mask); a whole bucket goes to `buckets`, a piece to its slot of `pieces`.
template <class A>
BPPP_DI void acc_points_sized(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ start, const uint32_t *__restrict__ count,
                              const uint2 *__restrict__ items, const uint32_t *__restrict__ ctr, const uint32_t *__restrict__ piece_base,
                              const uint32_t *__restrict__ points, uint32_t *__restrict__ buckets, uint32_t *__restrict__ pieces) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= ctr[3]) return;
  const uint2 it = items[g];
  const uint32_t fb = it.x, cnt = count[fb], first = it.y * ACC_CAP, len = min(ACC_CAP, cnt - first);
  const uint32_t *ent = sorted + start[fb] + first;
  uint32_t e = ent[0];
  typename A::sum acc = A::first(A::cneg(A::load(points + (size_t)(e & 0x7FFFFFFFu) * 16), (e >> 31) & 1u));
  e = len > 1 ? ent[1] : 0u;
  for (uint32_t k = 1; k < len; k++) {
    const uint32_t e_next = (k + 1 < len) ? ent[k + 1] : 0u;
    typename A::point P = A::cneg(A::load(points + (size_t)(e & 0x7FFFFFFFu) * 16), (e >> 31) & 1u);
    A::madd(acc, P);
    e = e_next;
  }
  xyzz_store(cnt > ACC_CAP ? pieces + ((size_t)piece_base[fb] + it.y) * XYZZ_WORDS : buckets + (size_t)fb * XYZZ_WORDS, A::stored(acc));
}
__global__ void __launch_bounds__(256) k_acc_points_sized(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ start,
                                                          const uint32_t *__restrict__ count, const uint2 *__restrict__ items,
                                                          const uint32_t *__restrict__ ctr, const uint32_t *__restrict__ piece_base,
                                                          const uint32_t *__restrict__ points, uint32_t *__restrict__ buckets,
                                                          uint32_t *__restrict__ pieces) {
  acc_points_sized<AccFq26>(sorted, start, count, items, ctr, piece_base, points, buckets, pieces);
}
__global__ void __launch_bounds__(256) k_acc_points_sized29(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ start,
                                                            const uint32_t *__restrict__ count, const uint2 *__restrict__ items,
                                                            const uint32_t *__restrict__ ctr, const uint32_t *__restrict__ piece_base,
                                                            const uint32_t *__restrict__ points, uint32_t *__restrict__ buckets,
                                                            uint32_t *__restrict__ pieces) {
  acc_points_sized<AccFq29>(sorted, start, count, items, ctr, piece_base, points, buckets, pieces);
}

// k_acc_points_sized29 without the exception tests of the mixed addition (MsmTune::acc_fast; DESIGN.md 0.2, "exception-free mixed addition").
// An item starts as affine + affine (xyzz29_from_two) and goes on with xyzz29_madd_fast; neither tests anything; P = Q or P = -Q against the running sum leaves ZZ = 0 (mod p) to the end of
// the item (ec29.hip.h), so one zero test of ZZ per item finds every such item, and its lane redoes it from the first entry with the complete
// loop, after the fast one.  Input points at infinity (0, 0) are skipped before they reach the formula; the sum starts from the first finite
// entry, and an item with no finite entry stores infinity.
BPPP_DI void acc_item_complete29(const uint32_t *__restrict__ ent, uint32_t len, const uint32_t *__restrict__ points, uint32_t *__restrict__ dst) {
  uint32_t e = ent[0];
  xyzz29 acc = xyzz29_from_aff(aff29_cneg(aff29_load(points + (size_t)(e & 0x7FFFFFFFu) * 16), (e >> 31) & 1u));
  for (uint32_t k = 1; k < len; k++) {
    e = ent[k];
    xyzz29_madd(acc, aff29_cneg(aff29_load(points + (size_t)(e & 0x7FFFFFFFu) * 16), (e >> 31) & 1u));
  }
  xyzz_store(dst, xyzz29_to_xyzz(acc));
}
// the next finite point of ent[k .. len) with its sign folded in, k left behind it; false when there is none
BPPP_DI bool acc_next_finite(const uint32_t *__restrict__ ent, uint32_t &k, uint32_t len, const uint32_t *__restrict__ points, aff29 &P) {
  bool finite = false;
  while (k < len && !finite) {
    const uint32_t e = ent[k++];
    P = aff29_load_finite(points + (size_t)(e & 0x7FFFFFFFu) * 16, (e >> 31) & 1u, finite);
  }
  return finite;
}
// The redo is inline, after the fast loop, and not a __noinline__ function: as a callee its 184 VGPRs became the kernel's and left two
// wavefronts per SIMD.  The fast loop itself does not carry the complete addition (no spill; profiles/r15_acc_fast_isa_histogram.txt); the
// attribute keeps four wavefronts per SIMD as in k_acc_points_sized29, where the compiler left to itself takes over 128 VGPRs and three.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_acc_points_sized29_fast(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ start, const uint32_t *__restrict__ count,
                          const uint2 *__restrict__ items, const uint32_t *__restrict__ ctr, const uint32_t *__restrict__ piece_base,
                          const uint32_t *__restrict__ points, uint32_t *__restrict__ buckets, uint32_t *__restrict__ pieces) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= ctr[3]) return;
  const uint2 it = items[g];
  const uint32_t fb = it.x, cnt = count[fb], first = it.y * ACC_CAP, len = min(ACC_CAP, cnt - first);
  const uint32_t *ent = sorted + start[fb] + first;
  uint32_t *dst = cnt > ACC_CAP ? pieces + ((size_t)piece_base[fb] + it.y) * XYZZ_WORDS : buckets + (size_t)fb * XYZZ_WORDS;
  uint32_t k = 0;
  aff29 P;
  if (!acc_next_finite(ent, k, len, points, P)) { xyzz_store(dst, xyzz29_to_xyzz(xyzz29_inf())); return; }
  xyzz29 acc;
  acc.X = P.x; acc.Y = P.y; acc.ZZ = fq29_zero(); acc.ZZ.n[0] = 1u; acc.ZZZ = acc.ZZ;
  aff29 P1;
  if (acc_next_finite(ent, k, len, points, P1)) acc = xyzz29_from_two(P, P1);      // two or more finite entries: affine + affine, 4 M + 2 S
  uint32_t e = k < len ? ent[k] : 0u;
  for (; k < len; k++) {
    const uint32_t e_next = (k + 1 < len) ? ent[k + 1] : 0u;
    bool finite;
    P = aff29_load_finite(points + (size_t)(e & 0x7FFFFFFFu) * 16, (e >> 31) & 1u, finite);
    if (finite) xyzz29_madd_fast(acc, P);
    e = e_next;
  }
  if (fq29_normalizes_to_zero(acc.ZZ)) { acc_item_complete29(ent, len, points, dst); return; }
  xyzz_store(dst, xyzz29_to_xyzz(acc));
}

// ------------------------------------------------------------------------------------------------
// 4. bucket reduction: per window  sum_{m=1..M} m * B_m
// One wavefront handles 64*Lw consecutive buckets: lane l takes buckets [ (wave*64+l)*Lw, +Lw ).
__global__ void __launch_bounds__(64) k_reduce1(const uint32_t *__restrict__ buckets, int M, int Lw, int WPW, uint32_t *__restrict__ red) {
  const uint32_t nbw = blockIdx.x, wave = blockIdx.y, lane = threadIdx.x;
  uint32_t t = wave * 64 + lane;                 // lane index within the window
  xyzz run = xyzz_inf(), acc = xyzz_inf();
  if ((uint64_t)t * Lw < (uint64_t)M) {
    const uint32_t *b = buckets + ((size_t)nbw * M + (size_t)t * Lw) * XYZZ_WORDS;
    for (int k = Lw - 1; k >= 0; k--) {          // running sum from the top: acc = sum (k+1) * B_k
      xyzz B = xyzz_load(b + (size_t)k * XYZZ_WORDS);
      xyzz_add(run, B);
      xyzz_add(acc, run);
    }
  }
  // inclusive suffix scan of the lane sums S_l over the wavefront
  xyzz suf = run;
  for (int d = 1; d < 64; d <<= 1) {
    xyzz o = xyzz_shfl_down(suf, d);
    if ((int)lane + d < 64) xyzz_add(suf, o);
  }
  // V_l = acc_l + Lw * (l >= 1 ? suf_l : 0);  sum_l l*S_l = sum_{l>=1} suf_l
  xyzz v = (lane >= 1) ? suf : xyzz_inf();
  for (int k = Lw; k > 1; k >>= 1) v = xyzz_dbl(v);
  xyzz_add(v, acc);
  for (int d = 32; d >= 1; d >>= 1) {
    xyzz o = xyzz_shfl_down(v, d);
    if ((int)lane + d < 64) xyzz_add(v, o);
  }
  if (lane == 0) {
    uint32_t *o = red + ((size_t)nbw * WPW + wave) * (2 * XYZZ_WORDS);
    xyzz_store(o, v);          // A_wave
    xyzz_store(o + XYZZ_WORDS, suf);   // S_wave (lane 0's inclusive suffix = whole-wave sum)
  }
}
// across the wavefronts of a window: total = sum_j A_j + (64*Lw) * sum_{j>=1} suffix_j(S)
__global__ void __launch_bounds__(64) k_reduce2(const uint32_t *__restrict__ red, int Lw, int WPW, uint32_t *__restrict__ winsum) {
  const uint32_t nbw = blockIdx.x, lane = threadIdx.x;
  xyzz A = xyzz_inf(), S = xyzz_inf();
  if ((int)lane < WPW) {
    const uint32_t *r = red + ((size_t)nbw * WPW + lane) * (2 * XYZZ_WORDS);
    A = xyzz_load(r); S = xyzz_load(r + XYZZ_WORDS);
  }
  xyzz suf = S;
  for (int d = 1; d < 64; d <<= 1) {
    xyzz o = xyzz_shfl_down(suf, d);
    if ((int)lane + d < 64) xyzz_add(suf, o);
  }
  xyzz v = (lane >= 1) ? suf : xyzz_inf();
  for (int k = 64 * Lw; k > 1; k >>= 1) v = xyzz_dbl(v);
  xyzz_add(v, A);
  for (int d = 32; d >= 1; d >>= 1) {
    xyzz o = xyzz_shfl_down(v, d);
    if ((int)lane + d < 64) xyzz_add(v, o);
  }
  if (lane == 0) xyzz_store(winsum + (size_t)nbw * XYZZ_WORDS, v);
}

// ---- 4'. bucket reduction by marginal sums (windows with M >= 256 buckets).
// A dependent chain of point additions runs at ONE wavefront's instruction rate (~6 us per addition), so the running-sum scheme
// above costs its depth: ~23 chained additions in k_reduce1 at 2 wavefronts per SIMD plus ~21 in k_reduce2 on 17 wavefronts.
// Here the bucket index splits as i = hi * LO + lo (weight i + 1 = LO * hi + (lo + 1)):
//     sum_i (i + 1) B_i  =  LO * sum_hi hi * R_hi  +  sum_lo (lo + 1) * C_lo,     R_hi = sum_lo B,   C_lo = sum_hi B
// R and C are PLAIN sums: k_reduce_marg gives every lane S consecutive (rows) or strided (columns) buckets — no scan, every
// lane busy, one wavefront per SIMD — and finishes them with a short segmented tree.  With the SIMD to itself the wavefront adds with
// xyzz_add_chain (ec.hip.h: the products of an addition issued in pairs, so that one fills the other's stall slots) and loads the
// next bucket while it adds the current one; so do the trees of k_merge_heavy.  The two weighted sums left are over HI and
// LO (<= 256) elements: k_reduce_tail_quad, on TR = HI / 16 row and TC = LO / 16 column blocks of 16 elements.  The factor LO is not
// applied on the device at all: the window combine, which doubles c times per window anyway, takes (W1, W2) and does
// r = (r * 2^(c-a) + W1) * 2^a + W2.  (MargGeom: msm_plan.hpp)

// the serial part of a lane: b[0] + b[stride] + ... (S terms).  Bucket k + 1 is loaded (ten 16-byte loads into a second set of registers)
// before bucket k is added, so the wavefront — alone on its SIMD, nothing else to hide a load behind — waits for memory once, not S times.
BPPP_DI xyzz marg_serial_sum(const uint32_t *b, int S, size_t stride) {
  xyzz acc = xyzz_load(b);
  if (S < 2) return acc;
  xyzz B = xyzz_load(b + stride);
  for (int k = 2; k < S; k++) {
    const xyzz Bn = xyzz_load(b + (size_t)k * stride);
    xyzz_add_chain(acc, B);
    B = Bn;
  }
  xyzz_add_chain(acc, B);
  return acc;
}

__global__ void __launch_bounds__(64) k_reduce_marg(const uint32_t *__restrict__ buckets, int M, MargGeom Gm, uint32_t *__restrict__ R, uint32_t *__restrict__ C) {
  const uint32_t nbw = blockIdx.y, lane = threadIdx.x;
  const uint32_t *wb = buckets + (size_t)nbw * M * XYZZ_WORDS;
  xyzz acc = xyzz_inf();
  if (blockIdx.x < Gm.row_tiles) {
    const uint32_t r = blockIdx.x * 64 + lane, hi = r / (uint32_t)Gm.PR, part = r % (uint32_t)Gm.PR;
    const bool act = hi < (uint32_t)Gm.HI;
    if (act) {
      const uint32_t *b = wb + ((size_t)hi * Gm.LO + (size_t)part * Gm.SR) * XYZZ_WORDS;
      acc = marg_serial_sum(b, Gm.SR, XYZZ_WORDS);
    }
    for (int d = Gm.PR >> 1; d >= 1; d >>= 1) {
      xyzz o = xyzz_shfl_down(acc, d);
      if ((int)part + d < Gm.PR) xyzz_add_chain(acc, o);
    }
    if (act && part == 0) xyzz_store(R + ((size_t)nbw * Gm.HI + hi) * XYZZ_WORDS, acc);
  } else {
    const uint32_t q = (blockIdx.x - Gm.row_tiles) * 64 + lane, lo = q / (uint32_t)Gm.PC, part = q % (uint32_t)Gm.PC;
    const bool act = lo < (uint32_t)Gm.LO;
    if (act) {
      const uint32_t *b = wb + ((size_t)part * Gm.SC * Gm.LO + lo) * XYZZ_WORDS;
      acc = marg_serial_sum(b, Gm.SC, (size_t)Gm.LO * XYZZ_WORDS);
    }
    for (int d = Gm.PC >> 1; d >= 1; d >>= 1) {
      xyzz o = xyzz_shfl_down(acc, d);
      if ((int)part + d < Gm.PC) xyzz_add_chain(acc, o);
    }
    if (act && part == 0) xyzz_store(C + ((size_t)nbw * Gm.LO + lo) * XYZZ_WORDS, acc);
  }
}

// The two weighted sums with one QUAD per element (ec_quad.hip.h): a quad addition is about a third of a lane addition's depth,
// and the extra lanes are free where the chip is idle.  A block of 16 elements is one single-wavefront workgroup (workgroups land
// on separate CUs, so every wavefront has a SIMD of its own; 16 wavefronts of one workgroup would share four).  The R kind reads
// its elements shifted by one, R'_k = R_{k+1}, so that both kinds are  W = sum_i (i + 1) E_i.  With i = 16 b + j:
//     W = sum_b A_b + 16 * sum_b b S_b,     A_b = sum_j (j + 1) E_{16b+j} = sum_j suffix_j,   S_b = sum_j E_{16b+j} = suffix_0
// Every block writes (A_b, S_b) to part[] and draws a ticket; the last block of a (window, kind) does the second line on one quad per
// block (suffix scan of S, four doublings, one addition, a tree).  Depth: 4 + 4 quad additions, then 2 log2(TB) + 1 additions and
// 4 doublings.  cnt[] (one word per (window, kind)) is zero at launch.
__global__ void __launch_bounds__(64) k_reduce_tail_quad(const uint32_t *__restrict__ R, const uint32_t *__restrict__ C, MargGeom Gm, uint32_t *__restrict__ part,
                                                         uint32_t *__restrict__ cnt, uint32_t *__restrict__ winsum2) {
  __shared__ uint32_t last;
  const uint32_t nbw = blockIdx.y, lane = threadIdx.x, qd = lane >> 2;
  const bool isC = blockIdx.x >= (uint32_t)Gm.TR;
  const uint32_t blk = isC ? blockIdx.x - Gm.TR : blockIdx.x, nb = isC ? Gm.TC : Gm.TR, i = blk * 16 + qd;
  xyzz suf = xyzz_inf();
  if (isC) suf = xyzz_load(C + ((size_t)nbw * Gm.LO + i) * XYZZ_WORDS);
  else if (i + 1 < (uint32_t)Gm.HI) suf = xyzz_load(R + ((size_t)nbw * Gm.HI + i + 1) * XYZZ_WORDS);
  for (int d = 1; d < 16; d <<= 1) {             // inclusive suffix scan over the 16 quads
    xyzz o = xyzz_shfl_down(suf, 4 * d);
    xyzz_add_quad<true>(suf, xyzz_or_inf(qd + d < 16, o));
  }
  xyzz v = suf;
  for (int d = 8; d >= 1; d >>= 1) {             // tree of the suffixes: A_b in quad 0
    xyzz o = xyzz_shfl_down(v, 4 * d);
    xyzz_add_quad<true>(v, xyzz_or_inf(qd + d < 16, o));
  }
  uint32_t *pb = part + (((size_t)nbw * 2 + (isC ? 1 : 0)) * 16 + blk) * 2 * XYZZ_WORDS;
  if (lane == 0) xyzz_store(pb, v);
  if (lane == 1) xyzz_store(pb + XYZZ_WORDS, suf);
  // publish (A_b, S_b): agent-scope release before the ticket; the last arriver acquires before it reads the other blocks' pairs
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (lane == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t t = __hip_atomic_fetch_add(cnt + (size_t)nbw * 2 + (isC ? 1 : 0), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = t == nb - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  // quad b < nb holds block b
  const uint32_t *pr = part + ((size_t)nbw * 2 + (isC ? 1 : 0)) * 16 * 2 * XYZZ_WORDS;
  xyzz A = xyzz_inf(), S = xyzz_inf();
  if (qd < nb) { A = xyzz_load(pr + (size_t)qd * 2 * XYZZ_WORDS); S = xyzz_load(pr + ((size_t)qd * 2 + 1) * XYZZ_WORDS); }
  for (uint32_t d = 1; d < nb; d <<= 1) {
    xyzz o = xyzz_shfl_down(S, 4 * d);
    xyzz_add_quad<true>(S, xyzz_or_inf(qd + d < nb, o));
  }
  // sum_b b S_b = sum_{b >= 1} suffix_b; times 16, plus A_b, summed over the blocks
  v = xyzz_or_inf(qd >= 1, S);
  for (int k = 0; k < 4; k++) xyzz_dbl_quad<true>(v);
  xyzz_add_quad<true>(v, A);
  for (uint32_t d = nb >> 1; d >= 1; d >>= 1) {
    xyzz o = xyzz_shfl_down(v, 4 * d);
    xyzz_add_quad<true>(v, xyzz_or_inf(qd + d < nb, o));
  }
  if (lane == 0) xyzz_store(winsum2 + ((size_t)nbw * 2 + (isC ? 1 : 0)) * XYZZ_WORDS, v);
}

// Many small windows (batched MSMs of a few hundred terms: M <= 256 buckets per window, thousands of windows): a whole
// wavefront per window leaves most lanes idle and pays two 6-step scans.  Here a GROUP of G lanes (G | 64, G <= M) owns one
// window: lane g sums its Lw = M/G buckets serially, the G lane sums go through a log2(G)-step suffix scan inside the
// group, and the window sum goes straight to `winsum` (no k_reduce2 pass).
__global__ void __launch_bounds__(64) k_reduce_groups(const uint32_t *__restrict__ buckets, int M, int G, uint32_t NB, uint32_t *__restrict__ winsum) {
  const uint32_t lane = threadIdx.x, gl = lane & (uint32_t)(G - 1);
  const uint32_t nbw = (blockIdx.x * 64u + lane) / (uint32_t)G;
  const int Lw = M / G;
  xyzz run = xyzz_inf(), acc = xyzz_inf();
  if (nbw < NB) {
    const uint32_t *b = buckets + ((size_t)nbw * M + (size_t)gl * Lw) * XYZZ_WORDS;
    for (int k = Lw - 1; k >= 0; k--) {
      xyzz B = xyzz_load(b + (size_t)k * XYZZ_WORDS);
      xyzz_add(run, B);
      xyzz_add(acc, run);
    }
  }
  xyzz suf = run;                                // inclusive suffix scan of the lane sums inside the group
  for (int d = 1; d < G; d <<= 1) {
    xyzz o = xyzz_shfl_down(suf, d);
    if ((int)gl + d < G) xyzz_add(suf, o);
  }
  xyzz v = (gl >= 1) ? suf : xyzz_inf();         // sum_g g * S_g = sum_{g>=1} suf_g, times Lw
  if (G > 1) for (int k = Lw; k > 1; k >>= 1) v = xyzz_dbl(v);
  xyzz_add(v, acc);
  for (int d = G >> 1; d >= 1; d >>= 1) {
    xyzz o = xyzz_shfl_down(v, d);
    if ((int)gl + d < G) xyzz_add(v, o);
  }
  if (gl == 0 && nbw < NB) xyzz_store(winsum + (size_t)nbw * XYZZ_WORDS, v);
}

// 5. batched window combine: one lane per MSM instance
// `a` > 0: every window comes as two points (W1, W2) with window value 2^a * W1 + W2 (marginal-sum reduction)
__global__ void __launch_bounds__(64) k_window_combine(const uint32_t *__restrict__ winsum, int W, int c, int a, uint32_t batch, uint32_t *__restrict__ out_aff) {
  uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  xyzz r = xyzz_inf();
  for (int w = W - 1; w >= 0; w--) {
    if (a) {
      for (int k = 0; k < c - a; k++) r = xyzz_dbl(r);
      xyzz t1 = xyzz_load(winsum + ((size_t)b * W + w) * 2 * XYZZ_WORDS);
      xyzz_add(r, t1);
      for (int k = 0; k < a; k++) r = xyzz_dbl(r);
      xyzz t2 = xyzz_load(winsum + (((size_t)b * W + w) * 2 + 1) * XYZZ_WORDS);
      xyzz_add(r, t2);
    } else {
      for (int k = 0; k < c; k++) r = xyzz_dbl(r);
      xyzz t = xyzz_load(winsum + ((size_t)b * W + w) * XYZZ_WORDS);
      xyzz_add(r, t);
    }
  }
  aff_store(out_aff + (size_t)b * 16, xyzz_to_aff(r));
}

// ------------------------------------------------------------------------------------------------
// 0. ONE small MSM (a few thousand terms, one instance) in one or two launches: the general pipeline is ~16 launches and four dependency
// chains deep (0.28 ms of kernels for the 858-term MSM of a single range-proof verification, whatever the window); here one workgroup per
// (window, slice of the terms) does all of it — sign fold + digit of its window for every scalar of the slice, a counting sort of the
// entries in LDS, M = 2^(c-1) buckets with 256 / M lanes each (a shuffle tree joins them), and the running-sum reduction sum (m + 1) B_m
// as a suffix scan + tree over M lanes.  c = 6: 43 windows, ~17 dependent point operations deep (0.13 ms).  k_msm_small_join adds the
// slices of a window (one wavefront per window); the window sums go to the host's Horner combine like the general path's.
// (MSM_SMALL_MAX terms per slice and the route's default length limit: msm_plan.hpp, MsmSmallPlan)
__global__ void __launch_bounds__(256) k_msm_small(const uint32_t *__restrict__ scalars_all, const uint32_t *__restrict__ points_all, uint32_t n_all, uint32_t slice_len,
                                                   int c, int acnt, int top, RecodeK K, uint32_t *__restrict__ winsum) {
  // slice blockIdx.y of the terms: its own bucket set, its own partial window sum (k_msm_small_join adds the slices of a window)
  const uint32_t j0 = blockIdx.y * slice_len, n = min(slice_len, n_all - j0);
  const uint32_t *scalars = scalars_all + (size_t)j0 * 8, *points = points_all + (size_t)j0 * 16;
  extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
  const int M = 1 << (c - 1);
  const uint32_t w = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
  uint32_t *hist = sm, *start = hist + M, *sorted = start + M + 1;
  uint16_t *key = (uint16_t *)(sorted + n);
  uint32_t *bsum = sm + (((size_t)(2 * M + 1) + n + (n + 1) / 2 + 3) & ~(size_t)3);    // [M + 4] bucket sums, then the wavefronts' results
  for (int t = tid; t < M; t += 256) hist[t] = 0;
  __syncthreads();
  // balanced windows (as make_plan's): windows [0, acnt) are c bits wide, the others c - 1 and use half of the M buckets — with uniform widths
  // the top window (3 real bits at c = 6) had 4 buckets of n / 4 entries and its workgroup set the kernel's time
  const int cw = (int)w < acnt ? c : c - 1;
  const uint32_t bit0 = (int)w < acnt ? (uint32_t)c * w : (uint32_t)(c * acnt + (c - 1) * ((int)w - acnt)), mask = (1u << cw) - 1u;
  const int half = 1 << (cw - 1);
  const uint32_t flip = (int)w == top ? 1u : 0u;                    // window `top` is unbiased: read negated with the sign flipped, as k_digits stores it
  for (uint32_t j = tid; j < n; j += 256) {
    uint32_t sp[9];
    const bool neg = recode_fold(fe_load(scalars + (size_t)j * 8), K, sp);
    uint32_t lo = 0, hi = 0;                                        // the two limbs around bit0 (above sp[8]: zero)
#pragma unroll
    for (int q = 0; q < 9; q++) if ((bit0 >> 5) == (uint32_t)q) { lo = sp[q]; hi = q < 8 ? sp[q + 1] : 0u; }
    const uint32_t sh = bit0 & 31u;
    const uint32_t d = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & mask;
    const int v = flip ? -(int)d : (int)d - half;
    uint16_t kx = 0xFFFFu;
    if (v) {
      const uint32_t mb = (uint32_t)(v < 0 ? -v : v) - 1u;
      kx = (uint16_t)((mb << 1) | ((((v < 0) != neg) ? 1u : 0u) ^ flip));
      atomicAdd(&hist[mb], 1u);
    }
    key[j] = kx;
  }
  __syncthreads();
  if (tid < 64) {                                                   // exclusive prefix of hist[M] (M <= 128): lane owns M / 64 or one bucket
    const int per = M > 64 ? M / 64 : 1;
    uint32_t s0 = 0;
    for (int q = 0; q < per; q++) { const int b = (int)lane * per + q; if (b < M) s0 += hist[b]; }
    uint32_t inc = s0;
    for (int dd = 1; dd < 64; dd <<= 1) { const uint32_t o = __shfl_up(inc, dd, 64); if ((int)lane >= dd) inc += o; }
    uint32_t run = inc - s0;
    for (int q = 0; q < per; q++) { const int b = (int)lane * per + q; if (b < M) { const uint32_t h = hist[b]; start[b] = run; hist[b] = run; run += h; } }
    if (lane == 63) start[M] = inc;
  }
  __syncthreads();
  for (uint32_t j = tid; j < n; j += 256) {
    const uint16_t kx = key[j];
    if (kx != 0xFFFFu) { const uint32_t pos = atomicAdd(&hist[kx >> 1], 1u); sorted[pos] = ((uint32_t)(kx & 1u) << 31) | j; }
  }
  __syncthreads();
  // ---- buckets: LPB = 256 / M lanes per bucket, entries dealt round-robin, then a shuffle tree inside the group
  const uint32_t LPB = 256u / (uint32_t)M, b = tid / LPB, sub = tid % LPB;
  xyzz acc = xyzz_inf();
  {
    const uint32_t p1 = start[b + 1];
    for (uint32_t p = start[b] + sub; p < p1; p += LPB) {
      const uint32_t e = sorted[p];
      xyzz_madd(acc, aff_cneg(aff_load(points + (size_t)(e & 0x7FFFFFFFu) * 16), (e >> 31) != 0));
    }
  }
  for (uint32_t dd = LPB >> 1; dd >= 1; dd >>= 1) {
    const xyzz o = xyzz_shfl_down(acc, (int)dd);
    if (sub + dd < LPB) xyzz_add(acc, o);
  }
  if (sub == 0) xyzz_store(bsum + (size_t)b * XYZZ_WORDS, acc);
  __syncthreads();
  // ---- sum_m (m + 1) B_m = sum over m of the inclusive suffix sums: suffix scan + tree over the M lanes of each wavefront
  const uint32_t nw = ((uint32_t)M + 63u) / 64u;
  if (tid < 64u * nw) {
    const uint32_t m = tid;
    xyzz suf = m < (uint32_t)M ? xyzz_load(bsum + (size_t)m * XYZZ_WORDS) : xyzz_inf();
    const int Mw = M < 64 ? M : 64;                                 // live lanes of a wavefront
    for (int dd = 1; dd < Mw; dd <<= 1) {
      const xyzz o = xyzz_shfl_down(suf, dd);
      if ((int)lane + dd < Mw) xyzz_add(suf, o);
    }
    xyzz tot = suf;                                                 // lane 0: the whole wavefront's plain sum
    xyzz v = suf;
    for (int dd = Mw >> 1; dd >= 1; dd >>= 1) {
      const xyzz o = xyzz_shfl_down(v, dd);
      if ((int)lane + dd < Mw) xyzz_add(v, o);
    }
    if (lane == 0) {                                                // results go past the M bucket sums the other wavefront may still be loading
      xyzz_store(bsum + (size_t)(M + 2 * (tid >> 6)) * XYZZ_WORDS, v);
      xyzz_store(bsum + (size_t)(M + 2 * (tid >> 6) + 1) * XYZZ_WORDS, tot);
    }
  }
  __syncthreads();
  if (tid == 0) {
    xyzz r = xyzz_load(bsum + (size_t)M * XYZZ_WORDS);              // A_0
    for (uint32_t j = 1; j < nw; j++) {                             // + A_j + 64 j T_j
      xyzz a = xyzz_load(bsum + (size_t)(M + 2 * j) * XYZZ_WORDS), t = xyzz_load(bsum + (size_t)(M + 2 * j + 1) * XYZZ_WORDS);
      for (int q = 0; q < 6; q++) t = xyzz_dbl(t);                  // 64 T_j (nw <= 2: j = 1)
      xyzz_add(r, a); xyzz_add(r, t);
    }
    xyzz_store(winsum + ((size_t)w * gridDim.y + blockIdx.y) * XYZZ_WORDS, r);
  }
}
// window w = the sum of its S slice partials: one wavefront per window
__global__ void __launch_bounds__(64) k_msm_small_join(const uint32_t *__restrict__ partials, uint32_t S, uint32_t *__restrict__ winsum) {
  const uint32_t w = blockIdx.x, lane = threadIdx.x;
  xyzz acc = xyzz_inf();
  for (uint32_t s_ = lane; s_ < S; s_ += 64) {
    const xyzz p = xyzz_load(partials + ((size_t)w * S + s_) * XYZZ_WORDS);
    if (s_ < 64) acc = p; else xyzz_add(acc, p);
  }
  uint32_t top = 1; while (top < S && top < 64) top <<= 1;
  for (uint32_t dd = top >> 1; dd >= 1; dd >>= 1) {
    const xyzz o = xyzz_shfl_down(acc, (int)dd);
    if (lane + dd < 64) xyzz_add(acc, o);
  }
  if (lane == 0) xyzz_store(winsum + (size_t)w * XYZZ_WORDS, acc);
}

// ------------------------------------------------------------------------------------------------
// host orchestration: the plan and the workspace layout come from msm_plan.hpp; here the small route and the stages of the general pipeline,
// one launcher each, in the order msm_run_ex calls them.  The prof_mark indices are the stage boundaries bench.py reads.

// the one-shot hook that runs right before the first kernel that reads the points (ctx.hpp)
static int run_pre_acc(bppp_ctx *ctx) {
  if (!ctx->pre_acc) return BPPP_OK;
  auto f = ctx->pre_acc; ctx->pre_acc = nullptr;
  return f(ctx->pre_acc_arg);
}

// ---- one small or mid-size MSM: k_msm_small over (window, slice of <= 4096 terms) workgroups, the slices of a window joined by one
// wavefront each, then the host's Horner combine over the W window sums
static int msm_small(bppp_ctx *ctx, const void *d_scalars, const void *d_points, size_t n, uint64_t *out_xy) {
  using namespace bppp_host;
  const MsmSmallPlan s = make_small_plan(n, ctx->tune);
  Carver sizing(nullptr, 0);
  carve_small(sizing, s);
  int rc = ensure_workspace(ctx, sizing.off); if (rc) return rc;
  Carver cv(ctx->ws, ctx->ws_bytes);
  const MsmSmallWorkspace ws = carve_small(cv, s);
  const size_t bytes = (size_t)s.W * XYZZ_WORDS * 4;
  rc = ensure_pinned(ctx, bytes); if (rc) return rc;
  hipStream_t st = ctx->stream;
  ctx->last_windows = s.W;
  ctx->last_msm_valid = false;       // this route lays the workspace out its own way (carve_small)
  ReduceLast &last = ctx->last_reduce;
  last = ReduceLast();
  last.route = 0; last.combine = 0; last.c = s.c; last.W = s.W; last.M = 1 << (s.c - 1); last.S = (int)s.S;
  for (int i = 0; i <= 2; i++) prof_mark(ctx, i);
  rc = run_pre_acc(ctx); if (rc) return rc;
  k_msm_small<<<dim3((unsigned)s.W, (unsigned)s.S), dim3(256), s.lds, st>>>((const uint32_t *)d_scalars, (const uint32_t *)d_points, (uint32_t)n, (uint32_t)s.len, s.c,
                                                                         s.acnt, s.top, make_recode_k(s.c, s.W, s.acnt, s.top >= 0), s.S > 1 ? ws.partials : ws.winsum);
  if (s.S > 1) k_msm_small_join<<<dim3((unsigned)s.W), dim3(64), 0, st>>>(ws.partials, (uint32_t)s.S, ws.winsum);
  for (int i = 3; i <= 5; i++) prof_mark(ctx, i);
  BPPP_HIP(ctx, hipMemcpyAsync(ctx->pinned, ws.winsum, bytes, hipMemcpyDeviceToHost, st));
  prof_mark(ctx, 6);
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  window_combine_host((const uint32_t *)ctx->pinned, s.W, s.c, s.acnt, false, 0, out_xy);
  BPPP_HIP(ctx, hipGetLastError());
  prof_collect(ctx, 7);
  return BPPP_OK;
}

// ---- the general pipeline
// the sort kernels' dynamic LDS above the 64 KiB a kernel gets unasked: set once per size, not per call
static int msm_sort_lds(bppp_ctx *ctx, const MsmPlan &p) {
  const size_t lds = sort_lds_bytes(p);
  if (lds > 64 * 1024 && lds > ctx->sort_lds_set) {
    BPPP_HIP(ctx, hipFuncSetAttribute((const void *)k_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    BPPP_HIP(ctx, hipFuncSetAttribute((const void *)k_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    BPPP_HIP(ctx, hipFuncSetAttribute((const void *)k_scatter_ranges, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    BPPP_HIP(ctx, hipFuncSetAttribute((const void *)k_scatter_one_read, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ctx->sort_lds_set = lds;
  }
  return BPPP_OK;
}

// 1. digits; the first kernel of the call also zeroes its counters and the scan's tile sums
static void msm_digits(bppp_ctx *ctx, const MsmPlan &p, const MsmWorkspace &ws, const void *d_scalars) {
  const uint64_t total_sc = (uint64_t)p.batch * p.n;
  k_digits<<<dim3((unsigned)((total_sc + 255) / 256)), dim3(256), 0, ctx->stream>>>((const uint32_t *)d_scalars, total_sc, (uint32_t)p.n, ws.stride, p.c, p.W, p.acnt, p.top,
                                                                                     make_recode_k(p.c, p.W, p.acnt, p.top >= 0), ws.dig, ws.negmask, ws.heavy_count,
                                                                                     (uint32_t)ws.nzero, ws.tiles, (uint32_t)p.ntiles);
}

// 2. sort
static void msm_sort(bppp_ctx *ctx, const MsmPlan &p, const MsmWorkspace &ws, size_t table_stride) {
  hipStream_t st = ctx->stream;
  const size_t lds = sort_lds_bytes(p);
  const uint32_t n = (uint32_t)p.n;
  const int h16 = p.hist16 ? 1 : 0;                          // 16-bit counts and prefixes in the front half of blockhist (a ranged scatter's plan only)
  k_hist<<<dim3((unsigned)p.NB, p.CH), dim3(p.hist_threads), lds, st>>>(ws.dig, n, ws.stride, p.c, p.CH, ws.blockhist, h16);
  // flat: the (window, chunk) histograms of an instance are W * CH chunks of ONE bucket set (same memory layout)
  if (h16) k_count_tiles16<<<dim3((unsigned)((p.FB / 2 + 255) / 256)), dim3(256), 0, st>>>(ws.blockhist, p.M, p.CH, p.FB, ws.count, ws.tiles);
  else k_count_tiles<<<dim3((unsigned)((p.FB + 255) / 256)), dim3(256), 0, st>>>(ws.blockhist, p.M, p.flat ? p.W * p.CH : p.CH, p.FB, ws.count, ws.tiles);
  k_scan_apply<<<dim3(p.ntiles), dim3(256), 0, st>>>(ws.count, p.FB, ws.tiles, ws.start, ws.size_hist);
  ctx->last_sort_ranges = p.Q;
  ctx->last_windows = p.W;
  ctx->last_scatter_one_read = p.one_read ? 1 : 0;
  ctx->last_hist16 = h16;
  if (p.one_read) {
    // 8 slots x ceil(W / 8) windows x CH chunks; the cursors of all M buckets take the whole request, which leaves ONE workgroup per CU
    k_scatter_one_read<<<dim3(ranged_grid(p)), dim3(p.hist_threads), lds, st>>>(ws.dig, ws.negmask, n, ws.stride, p.c, p.CH, p.Q, (uint32_t)p.W, p.top, ws.blockhist,
                                                                                ws.start, ws.sorted, h16);
  } else if (p.Q) {
    // units (window, range); 8 slots x ceil(U / 8) units x CH chunks
    k_scatter_ranges<<<dim3(ranged_grid(p)), dim3(p.hist_threads), ranges_lds_bytes(p), st>>>(ws.dig, ws.negmask, n, ws.stride, p.c, p.CH, p.Q, ranges_units(p), p.top,
                                                                                              ws.blockhist, ws.start, ws.sorted, h16);
  } else
    k_scatter<<<dim3((unsigned)p.NB, p.CH), dim3(p.hist_threads), lds, st>>>(ws.dig, ws.negmask, n, ws.stride, p.c, p.CH, p.W, ws.blockhist, ws.start, ws.sorted,
                                                                             p.flat ? (uint32_t)table_stride : 0u, p.top);
}

// 3. accumulate: bucket sums from the sorted entries, then the buckets left in several partial sums
static int msm_accumulate(bppp_ctx *ctx, const MsmPlan &p, const MsmWorkspace &ws, const void *d_points, int shared_points) {
  hipStream_t st = ctx->stream;
  uint2 *items = (uint2 *)ws.items, *heavy_items = (uint2 *)ws.heavy_items;
  uint4 *heavy_buckets = (uint4 *)ws.heavy_buckets;
  ctx->last_acc_sized = p.sized ? 1 : 0;
  ctx->last_acc_fq29 = p.fq29 ? 1 : 0;
  // the ordering pass has to precede the accumulation, so its time is booked with acc_points; acc_points + acc_records is the accumulation
  // on either route
  if (p.sized)
    k_order<<<dim3(p.ntiles), dim3(256), 0, st>>>(ws.count, p.FB, ws.size_hist, ws.cursors, items, ws.piece_base, ws.buckets, heavy_items, ws.heavy_slot, heavy_buckets,
                                                  ws.heavy_count);
  int rc = run_pre_acc(ctx); if (rc) return rc;
  if (p.sized) {
    (p.acc_fast ? k_acc_points_sized29_fast : p.fq29 ? k_acc_points_sized29 : k_acc_points_sized)<<<dim3((unsigned)((ws.items_max + 255) / 256)), dim3(256), 0, st>>>(
        ws.sorted, ws.start, ws.count, items, ws.heavy_count, ws.piece_base, (const uint32_t *)d_points, ws.buckets, ws.rec_pt);
    prof_mark(ctx, 3);
    k_merge_heavy<true><<<dim3(2048), dim3(64), 0, st>>>(ws.start, ws.count, 0, ws.rec_pt, ws.piece_base, ws.buckets, heavy_items, ws.heavy_slot, heavy_buckets,
                                                         ws.heavy_count, ws.chunk_sums);
  } else {
    k_acc_points<<<dim3((unsigned)((p.G + 255) / 256)), dim3(256), 0, st>>>(ws.sorted, ws.start, (uint32_t)p.FB, (const uint32_t *)d_points, (uint32_t)p.n,
                                                                            (uint32_t)(p.Wc * p.M), shared_points, p.L, p.G, ws.buckets, ws.rec_pt);
    prof_mark(ctx, 3);
    k_merge<<<dim3((unsigned)((p.FB + 255) / 256)), dim3(256), 0, st>>>(ws.start, ws.count, p.FB, p.L, ws.rec_pt, ws.buckets, heavy_items, ws.heavy_slot, heavy_buckets,
                                                                        ws.heavy_count);
    k_merge_heavy<false><<<dim3(2048), dim3(64), 0, st>>>(ws.start, ws.count, p.L, ws.rec_pt, nullptr, ws.buckets, heavy_items, ws.heavy_slot, heavy_buckets,
                                                          ws.heavy_count, ws.chunk_sums);
  }
  return BPPP_OK;
}

// 4. bucket reduce
static void msm_reduce(bppp_ctx *ctx, const MsmPlan &p, const MsmWorkspace &ws) {
  hipStream_t st = ctx->stream;
  ReduceLast &last = ctx->last_reduce;
  last = ReduceLast();
  last.route = p.RG ? 1 : p.marg ? 2 : 3; last.c = p.c; last.W = p.Wc; last.M = p.M;
  if (p.RG) { last.RG = p.RG; last.Lw = p.M / p.RG; }
  else if (p.marg) {
    last.a = p.mg.a; last.LO = p.mg.LO; last.HI = p.mg.HI; last.PR = p.mg.PR; last.PC = p.mg.PC; last.SR = p.mg.SR; last.SC = p.mg.SC;
    last.TR = p.mg.TR; last.TC = p.mg.TC;
  } else { last.Lw = p.Lw; last.WPW = p.WPW; }
  if (p.RG) {
    k_reduce_groups<<<dim3((unsigned)((p.NS * p.RG + 63) / 64)), dim3(64), 0, st>>>(ws.buckets, p.M, p.RG, (uint32_t)p.NS, ws.winsum);
  } else if (p.marg) {
    uint32_t *Rm = ws.red, *Cm = ws.red + (size_t)p.NS * p.mg.HI * XYZZ_WORDS;
    k_reduce_marg<<<dim3(p.mg.row_tiles + p.mg.col_tiles, (unsigned)p.NS), dim3(64), 0, st>>>(ws.buckets, p.M, p.mg, Rm, Cm);
    k_reduce_tail_quad<<<dim3((unsigned)(p.mg.TR + p.mg.TC), (unsigned)p.NS), dim3(64), 0, st>>>(Rm, Cm, p.mg, ws.tail_part, ws.tail_cnt, ws.winsum);
  } else {
    k_reduce1<<<dim3((unsigned)p.NS, p.WPW), dim3(64), 0, st>>>(ws.buckets, p.M, p.Lw, p.WPW, ws.red);
    k_reduce2<<<dim3((unsigned)p.NS), dim3(64), 0, st>>>(ws.red, p.Lw, p.WPW, ws.winsum);
  }
}

// 5. window combine: left in HBM and not waited for (d_out_dev), on the device for a batch, on the host for up to four MSMs
static int msm_finish(bppp_ctx *ctx, const MsmPlan &p, const MsmWorkspace &ws, uint64_t *out_xy, uint32_t *d_out_dev) {
  using namespace bppp_host;
  hipStream_t st = ctx->stream;
  const size_t batch = p.batch;
  const int a = p.marg ? p.mg.a : 0;
  ctx->last_reduce.combine = d_out_dev || batch > 4 ? 1 : 0;
  if (d_out_dev) {
    k_window_combine<<<dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, st>>>(ws.winsum, p.Wc, p.c, a, (uint32_t)batch, d_out_dev);
    BPPP_HIP(ctx, hipGetLastError());
    return BPPP_OK;
  }
  if (batch > 4) {
    k_window_combine<<<dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, st>>>(ws.winsum, p.Wc, p.c, a, (uint32_t)batch, ws.out_aff);
    BPPP_HIP(ctx, hipMemcpyAsync(out_xy, ws.out_aff, batch * 64, hipMemcpyDeviceToHost, st));
    prof_mark(ctx, 6);
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  } else {
    size_t bytes = (size_t)p.NS * (p.marg ? 2 : 1) * XYZZ_WORDS * 4;
    int rc = ensure_pinned(ctx, bytes); if (rc) return rc;
    BPPP_HIP(ctx, hipMemcpyAsync(ctx->pinned, ws.winsum, bytes, hipMemcpyDeviceToHost, st));
    prof_mark(ctx, 6);
    BPPP_HIP(ctx, hipStreamSynchronize(st));
    const uint32_t *wsum = (const uint32_t *)ctx->pinned;
    // a flat table has one bucket set and windows of c bits throughout; the marginal reduction leaves (W1, W2) per window
    for (size_t b = 0; b < batch; b++)
      window_combine_host(wsum + b * p.Wc * (p.marg ? 2 : 1) * XYZZ_WORDS, p.Wc, p.c, p.flat ? p.Wc : p.acnt, p.marg, a, out_xy + 8 * b);
  }
  BPPP_HIP(ctx, hipGetLastError());
  prof_collect(ctx, 7);
  return BPPP_OK;
}

int msm_run_ex(bppp_ctx *ctx, const void *d_scalars, const void *d_points, size_t n, size_t batch, int shared_points, int window_bits, uint64_t *out_xy,
               size_t table_stride, uint32_t *d_out_dev = nullptr);
int msm_run(bppp_ctx *ctx, const void *d_scalars, const void *d_points, size_t n, size_t batch, int shared_points,
            int window_bits, uint64_t *out_xy) {
  return msm_run_ex(ctx, d_scalars, d_points, n, batch, shared_points, window_bits, out_xy, 0);
}
// the same batch of MSMs with the results LEFT IN HBM (d_out [batch][16], canonical affine) and nothing waited for: a link in a stream of kernels
// (the lockstep argument's late rounds over per-proof bases, csrc/nlb.hip).  batch > 4.
int msm_batch_dev(bppp_ctx *ctx, const void *d_scalars, const void *d_points, size_t n, size_t batch, int shared_points, int window_bits, uint32_t *d_out) {
  if (!d_out || batch <= 4 || !n) return fail(ctx, BPPP_ERR_ARG, "msm_batch_dev: bad arguments");
  uint64_t dummy[8];
  return msm_run_ex(ctx, d_scalars, d_points, n, batch, shared_points, window_bits, dummy, 0, d_out);
}
// table_stride != 0: d_points is a precomputed table [W][table_stride] of 2^(c w) P_i for the given window_bits = c (bppp_basis):
// all windows of an instance share one bucket set, so there is one bucket reduction per instance and no window combine
int msm_run_ex(bppp_ctx *ctx, const void *d_scalars, const void *d_points, size_t n, size_t batch, int shared_points, int window_bits, uint64_t *out_xy,
               size_t table_stride, uint32_t *d_out_dev) {
  if (!out_xy) return fail(ctx, BPPP_ERR_ARG, "msm: null output");
  if (n == 0 || batch == 0) { memset(out_xy, 0, 64 * (batch ? batch : 1)); return BPPP_OK; }
  if (!d_scalars || !d_points) return fail(ctx, BPPP_ERR_ARG, "msm: null input");
  if (n >= (1ull << 31)) return fail(ctx, BPPP_ERR_ARG, "msm: n must be < 2^31");
  if (msm_small_route(n, batch, window_bits, table_stride, d_out_dev != nullptr, ctx->tune)) return msm_small(ctx, d_scalars, d_points, n, out_xy);
  int c = window_bits ? window_bits : choose_window(n, batch, ctx->tune);
  if (!window_bits && ctx->tune.window_batched) { const int v = ctx->tune.window_batched; if (batch > 4 && v >= 2 && v <= 16) c = v; }   // tuning sweeps
  if (c < 2 || c > 16) return fail(ctx, BPPP_ERR_ARG, "msm: window_bits must be in [2,16]");
  const bool flat = table_stride != 0;
  if (flat && (!window_bits || shared_points != 1 || n > table_stride || (uint64_t)(256 / c + 1) * table_stride >= (1ull << 31)))
    return fail(ctx, BPPP_ERR_ARG, "msm: bad precomputed-table arguments");
  const MsmPlan p = make_plan(n, batch, c, flat, ctx->tune);
  if (p.FB >= (1ull << 32) - 1 || p.total_max >= (1ull << 32) - 1)
    return fail(ctx, BPPP_ERR_ARG, "msm: batch*windows*buckets or batch*n*windows exceeds 2^32; split the batch");
  // the workspace: laid out once over a null base for its size, once over the real one
  Carver sizing(nullptr, 0);
  carve(sizing, p, n, batch);
  int rc = ensure_workspace(ctx, sizing.off); if (rc) return rc;
  Carver cv(ctx->ws, ctx->ws_bytes);
  const MsmWorkspace ws = carve(cv, p, n, batch);
  rc = msm_sort_lds(ctx, p); if (rc) return rc;
  ctx->last_msm_valid = true; ctx->last_msm_plan = p; ctx->last_msm_n = n; ctx->last_msm_batch = batch; ctx->last_msm_shared_points = shared_points;
  ctx->last_msm_table_stride = table_stride;

  prof_mark(ctx, 0);
  msm_digits(ctx, p, ws, d_scalars);
  prof_mark(ctx, 1);
  msm_sort(ctx, p, ws, table_stride);
  prof_mark(ctx, 2);
  rc = msm_accumulate(ctx, p, ws, d_points, shared_points); if (rc) return rc;   // prof_mark 3 between the accumulation and the merges
  prof_mark(ctx, 4);
  msm_reduce(ctx, p, ws);
  prof_mark(ctx, 5);
  return msm_finish(ctx, p, ws, out_xy, d_out_dev);                              // prof_mark 6 after the copy is queued
}

}  // namespace bppp
