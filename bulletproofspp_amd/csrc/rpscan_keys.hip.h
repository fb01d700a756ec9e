// rpscan_keys.hip.h — a_k P for a LIST of scalars a_0 .. a_{kt-1} and a point P of its own per lane: the walk of the many-key scan
// (csrc/rpscan_keys.hip), where a scanning service tests every output against each of its accounts' view secrets.  In a header because the test
// library (csrc/testhooks.hip) runs the table, the walk and the batched affine conversion alone.
//
// What carries over from the one-key walk (csrc/rpseal.hip.h): a scalar is uniform over the grid, so its digit tests are scalar branches.  That
// still holds when the grid walks a list of scalars one after another: the recoded keys of a tile sit in HBM (ScanKeyRec,
// csrc/rpscan_keys_plan.hpp), are read at wavefront-uniform addresses, and one launch walks all of them.
//
// What only many keys per row pay for: a table of P that NO key's signs are baked into, made once per row and pass, which makes a wider window
// affordable.  Form: a width-4 signed sliding window (wNAF, digits +-1, +-3, +-5, +-7) over each GLV half of a = a1 + a2 lambda.  The table is
// P, 3P, 5P, 7P, the three multiples made AFFINE by one inversion a row; a digit of a1 adds +-(x_m, y_m), a digit of a2 +-(beta x_m, y_m) —
// lambda (x, y) = (beta x, y), one product where the entry is read — and the signs of the halves are folded into the digits on the host.  About
// 130 doublings and 52 additions, all mixed.  Eight field elements a lane, each as its eight canonical 32-bit words (unpacked to limbs where an
// entry is read): 64 words a lane, word-major (one column per lane, no bank conflict, no barrier: a lane reads only its own column), 16 KB a
// wavefront.  The table is written to HBM once per pass (k_rp_scan_table_keys) and loaded into LDS by every workgroup of a walk launch.
// The GLV joint walk of the one-key scan over a sign-free table (P, beta x, P + lambda P, P - lambda P, the sums affine) was built and timed
// against this form and lost.
//
// Every operation is the complete XYZZ law of csrc/ec.hip.h: P at infinity (a table of zeros: every entry is the infinity encoding), a = 0 (no
// digit: the accumulator stays at infinity) and an accumulator that meets a table entry or its negative are ordinary input.
#pragma once
#include "ec.hip.h"
#include "rpseal.hip.h"
#include "rpscan_keys_plan.hpp"

namespace bppp {

// a block's table from HBM into the wavefront's LDS, each lane its own column
BPPP_DI void scan_keys_tab_load(ScanTab *tab, const uint32_t *blk, uint32_t lane, uint32_t words) {
#pragma unroll 8
  for (uint32_t w = 0; w < words; w++) tab[w][lane] = blk[w * 64 + lane];
}
BPPP_DI fq scan_keys_tab_get(const ScanTab *tab, uint32_t lane, uint32_t o) {
  fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = tab[o + i][lane];
  return fq_from_fe(r);
}

// The accumulators of one row under the kt keys of a tile (acc[k * stride], XYZZ) made affine with ONE inversion by Montgomery's trick, three
// products an element: forward, the running product of the ZZ ZZZ is parked in the output slot of its key (P[k * pstride], 10 of its 16 words);
// backward, each slot is read once more and then receives its point.  An accumulator at infinity (ZZ = 0: the scalar = 0 mod n, or P at
// infinity) is left out of the product and gives the all-zero point.
BPPP_DI void scan_keys_affine_lane(uint32_t kt, const uint32_t *acc, size_t stride, uint32_t *P, size_t pstride) {
  fq run = fq_one();
#pragma unroll 1
  for (uint32_t k = 0; k < kt; k++) {
    const uint32_t *a = acc + k * stride;
    fq zz, zzz;
#pragma unroll
    for (int i = 0; i < 10; i++) { zz.n[i] = a[20 + i]; zzz.n[i] = a[30 + i]; }
    if (!fq_all_zero(zz)) run = fq_mul(run, fq_mul(zz, zzz));
#pragma unroll
    for (int i = 0; i < 10; i++) P[k * pstride + i] = run.n[i];
  }
  fq inv = fq_inv(run);
#pragma unroll 1
  for (uint32_t k = kt; k-- > 0;) {
    const xyzz p = xyzz_load(acc + k * stride);
    uint32_t *out = P + k * pstride;
    if (xyzz_is_inf(p)) { aff_store(out, aff_inf()); continue; }
    fq before = fq_one();
    if (k) {
#pragma unroll
      for (int i = 0; i < 10; i++) before.n[i] = out[(ptrdiff_t)i - (ptrdiff_t)pstride];
    }
    const fq mine = fq_mul(inv, before);                 // 1 / (ZZ ZZZ) of this key
    inv = fq_mul(inv, fq_mul(p.ZZ, p.ZZZ));
    aff r;
    r.x = fq_normalize(fq_mul(p.X, fq_mul(mine, p.ZZZ)));
    r.y = fq_normalize(fq_mul(p.Y, fq_mul(mine, p.ZZ)));
    aff_store(out, r);
  }
}

// ---- the table and the walk.  Table: R, 3R, 5R, 7R affine (one inversion a row for the three
// multiples), eight field elements of eight words, 64 words a lane; beta x of an entry is one product where the second half reads it.
static constexpr uint32_t SCANK_TAB_WORDS = 64;
BPPP_DI void scan_keys_table_lane(const aff &P, bool open, uint32_t *blk, uint32_t lane) {
  aff T[4] = {aff_inf(), aff_inf(), aff_inf(), aff_inf()};
  if (open && !aff_is_inf(P)) {
    T[0] = P;
    const xyzz P2 = xyzz_dbl_aff(P);
    xyzz m[3];
    m[0] = P2; xyzz_madd(m[0], P);
    m[1] = m[0]; xyzz_add(m[1], P2);
    m[2] = m[1]; xyzz_add(m[2], P2);
    fq z[3];
#pragma unroll
    for (int j = 0; j < 3; j++) z[j] = xyzz_is_inf(m[j]) ? fq_one() : fq_mul(m[j].ZZ, m[j].ZZZ);      // a multiple at infinity is left out of the product
    const fq z01 = fq_mul(z[0], z[1]), inv = fq_inv(fq_mul(z01, z[2]));
    const fq i2 = fq_mul(inv, z01), i01 = fq_mul(inv, z[2]);
    const fq iv[3] = {fq_mul(i01, z[1]), fq_mul(i01, z[0]), i2};
#pragma unroll
    for (int j = 0; j < 3; j++)
      if (!xyzz_is_inf(m[j])) { T[j + 1].x = fq_normalize(fq_mul(m[j].X, fq_mul(iv[j], m[j].ZZZ))); T[j + 1].y = fq_normalize(fq_mul(m[j].Y, fq_mul(iv[j], m[j].ZZ))); }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const fe x = fq_to_fe(T[j].x), y = fq_to_fe(T[j].y);
#pragma unroll
    for (int i = 0; i < 8; i++) { blk[(16 * j + i) * 64 + lane] = x.v[i]; blk[(16 * j + 8 + i) * 64 + lane] = y.v[i]; }
  }
}
// W: the key's record in HBM at a wavefront-uniform address; a word of digits is read once per four positions
BPPP_DI xyzz scan_keys_mul_lane(const ScanKeyRec *__restrict__ W, const ScanTab *tab, uint32_t lane) {
  const int nbits = (int)W->nbits;
  xyzz acc = xyzz_inf();
  uint32_t word = 0;
#pragma unroll 1
  for (int i = nbits - 1; i >= 0; i--) {
    if (i == nbits - 1 || (i & 3) == 3) word = W->d[i >> 2];
    acc = xyzz_dbl(acc);
    const uint32_t by = (word >> (8 * (i & 3))) & 0xFFu, n1 = by & 15u, n2 = by >> 4;
    if (n1) {
      const uint32_t o = ((n1 & 7u) - 1u) * 16u;
      aff T;
      T.x = scan_keys_tab_get(tab, lane, o); T.y = scan_keys_tab_get(tab, lane, o + 8);
      xyzz_madd(acc, aff_cneg(T, (n1 & 8u) != 0));
    }
    if (n2) {
      const uint32_t o = ((n2 & 7u) - 1u) * 16u;
      aff T;
      T.x = scan_keys_tab_get(tab, lane, o); T.y = scan_keys_tab_get(tab, lane, o + 8);
      if (!aff_is_inf(T)) T.x = fq_normalize(fq_mul(T.x, scan_beta()));
      xyzz_madd(acc, aff_cneg(T, (n2 & 8u) != 0));
    }
  }
  return acc;
}

// ---- the kernels, shared by csrc/rpscan_keys.hip and the test hooks
// one lane per row: the table of R; status NULL: every row is open, else a row whose status is not `open_value` gets the table of infinity
static __global__ void __launch_bounds__(64) k_rp_scan_table_keys(uint32_t n, const uint32_t *__restrict__ R, const uint32_t *__restrict__ status, uint32_t open_value,
                                                                               uint32_t *__restrict__ tab) {
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n) return;
  const bool open = !status || status[b] == open_value;
  uint32_t *blk = tab + (size_t)blockIdx.x * SCANK_TAB_WORDS * 64;
  scan_keys_table_lane(aff_load(R + (size_t)b * 16), open, blk, threadIdx.x);
}
// one lane per row, a workgroup is one wavefront with its table in LDS; acc: [kt][n] XYZZ.  blockIdx.y: the workgroup's first key; gridDim.y:
// the stride.  The launches give every (block of rows, key) a workgroup of its own: one of 64 rows x 16 keys runs 16 times as long, and the last
// round of such workgroups leaves most of the device idle
static __global__ void __launch_bounds__(64) k_rp_scan_walk_keys(uint32_t n, uint32_t kt, const ScanKeyRec *__restrict__ keys,
                                                                              const uint32_t *__restrict__ tabg, uint32_t *__restrict__ acc) {
  __shared__ ScanTab tab[SCANK_TAB_WORDS];
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n) return;
  scan_keys_tab_load(tab, tabg + (size_t)blockIdx.x * SCANK_TAB_WORDS * 64, threadIdx.x, SCANK_TAB_WORDS);
#pragma unroll 1
  for (uint32_t k = blockIdx.y; k < kt; k += gridDim.y) {
    xyzz_store(acc + ((size_t)k * n + b) * XYZZ_WORDS, scan_keys_mul_lane(keys + k, tab, threadIdx.x));
  }
}
// one lane per row: the kt accumulators of the row made affine; P: [kt][n] affine
static __global__ void __launch_bounds__(64) k_rp_scan_affine_keys(uint32_t n, uint32_t kt, const uint32_t *__restrict__ acc, uint32_t *__restrict__ P) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  scan_keys_affine_lane(kt, acc + (size_t)b * XYZZ_WORDS, (size_t)n * XYZZ_WORDS, P + (size_t)b * 16, (size_t)n * 16);
}
// table, walk and conversion of the keys recs[0 .. nk) in tiles of kt over n points, queued on st: out [nk][n] affine; tab, acc, d_keys: workspace of
// (n + 63) / 64 * 64 * TAB_WORDS, kt * n * XYZZ_WORDS and kt * SCAN_KEY_WORDS words.  What the test hook runs; the scan launches the same kernels.
inline hipError_t scan_keys_mul_launch(hipStream_t st, uint32_t n, const ScanKeyRec *recs, size_t nk, size_t kt, const uint32_t *pts,
                                                           uint32_t *tab, uint32_t *acc, uint32_t *d_keys, uint32_t *out) {
  const dim3 grid((n + 63) / 64);
  k_rp_scan_table_keys<<<grid, dim3(64), 0, st>>>(n, pts, nullptr, 0u, tab);
  for (size_t k0 = 0; k0 < nk; k0 += kt) {
    const uint32_t m = (uint32_t)std::min(kt, nk - k0);
    hipError_t e = hipMemcpyAsync(d_keys, recs + k0, m * sizeof(ScanKeyRec), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    k_rp_scan_walk_keys<<<dim3(grid.x, m), dim3(64), 0, st>>>(n, m, (const ScanKeyRec *)d_keys, tab, acc);
    k_rp_scan_affine_keys<<<grid, dim3(64), 0, st>>>(n, m, acc, out + k0 * n * 16);
  }
  return hipGetLastError();
}

}  // namespace bppp
