// testhooks.hip — device field / group arithmetic exposed to the parity tests (include/bppp_test.h).
#include "../../include/bppp_test.h"
#include <vector>
#include "ctx.hpp"
#include "ec.hip.h"
#include "ec29.hip.h"
#include "ec_quad.hip.h"
#include "modinv.hip.h"
#include "fr26.hip.h"
#include "rp_internal.hpp"
#include "rpwitness.hip.h"
#include "rpdecode.hip.h"
#include "rpexcess.hip.h"
#include "rpexpart.hip.h"
#include "rpseal.hip.h"
#include "rpscan_keys.hip.h"
#include "seedpoints.hip.h"
#include "comb.hip.h"
#include "rpp_transcript.hpp"
#include "rpprove_dev.hpp"
#include "trrp.hpp"

namespace bppp {
template <int MOD> BPPP_DI fe apply_op(int op, const fe &a, const fe &b) {
  switch (op) {
    case BPPP_FE_ADD: return fe_add<MOD>(a, b);
    case BPPP_FE_SUB: return fe_sub<MOD>(a, b);
    case BPPP_FE_MUL: return fe_mul<MOD>(a, b);
    case BPPP_FE_SQR: return fe_sqr<MOD>(a);
    case BPPP_FE_INV: return fe_inv<MOD>(a);
    case 7: return fe_inv_vartime<MOD>(a);       // binary extended Euclid (fe.hip.h)
    case 8: return fe_modinv<MOD>(a);            // safegcd division steps (modinv.hip.h)
    default: return fe_neg<MOD>(a);
  }
}
// Fq through the production representation (10 x 26-bit limbs, csrc/fq26.hip.h)
BPPP_DI fe apply_op_fq(int op, const fe &a, const fe &b) {
  fq x = fq_from_fe(a), y = fq_from_fe(b);
  switch (op) {
    case BPPP_FE_ADD: return fq_to_fe(fq_add(x, y));
    case BPPP_FE_SUB: return fq_to_fe(fq_sub<1>(x, y));
    case BPPP_FE_MUL: return fq_to_fe(fq_mul(x, y));
    case BPPP_FE_SQR: return fq_to_fe(fq_sqr(x));
    case BPPP_FE_INV: return fq_to_fe(fq_inv(x));            // production: safegcd
    case 9: return fq_to_fe(fq_inv_fermat(x));               // the addition chain, kept as a cross-check
    default: return fq_to_fe(fq_neg<1>(x));
  }
}
// worst-case magnitudes: (8a) * (8b) with both operands built by repeated lazy additions
BPPP_DI fe apply_mag8_mul(const fe &a, const fe &b) {
  fq x = fq_from_fe(a), y = fq_from_fe(b);
  fq x8 = fq_mul_int(x, 8), y8 = fq_neg<7>(fq_mul_int(y, 7));   // magnitudes 8 and 8
  return fq_to_fe(fq_mul(x8, y8));                               // = -56 a b
}
// Fr through the 10 x 26-bit lazy limbs the verifier's and provers' scalar kernels use (csrc/fr26.hip.h)
BPPP_DI fe apply_op_fr26(int op, const fe &a, const fe &b) {
  fr x = fr_from_fe(a), y = fr_from_fe(b);
  switch (op) {
    case BPPP_FE_ADD: return fr_to_fe(fr_add(x, y));
    case BPPP_FE_SUB: return fr_to_fe(fr_sub<1>(x, y));
    case BPPP_FE_MUL: return fr_to_fe(fr_mul(x, y));
    case BPPP_FE_SQR: return fr_to_fe(fr_sqr(x));
    case 6: {                                                 // (8a) * (-7b): both operands at the magnitude-8 bound of fr_mul
      fr x8 = fr_mul_int(x, 8), y8 = fr_neg<7>(fr_mul_int(y, 7));
      return fr_to_fe(fr_mul(x8, y8));
    }
    case 10: {                                                // (8a)^2 through fr_sqr's doubled operand (a2 = a << 1 < 2^31)
      return fr_to_fe(fr_sqr(fr_mul_int(x, 8)));
    }
    case 11: {                                                // magnitude 16 into fr_normalize: 8a - 7b with sub<7>, result magnitude 16
      return fr_to_fe(fr_sub<7>(fr_mul_int(x, 8), fr_mul_int(y, 7)));
    }
    case 12: {                                                // the reduced linear operations, chained: ((a + b) - 2b) + (-a) + 2a = a - b + ... = 2a - b
      fr t = fr_subr(fr_addr(x, y), fr_dblr(y));             // a - b
      return fr_to_fe(fr_addr(fr_addr(t, fr_negr(x)), fr_dblr(x)));   // a - b - a + 2a = 2a - b
    }
    case 13: return fr_to_fe(fr_weak(fr_mul_int(x, 16)));    // one weak pass from magnitude 16, then normalise: 16a
    case 14: return fe{{(uint32_t)fr_is_zero(fr_sub<7>(fr_mul_int(x, 8), fr_mul_int(y, 7))), 0, 0, 0, 0, 0, 0, 0}};   // 8a == 7b ? (magnitude 16)
    default: return fr_to_fe(fr_neg<1>(x));
  }
}
__global__ void k_test_fe(int op, int mod, const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe x = fe_load(a + (size_t)i * 8), y = fe_load(b + (size_t)i * 8);
  fe r;
  if (mod == 1) r = apply_op<1>(op, x, y);            // Fr, 8 x 32
  else if (mod == 2) r = apply_op<0>(op, x, y);       // Fq, legacy 8 x 32 code path (cross-check)
  else if (mod == 3) r = apply_op_fr26(op, x, y);     // Fr, production 10 x 26 (fr26.hip.h)
  else if (op == 6) r = apply_mag8_mul(x, y);
  else r = apply_op_fq(op, x, y);                     // Fq, production 10 x 26
  fe_store(out + (size_t)i * 8, r);
}
__global__ void k_test_point(int op, const uint32_t *p, const uint32_t *q, uint32_t n, uint32_t *out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  aff P = aff_load(p + (size_t)i * 16), Q = aff_load(q + (size_t)i * 16);
  xyzz acc = xyzz_from_aff(P);
  if (op == 0) xyzz_madd(acc, Q);
  else if (op == 1) { xyzz t = xyzz_dbl_aff(Q); xyzz_madd(t, aff_cneg(Q, true)); /* t = Q in non-trivial XYZZ form */ xyzz_add(acc, t); }
  else acc = xyzz_dbl(xyzz_dbl_aff(P));  // 4P via both doubling forms
  aff_store(out + (size_t)i * 16, xyzz_to_aff(acc));
}
// the quad forms (ec_quad.hip.h) against the one-lane forms: one quad per element, the scalar routine on every lane beside it
BPPP_DI xyzz test_xyzz_of(const aff &P, bool bounds) {
  xyzz t = xyzz_dbl_aff(P);                       // 2P - P: P with ZZ != 1
  xyzz_madd(t, aff_cneg(P, true));
  if (bounds) {                                   // the same point with every X limb near magnitude 5 and every Y limb near 3
    t.X = fq_sub<3>(fq_normalize(t.X), fq_zero());
    t.Y = fq_sub<1>(fq_normalize(t.Y), fq_zero());
  }
  return t;
}
BPPP_DI uint32_t quad_or(uint32_t v) {          // OR over the quad, through the same pinned broadcasts as the point operations
  fq t = fq_zero();
  t.n[0] = v;
  return fq_quad_bcast<0>(t).n[0] | fq_quad_bcast<1>(t).n[0] | fq_quad_bcast<2>(t).n[0] | fq_quad_bcast<3>(t).n[0];
}
__global__ void __launch_bounds__(64) k_test_point_quad(int op, const uint32_t *p, const uint32_t *q, uint32_t n, uint32_t *out, uint32_t *raw) {
  const uint32_t i = (blockIdx.x * 64 + threadIdx.x) >> 2;
  const bool valid = i < n, bounds = (op & 1) != 0;
  xyzz A = xyzz_inf(), B = xyzz_inf();           // a quad past the end adds infinity: every quad takes part in the exchanges
  if (valid) { A = test_xyzz_of(aff_load(p + (size_t)i * 16), bounds); B = test_xyzz_of(aff_load(q + (size_t)i * 16), bounds); }
  xyzz s = A, r = A;
  if (op & 4) {                                    // the forms on fq_mul_lone (k_reduce_tail_quad's)
    if ((op & 3) < 2) { xyzz_add(s, B); xyzz_add_quad<true>(r, B); }
    else { s = xyzz_dbl(A); xyzz_dbl_quad<true>(r); }
  } else if (op < 2) { xyzz_add(s, B); xyzz_add_quad(r, B); }
  else { s = xyzz_dbl(A); xyzz_dbl_quad(r); }
  // do the four lanes of the quad hold the same limbs?
  uint32_t d = 0;
  const xyzz r0 = { fq_quad_bcast<0>(r.X), fq_quad_bcast<0>(r.Y), fq_quad_bcast<0>(r.ZZ), fq_quad_bcast<0>(r.ZZZ) };
#pragma unroll
  for (int k = 0; k < 10; k++) d |= (r.X.n[k] ^ r0.X.n[k]) | (r.Y.n[k] ^ r0.Y.n[k]) | (r.ZZ.n[k] ^ r0.ZZ.n[k]) | (r.ZZZ.n[k] ^ r0.ZZZ.n[k]);
  d = quad_or(d);
  if (valid && (threadIdx.x & 3u) == 0) {
    uint32_t *o = raw + (size_t)i * 81;
#pragma unroll
    for (int k = 0; k < 10; k++) {
      o[k] = r.X.n[k]; o[10 + k] = r.Y.n[k]; o[20 + k] = r.ZZ.n[k]; o[30 + k] = r.ZZZ.n[k];
      o[40 + k] = s.X.n[k]; o[50 + k] = s.Y.n[k]; o[60 + k] = s.ZZ.n[k]; o[70 + k] = s.ZZZ.n[k];
    }
    o[80] = d == 0 ? 1u : 0u;
    aff_store(out + (size_t)i * 16, xyzz_to_aff(r));
  }
}
// the pair forms of fq26.hip.h against fq_mul / fq_sqr on raw limbs (any magnitude <= 8 the caller builds): per element 40 words,
// pair r1, pair r2, one-product r1, one-product r2.  kind 0: (a b, c d)  1: (a b, c^2)  2: (a^2, c^2)
__global__ void __launch_bounds__(64) k_test_fq_pair(int kind, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t n, uint32_t *raw) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const fq A = fq_load10(a + (size_t)i * 10), B = fq_load10(b + (size_t)i * 10), Cc = fq_load10(c + (size_t)i * 10), D = fq_load10(d + (size_t)i * 10);
  fq r1, r2, s1, s2;
  if (kind == 0) { fq_mul2(A, B, Cc, D, r1, r2); s1 = fq_mul(A, B); s2 = fq_mul(Cc, D); }
  else if (kind == 1) { fq_mul_sqr(A, B, Cc, r1, r2); s1 = fq_mul(A, B); s2 = fq_sqr(Cc); }
  else { fq_sqr2(A, Cc, r1, r2); s1 = fq_sqr(A); s2 = fq_sqr(Cc); }
  uint32_t *o = raw + (size_t)i * 40;
  fq_store10(o, r1); fq_store10(o + 10, r2); fq_store10(o + 20, s1); fq_store10(o + 30, s2);
}
// xyzz_add_chain / xyzz_dbl_chain against xyzz_add / xyzz_dbl, one lane per element.  op bit 0: the left operand is 3 p[i] built as a sum
// of three points (ZZ != 1) instead of p[i] with ZZ = 1; bit 1: the same for the right operand; bit 2: doubling of the left operand
__global__ void __launch_bounds__(64) k_test_point_chain(int op, const uint32_t *p, const uint32_t *q, uint32_t n, uint32_t *out, uint32_t *raw) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const aff P = aff_load(p + (size_t)i * 16), Q = aff_load(q + (size_t)i * 16);
  xyzz A = xyzz_from_aff(P), B = xyzz_from_aff(Q);
  if (op & 1) { A = xyzz_dbl_aff(P); xyzz_madd(A, P); }
  if (op & 2) { B = xyzz_dbl_aff(Q); xyzz_madd(B, Q); }
  xyzz r = A, s = A;
  if (op & 4) { r = xyzz_dbl_chain(A); s = xyzz_dbl(A); }
  else { xyzz_add_chain(r, B); xyzz_add(s, B); }
  uint32_t *o = raw + (size_t)i * 80;
  xyzz_store(o, r); xyzz_store(o + 40, s);
  aff_store(out + (size_t)i * 16, xyzz_to_aff(r));
}
// fq29.hip.h on raw limbs (n x 9 words each, the caller keeps to the magnitude contract).  op 0: a b, 1: a^2, 2: weak_pass(sub<3>(a, b)),
// 3: from_fe of the canonical 8 x 32 value in a's first 8 words.  raw: the 9 result limbs, then the 10 limbs of fq29_to_fq26(result);
// out: that value canonical, 8 words
__global__ void __launch_bounds__(64) k_test_fq29(int op, const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *raw, uint32_t *out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const fq29 A = fq29_load9(a + (size_t)i * 9), B = fq29_load9(b + (size_t)i * 9);
  fq29 r;
  if (op == 0) r = fq29_mul(A, B);
  else if (op == 1) r = fq29_sqr(A);
  else if (op == 2) r = fq29_weak_pass(fq29_sub<3>(A, B));
  else { fe v; for (int k = 0; k < 8; k++) v.v[k] = A.n[k]; r = fq29_from_fe(v); }
  const fq t = fq29_to_fq26(r);
  fq29_store9(raw + (size_t)i * 19, r);
  fq_store10(raw + (size_t)i * 19 + 9, t);
  fe_store(out + (size_t)i * 8, fq_to_fe(t));
}
// one chain of k mixed additions per lane, as k_acc_points_sized29 walks an item: the first point is loaded into the accumulator, the others
// are added with xyzz29_madd; flags[j] != 0 negates point j (the sign fold).  raw: the 40 stored words of the sum (xyzz29_to_xyzz)
__global__ void __launch_bounds__(64) k_test_madd29_chain(const uint32_t *pts, const uint32_t *flags, uint32_t k, uint32_t n, uint32_t *out, uint32_t *raw) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t *p = pts + (size_t)i * k * 16, *f = flags + (size_t)i * k;
  xyzz29 acc = xyzz29_from_aff(aff29_cneg(aff29_load(p), f[0] != 0));
  for (uint32_t j = 1; j < k; j++) xyzz29_madd(acc, aff29_cneg(aff29_load(p + (size_t)j * 16), f[j] != 0));
  const xyzz s = xyzz29_to_xyzz(acc);
  xyzz_store(raw + (size_t)i * XYZZ_WORDS, s);
  aff_store(out + (size_t)i * 16, xyzz_to_aff(s));
}
// fq29_mul_add2, xyzz29_madd_fast and xyzz29_from_two on raw limbs.  op 0: mul_add2 of 4 elements, 1: madd_fast of X Y ZZ ZZZ x y, 2: from_two of
// x1 y1 x2 y2; raw: 36 words per element,
// the result's limbs (op 0: the first 9)
__global__ void __launch_bounds__(64) k_test_ec29_fast(int op, const uint32_t *in, uint32_t n, uint32_t *raw) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t *p = in + (size_t)i * (op == 1 ? 54 : 36);
  uint32_t *o = raw + (size_t)i * 36;
  xyzz29 r = xyzz29_inf();
  if (op == 0) r.X = fq29_mul_add2(fq29_load9(p), fq29_load9(p + 9), fq29_load9(p + 18), fq29_load9(p + 27));
  else if (op == 1) {
    r.X = fq29_load9(p); r.Y = fq29_load9(p + 9); r.ZZ = fq29_load9(p + 18); r.ZZZ = fq29_load9(p + 27);
    aff29 q; q.x = fq29_load9(p + 36); q.y = fq29_load9(p + 45);
    xyzz29_madd_fast(r, q);
  } else {
    aff29 a, b; a.x = fq29_load9(p); a.y = fq29_load9(p + 9); b.x = fq29_load9(p + 18); b.y = fq29_load9(p + 27);
    r = xyzz29_from_two(a, b);
  }
  fq29_store9(o, r.X); fq29_store9(o + 9, r.Y); fq29_store9(o + 18, r.ZZ); fq29_store9(o + 27, r.ZZZ);
}
// the same walk over 10 x 26-bit limbs, as k_acc_points_sized walks an item (and, from the second entry on, k_acc_points a run): xyzz_from_aff,
// aff_cneg, xyzz_madd
__global__ void __launch_bounds__(64) k_test_madd26_chain(const uint32_t *pts, const uint32_t *flags, uint32_t k, uint32_t n, uint32_t *out, uint32_t *raw) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t *p = pts + (size_t)i * k * 16, *f = flags + (size_t)i * k;
  xyzz acc = xyzz_from_aff(aff_cneg(aff_load(p), f[0] != 0));
  for (uint32_t j = 1; j < k; j++) xyzz_madd(acc, aff_cneg(aff_load(p + (size_t)j * 16), f[j] != 0));
  xyzz_store(raw + (size_t)i * XYZZ_WORDS, acc);
  aff_store(out + (size_t)i * 16, xyzz_to_aff(acc));
}
// the bucket array of an MSM as canonical affine points, infinity as (0, 0): one lane per bucket
__global__ void __launch_bounds__(64) k_test_buckets_aff(const uint32_t *__restrict__ buckets, uint64_t FB, uint32_t *__restrict__ out) {
  const uint64_t fb = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (fb >= FB) return;
  aff_store(out + fb * 16, xyzz_to_aff(xyzz_load(buckets + fb * XYZZ_WORDS)));
}
}  // namespace bppp

using namespace bppp;

static int run2(bppp_ctx *ctx, const uint64_t *a, const uint64_t *b, size_t n, size_t words, uint64_t *out, void **da, void **db, void **dout) {
  size_t bytes = n * words * 8;
  BPPP_HIP(ctx, hipMalloc(da, bytes)); BPPP_HIP(ctx, hipMalloc(db, bytes)); BPPP_HIP(ctx, hipMalloc(dout, bytes));
  BPPP_HIP(ctx, hipMemcpyAsync(*da, a, bytes, hipMemcpyHostToDevice, ctx->stream));
  BPPP_HIP(ctx, hipMemcpyAsync(*db, b, bytes, hipMemcpyHostToDevice, ctx->stream));
  (void)out;
  return BPPP_OK;
}

extern "C" int bppp_test_fe_op(bppp_ctx *ctx, int op, int modulus, const uint64_t *a, const uint64_t *b, size_t n, uint64_t *out) {
  if (!ctx || !a || !b || !out) return BPPP_ERR_ARG;
  if (n == 0) return BPPP_OK;
  hipSetDevice(ctx->device);
  void *da = nullptr, *db = nullptr, *dout = nullptr;
  int rc = run2(ctx, a, b, n, 4, out, &da, &db, &dout);
  if (!rc) {
    k_test_fe<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream>>>(op, modulus, (const uint32_t *)da, (const uint32_t *)db, (uint32_t)n, (uint32_t *)dout);
    if (hipMemcpyAsync(out, dout, n * 32, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
      rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_fe_op: kernel or copy failed");
  }
  hipFree(da); hipFree(db); hipFree(dout);
  return rc;
}
extern "C" int bppp_test_point_op(bppp_ctx *ctx, int op, const uint64_t *p, const uint64_t *q, size_t n, uint64_t *out) {
  if (!ctx || !p || !q || !out) return BPPP_ERR_ARG;
  if (n == 0) return BPPP_OK;
  hipSetDevice(ctx->device);
  void *da = nullptr, *db = nullptr, *dout = nullptr;
  int rc = run2(ctx, p, q, n, 8, out, &da, &db, &dout);
  if (!rc) {
    k_test_point<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream>>>(op, (const uint32_t *)da, (const uint32_t *)db, (uint32_t)n, (uint32_t *)dout);
    if (hipMemcpyAsync(out, dout, n * 64, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
      rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_point_op: kernel or copy failed");
  }
  hipFree(da); hipFree(db); hipFree(dout);
  return rc;
}
extern "C" int bppp_test_point_quad(bppp_ctx *ctx, int op, const uint64_t *p, const uint64_t *q, size_t n, uint64_t *out, uint32_t *raw) {
  if (!ctx || !p || !q || !out || !raw || op < 0 || op > 7) return BPPP_ERR_ARG;
  if (n == 0) return BPPP_OK;
  hipSetDevice(ctx->device);
  void *da = nullptr, *db = nullptr, *dout = nullptr, *draw = nullptr;
  int rc = run2(ctx, p, q, n, 8, out, &da, &db, &dout);
  if (!rc && hipMalloc(&draw, n * 81 * 4) != hipSuccess) rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_point_quad: hipMalloc");
  if (!rc) {
    k_test_point_quad<<<dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, ctx->stream>>>(op, (const uint32_t *)da, (const uint32_t *)db, (uint32_t)n, (uint32_t *)dout,
                                                                                        (uint32_t *)draw);
    if (hipMemcpyAsync(out, dout, n * 64, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(raw, draw, n * 81 * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
      rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_point_quad: kernel or copy failed");
  }
  hipFree(da); hipFree(db); hipFree(dout); hipFree(draw);
  return rc;
}
extern "C" int bppp_test_fq_pair(bppp_ctx *ctx, int kind, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, size_t n, uint32_t *raw) {
  if (!ctx || !a || !b || !c || !d || !raw || kind < 0 || kind > 2) return BPPP_ERR_ARG;
  if (n == 0) return BPPP_OK;
  hipSetDevice(ctx->device);
  uint32_t *din = nullptr, *draw = nullptr;
  const size_t words = n * 10;
  if (hipMalloc(&din, 4 * words * 4) != hipSuccess || hipMalloc(&draw, n * 40 * 4) != hipSuccess) { hipFree(din); return bppp::fail(ctx, BPPP_ERR_HIP, "test_fq_pair: hipMalloc"); }
  const uint32_t *src[4] = {a, b, c, d};
  int rc = BPPP_OK;
  for (int k = 0; k < 4 && !rc; k++)
    if (hipMemcpyAsync(din + k * words, src[k], words * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_fq_pair: copy failed");
  if (!rc) {
    k_test_fq_pair<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream>>>(kind, din, din + words, din + 2 * words, din + 3 * words, (uint32_t)n, draw);
    if (hipMemcpyAsync(raw, draw, n * 40 * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
      rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_fq_pair: kernel or copy failed");
  }
  hipFree(din); hipFree(draw);
  return rc;
}
extern "C" int bppp_test_point_chain(bppp_ctx *ctx, int op, const uint64_t *p, const uint64_t *q, size_t n, uint64_t *out, uint32_t *raw) {
  if (!ctx || !p || !q || !out || !raw || op < 0 || op > 7) return BPPP_ERR_ARG;
  if (n == 0) return BPPP_OK;
  hipSetDevice(ctx->device);
  void *da = nullptr, *db = nullptr, *dout = nullptr, *draw = nullptr;
  int rc = run2(ctx, p, q, n, 8, out, &da, &db, &dout);
  if (!rc && hipMalloc(&draw, n * 80 * 4) != hipSuccess) rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_point_chain: hipMalloc");
  if (!rc) {
    k_test_point_chain<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream>>>(op, (const uint32_t *)da, (const uint32_t *)db, (uint32_t)n, (uint32_t *)dout, (uint32_t *)draw);
    if (hipMemcpyAsync(out, dout, n * 64, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(raw, draw, n * 80 * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
      rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_point_chain: kernel or copy failed");
  }
  hipFree(da); hipFree(db); hipFree(dout); hipFree(draw);
  return rc;
}

// ---- measured VALU ceiling for the field layer: independent fq_mul chains, 8 waves per SIMD, nothing but multiplies.
// bench.py reports the accumulate kernel's modular-multiplication rate as a fraction of this.
namespace bppp {
__global__ void __launch_bounds__(256) k_mulmod_rate(const uint32_t *__restrict__ seed, int iters, uint32_t *__restrict__ sink) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  fq a[4], b;
  for (int k = 0; k < 4; k++) a[k] = fq_from_fe(fe_load(seed + (size_t)((t + 17 * k) & 1023) * 8));
  b = fq_from_fe(fe_load(seed + (size_t)((t * 7 + 3) & 1023) * 8));
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = fq_mul(a[k], b);
  }
  fq r = fq_add(fq_add(a[0], a[1]), fq_add(a[2], a[3]));
  uint32_t x = 0;
  for (int i = 0; i < 10; i++) x ^= r.n[i];
  if (x == 0x12345u) sink[t & 63] = x;       // keeps the chains live; practically never taken
}
}  // namespace bppp
extern "C" int bppp_test_mulmod_rate(bppp_ctx *ctx, int iters, double *mulmods_per_sec) {
  if (!ctx || !mulmods_per_sec || iters < 1) return BPPP_ERR_ARG;
  hipSetDevice(ctx->device);
  uint32_t *seed = nullptr, *sink = nullptr;
  if (hipMalloc(&seed, 1024 * 32) != hipSuccess || hipMalloc(&sink, 256) != hipSuccess) { hipFree(seed); return bppp::fail(ctx, BPPP_ERR_HIP, "mulmod_rate: hipMalloc"); }
  std::vector<uint32_t> h(1024 * 8);
  uint64_t z = 0x9E3779B97F4A7C15ull;
  for (auto &w : h) { z ^= z << 13; z ^= z >> 7; z ^= z << 17; w = (uint32_t)(z >> 16); }
  for (int i = 0; i < 1024; i++) h[8 * i + 7] &= 0x7FFFFFFFu;      // < p
  hipMemcpy(seed, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  hipMemset(sink, 0, 256);
  const int blocks = 256 * 4 * 8 / 4 * 2;     // 8 waves per SIMD on 256 CUs, two rounds of them
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  bppp::k_mulmod_rate<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(seed, 8, sink);          // warm-up
  hipEventRecord(e0, ctx->stream);
  bppp::k_mulmod_rate<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(seed, iters, sink);
  hipEventRecord(e1, ctx->stream);
  int rc = BPPP_OK;
  if (hipEventSynchronize(e1) != hipSuccess) rc = bppp::fail(ctx, BPPP_ERR_HIP, "mulmod_rate: kernel failed");
  float ms = 0; hipEventElapsedTime(&ms, e0, e1);
  *mulmods_per_sec = ms > 0 ? (double)blocks * 256.0 * 4.0 * iters / (ms * 1e-3) : 0.0;
  hipEventDestroy(e0); hipEventDestroy(e1); hipFree(seed); hipFree(sink);
  return rc;
}

extern "C" int bppp_test_last_mixed_msm_terms(bppp_ctx *ctx, uint64_t *terms) {
  if (!ctx || !terms) return BPPP_ERR_ARG;
  *terms = ctx->last_mixed_terms;
  return BPPP_OK;
}

extern "C" int bppp_test_last_sort_ranges(bppp_ctx *ctx, int *q) {
  if (!ctx || !q) return BPPP_ERR_ARG;
  *q = ctx->last_sort_ranges;
  return BPPP_OK;
}

extern "C" int bppp_test_last_scatter_one_read(bppp_ctx *ctx, int *one_read) {
  if (!ctx || !one_read) return BPPP_ERR_ARG;
  *one_read = ctx->last_scatter_one_read;
  return BPPP_OK;
}

extern "C" int bppp_test_last_hist16(bppp_ctx *ctx, int *hist16) {
  if (!ctx || !hist16) return BPPP_ERR_ARG;
  *hist16 = ctx->last_hist16;
  return BPPP_OK;
}

extern "C" int bppp_test_last_acc_sized(bppp_ctx *ctx, int *sized) {
  if (!ctx || !sized) return BPPP_ERR_ARG;
  *sized = ctx->last_acc_sized;
  return BPPP_OK;
}

extern "C" int bppp_test_last_acc_fq29(bppp_ctx *ctx, int *fq29) {
  if (!ctx || !fq29) return BPPP_ERR_ARG;
  *fq29 = ctx->last_acc_fq29;
  return BPPP_OK;
}

extern "C" int bppp_test_fq29_op(bppp_ctx *ctx, int op, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *raw, uint32_t *out) {
  if (!ctx || !a || !b || !raw || !out || op < 0 || op > 3 || n >= (1u << 24)) return BPPP_ERR_ARG;
  if (n == 0) return BPPP_OK;
  hipSetDevice(ctx->device);
  uint32_t *d = nullptr;                       // a | b | raw | out
  if (hipMalloc(&d, n * (9 + 9 + 19 + 8) * 4) != hipSuccess) return bppp::fail(ctx, BPPP_ERR_HIP, "test_fq29_op: hipMalloc");
  uint32_t *d_b = d + n * 9, *d_raw = d_b + n * 9, *d_out = d_raw + n * 19;
  hipStream_t st = ctx->stream;
  bool ok = hipMemcpyAsync(d, a, n * 36, hipMemcpyHostToDevice, st) == hipSuccess && hipMemcpyAsync(d_b, b, n * 36, hipMemcpyHostToDevice, st) == hipSuccess;
  if (ok) k_test_fq29<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st>>>(op, d, d_b, (uint32_t)n, d_raw, d_out);
  ok = ok && hipMemcpyAsync(raw, d_raw, n * 19 * 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipMemcpyAsync(out, d_out, n * 32, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (hipStreamSynchronize(st) != hipSuccess) ok = false;
  hipFree(d);
  return ok ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_fq29_op: kernel or copy failed");
}
extern "C" int bppp_test_ec29_fast_op(bppp_ctx *ctx, int op, const uint32_t *in, size_t n, uint32_t *raw) {
  if (!ctx || !in || !raw || op < 0 || op > 2 || n >= (1u << 24)) return BPPP_ERR_ARG;
  if (n == 0) return BPPP_OK;
  hipSetDevice(ctx->device);
  const size_t win = n * (op == 1 ? 54 : 36), wout = n * 36;
  uint32_t *d = nullptr;                       // in | raw
  if (hipMalloc(&d, (win + wout) * 4) != hipSuccess) return bppp::fail(ctx, BPPP_ERR_HIP, "test_ec29_fast_op: hipMalloc");
  hipStream_t st = ctx->stream;
  bool ok = hipMemcpyAsync(d, in, win * 4, hipMemcpyHostToDevice, st) == hipSuccess;
  if (ok) k_test_ec29_fast<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st>>>(op, d, (uint32_t)n, d + win);
  ok = ok && hipMemcpyAsync(raw, d + win, wout * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (hipStreamSynchronize(st) != hipSuccess) ok = false;
  hipFree(d);
  return ok ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_ec29_fast_op: kernel or copy failed");
}
static int madd_chain(bppp_ctx *ctx, bool fq29, const uint64_t *points, const uint32_t *flags, size_t k, size_t n, uint64_t *out, uint32_t *raw) {
  if (!ctx || !points || !flags || !out || !raw || !k || k >= (1u << 16) || n >= (1u << 16)) return BPPP_ERR_ARG;
  if (n == 0) return BPPP_OK;
  hipSetDevice(ctx->device);
  uint32_t *d = nullptr;                       // points | flags | out | raw
  if (hipMalloc(&d, (n * k * 17 + n * (16 + XYZZ_WORDS)) * 4) != hipSuccess) return bppp::fail(ctx, BPPP_ERR_HIP, "test_madd_chain: hipMalloc");
  uint32_t *d_f = d + n * k * 16, *d_out = d_f + n * k, *d_raw = d_out + n * 16;
  hipStream_t st = ctx->stream;
  bool ok = hipMemcpyAsync(d, points, n * k * 64, hipMemcpyHostToDevice, st) == hipSuccess && hipMemcpyAsync(d_f, flags, n * k * 4, hipMemcpyHostToDevice, st) == hipSuccess;
  if (ok && fq29) k_test_madd29_chain<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st>>>(d, d_f, (uint32_t)k, (uint32_t)n, d_out, d_raw);
  else if (ok) k_test_madd26_chain<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st>>>(d, d_f, (uint32_t)k, (uint32_t)n, d_out, d_raw);
  ok = ok && hipMemcpyAsync(out, d_out, n * 64, hipMemcpyDeviceToHost, st) == hipSuccess && hipMemcpyAsync(raw, d_raw, n * XYZZ_WORDS * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (hipStreamSynchronize(st) != hipSuccess) ok = false;
  hipFree(d);
  return ok ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_madd_chain: kernel or copy failed");
}
extern "C" int bppp_test_madd29_chain(bppp_ctx *ctx, const uint64_t *points, const uint32_t *flags, size_t k, size_t n, uint64_t *out, uint32_t *raw) {
  return madd_chain(ctx, true, points, flags, k, n, out, raw);
}
extern "C" int bppp_test_madd26_chain(bppp_ctx *ctx, const uint64_t *points, const uint32_t *flags, size_t k, size_t n, uint64_t *out, uint32_t *raw) {
  return madd_chain(ctx, false, points, flags, k, n, out, raw);
}

// ---- the stages of the last general-pipeline MSM on a context, read back from its workspace (ctx.hpp: last_msm_*)
static bool last_msm_total(bppp_ctx *ctx, const MsmWorkspace &ws, uint64_t FB, uint32_t *total) {
  return hipStreamSynchronize(ctx->stream) == hipSuccess && hipMemcpy(total, ws.start + FB, 4, hipMemcpyDeviceToHost) == hipSuccess;
}
extern "C" int bppp_test_last_msm_layout(bppp_ctx *ctx, bppp_test_msm_layout *r) {
  if (!ctx || !r) return BPPP_ERR_ARG;
  if (!ctx->last_msm_valid) return bppp::fail(ctx, BPPP_ERR_ARG, "test_last_msm_layout: no general-pipeline MSM has run on this context");
  hipSetDevice(ctx->device);
  const MsmPlan &p = ctx->last_msm_plan;
  const size_t n = ctx->last_msm_n, batch = ctx->last_msm_batch;
  Carver cv(ctx->ws, ctx->ws_bytes);
  const MsmWorkspace ws = carve(cv, p, n, batch);
  if (cv.off > ctx->ws_bytes) return bppp::fail(ctx, BPPP_ERR_ARG, "test_last_msm_layout: the workspace is smaller than the stored plan's layout");
  uint32_t total = 0;
  if (!last_msm_total(ctx, ws, p.FB, &total)) return bppp::fail(ctx, BPPP_ERR_HIP, "test_last_msm_layout: copy failed");
  memset(r, 0, sizeof *r);
  r->c = p.c; r->W = p.W; r->acnt = p.acnt; r->top = p.top; r->M = p.M; r->flat = p.flat ? 1 : 0; r->CH = p.CH; r->Q = p.Q; r->one_read = p.one_read ? 1 : 0;
  r->sized = p.sized ? 1 : 0; r->fq29 = p.fq29 ? 1 : 0; r->acc_fast = p.acc_fast ? 1 : 0; r->L = p.L; r->shared_points = ctx->last_msm_shared_points;
  r->stride = ws.stride;
  r->per = ((((uint32_t)n + p.CH - 1) / p.CH) + 7u) & ~7u;      // the chunk length of k_hist and the three scatters
  r->batch = batch; r->n = n; r->FB = p.FB; r->G = p.G; r->total = total; r->table_stride = ctx->last_msm_table_stride;
  return BPPP_OK;
}
extern "C" int bppp_test_last_msm_copy(bppp_ctx *ctx, int what, void *out, size_t bytes) {
  if (!ctx || !out) return BPPP_ERR_ARG;
  if (!ctx->last_msm_valid) return bppp::fail(ctx, BPPP_ERR_ARG, "test_last_msm_copy: no general-pipeline MSM has run on this context");
  hipSetDevice(ctx->device);
  const MsmPlan &p = ctx->last_msm_plan;
  const size_t n = ctx->last_msm_n, batch = ctx->last_msm_batch;
  Carver cv(ctx->ws, ctx->ws_bytes);
  const MsmWorkspace ws = carve(cv, p, n, batch);
  if (cv.off > ctx->ws_bytes) return bppp::fail(ctx, BPPP_ERR_ARG, "test_last_msm_copy: the workspace is smaller than the stored plan's layout");
  uint32_t total = 0;
  if (!last_msm_total(ctx, ws, p.FB, &total)) return bppp::fail(ctx, BPPP_ERR_HIP, "test_last_msm_copy: copy failed");
  const void *src = nullptr; size_t want = 0;
  switch (what) {
    case BPPP_TEST_MSM_DIGITS: src = ws.dig; want = (size_t)p.NB * ws.stride * 2; break;
    case BPPP_TEST_MSM_NEGMASK: src = ws.negmask; want = ((batch * n + 63) / 64) * 8; break;
    case BPPP_TEST_MSM_COUNT: src = ws.count; want = (size_t)p.FB * 4; break;
    case BPPP_TEST_MSM_START: src = ws.start; want = ((size_t)p.FB + 1) * 4; break;
    case BPPP_TEST_MSM_SORTED: src = ws.sorted; want = (size_t)total * 4; break;
    case BPPP_TEST_MSM_BUCKETS_RAW: src = ws.buckets; want = (size_t)p.FB * XYZZ_WORDS * 4; break;
    case BPPP_TEST_MSM_BUCKETS_AFF: want = (size_t)p.FB * 64; break;
    default: return bppp::fail(ctx, BPPP_ERR_ARG, "test_last_msm_copy: unknown array");
  }
  if (bytes != want) return bppp::fail(ctx, BPPP_ERR_ARG, "test_last_msm_copy: the array has " + std::to_string(want) + " bytes, not " + std::to_string(bytes));
  if (!want) return BPPP_OK;
  uint32_t *d_aff = nullptr;
  if (what == BPPP_TEST_MSM_BUCKETS_AFF) {
    if (hipMalloc(&d_aff, want) != hipSuccess) return bppp::fail(ctx, BPPP_ERR_HIP, "test_last_msm_copy: hipMalloc");
    k_test_buckets_aff<<<dim3((unsigned)((p.FB + 63) / 64)), dim3(64), 0, ctx->stream>>>(ws.buckets, p.FB, d_aff);
    src = d_aff;
  }
  const bool ok = hipMemcpyAsync(out, src, want, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
  hipFree(d_aff);
  return ok ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_last_msm_copy: kernel or copy failed");
}

extern "C" int bppp_test_last_windows(bppp_ctx *ctx, int *windows) {
  if (!ctx || !windows) return BPPP_ERR_ARG;
  *windows = ctx->last_windows;
  return BPPP_OK;
}

extern "C" int bppp_test_rp_last_verify_counts(bppp_rp *rp, uint64_t *combined_msms, uint64_t *each_passes) {
  if (!rp || !combined_msms || !each_passes) return BPPP_ERR_ARG;
  *combined_msms = rp->n_combined;
  *each_passes = rp->n_each;
  return BPPP_OK;
}

extern "C" int bppp_test_rp_last_block_counts(bppp_rp *rp, uint64_t *msms, uint64_t *terms, uint64_t *key_lifts, uint64_t *coms_decoded) {
  if (!rp || !msms || !terms || !key_lifts || !coms_decoded) return BPPP_ERR_ARG;
  *msms = rp->blk_msms; *terms = rp->blk_terms; *key_lifts = rp->blk_key_lifts; *coms_decoded = rp->blk_coms;
  return BPPP_OK;
}

extern "C" int bppp_test_rp_set_each_chunk(bppp_rp *rp, size_t proofs) {
  if (!rp || (proofs && proofs < 8)) return BPPP_ERR_ARG;
  rp->each_chunk = proofs;
  return BPPP_OK;
}

extern "C" int bppp_test_rp_set_tally_short_max(bppp_rp *rp, size_t entries) {
  if (!rp) return BPPP_ERR_ARG;
  rp->tally_short_max = entries ? entries : bppp_rp().tally_short_max;
  return BPPP_OK;
}
extern "C" int bppp_test_rp_set_tally_piece(bppp_rp *rp, size_t entries) {
  if (!rp || entries == 1) return BPPP_ERR_ARG;
  rp->tally_piece = entries ? entries : bppp_rp().tally_piece;
  return BPPP_OK;
}
extern "C" int bppp_test_rp_set_tally_chunk(bppp_rp *rp, size_t entries) {
  if (!rp) return BPPP_ERR_ARG;
  rp->tally_chunk = entries ? entries : bppp_rp().tally_chunk;
  return BPPP_OK;
}
extern "C" int bppp_test_rp_set_flat_chunk(bppp_rp *rp, size_t items) {
  if (!rp) return BPPP_ERR_ARG;
  rp->flat_chunk = items ? items : bppp_rp().flat_chunk;
  return BPPP_OK;
}
extern "C" int bppp_test_rp_cut_through_force(bppp_rp *rp, int mode, const uint8_t *salt, int table_bits) {
  if (!rp || mode < 0 || mode > 1 || table_bits < 0 || table_bits > 32) return BPPP_ERR_ARG;
  rp->cut_same_hash = mode == 1;
  rp->cut_salt_pinned = salt != nullptr;
  if (salt) memcpy(rp->cut_salt, salt, 16); else memset(rp->cut_salt, 0, 16);
  rp->cut_table_bits = table_bits;
  return BPPP_OK;
}
extern "C" int bppp_test_rp_cut_through_last(bppp_rp *rp, uint64_t *slots, uint64_t *groups, uint64_t *passes) {
  if (!rp || !slots || !groups || !passes) return BPPP_ERR_ARG;
  *slots = rp->cut_slots; *groups = rp->cut_groups; *passes = rp->cut_passes;
  return BPPP_OK;
}

// one quad per instance; all four lanes hold the product, lane 0 of the quad inverts and stores
namespace bppp {
__global__ void __launch_bounds__(64) k_test_excess_mul(uint32_t n, const uint32_t *__restrict__ sc, const uint32_t *__restrict__ pts, uint32_t *__restrict__ out) {
  const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  if (i >= n) return;
  const xyzz r = excess_mul_quad(fe_load(sc + (size_t)i * 8), aff_load(pts + (size_t)i * 16));
  if (quad_lane() == 0) aff_store(out + (size_t)i * 16, xyzz_to_aff(r));
}
}  // namespace bppp
extern "C" int bppp_test_rp_excess_mul(bppp_rp *rp, size_t n, const void *d_scalars, const void *d_points_xy, void *d_out_xy) {
  if (!rp || !n || n >= (1u << 24) || !d_scalars || !d_points_xy || !d_out_xy) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  hipSetDevice(ctx->device);
  k_test_excess_mul<<<dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, ctx->stream>>>((uint32_t)n, (const uint32_t *)d_scalars, (const uint32_t *)d_points_xy, (uint32_t *)d_out_xy);
  const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
  return ok ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_rp_excess_mul: kernel failed");
}

// the joint walk of k_rp_expart_mulcheck alone: one quad per instance; lane 0 of the quad inverts and stores
namespace bppp {
__global__ void __launch_bounds__(64) k_test_excess_mul2(uint32_t n, const uint32_t *__restrict__ b, const uint32_t *__restrict__ P, const uint32_t *__restrict__ c,
                                                         const uint32_t *__restrict__ Q, uint32_t *__restrict__ out) {
  const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  if (i >= n) return;
  const xyzz r = excess_mul2_quad(fe_load(b + (size_t)i * 8), aff_load(P + (size_t)i * 16), fe_load(c + (size_t)i * 8), aff_load(Q + (size_t)i * 16));
  if (quad_lane() == 0) aff_store(out + (size_t)i * 16, xyzz_to_aff(r));
}
}  // namespace bppp
extern "C" int bppp_test_rp_excess_mul2(bppp_rp *rp, size_t n, const void *d_b, const void *d_P_xy, const void *d_c, const void *d_Q_xy, void *d_out_xy) {
  if (!rp || !n || n >= (1u << 24) || !d_b || !d_P_xy || !d_c || !d_Q_xy || !d_out_xy) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  hipSetDevice(ctx->device);
  k_test_excess_mul2<<<dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, ctx->stream>>>((uint32_t)n, (const uint32_t *)d_b, (const uint32_t *)d_P_xy, (const uint32_t *)d_c,
                                                                                       (const uint32_t *)d_Q_xy, (uint32_t *)d_out_xy);
  const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
  return ok ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_rp_excess_mul2: kernel failed");
}

// the fixed-scalar walk of bppp_rp_scan alone: one lane per point, the recoded scalar a kernel argument; a second launch inverts and stores
namespace bppp {
__global__ void __launch_bounds__(64) k_test_scan_mul(uint32_t n, ScanWalk W, const uint32_t *__restrict__ pts, uint32_t *__restrict__ acc) {
  __shared__ ScanTab tab[SCAN_TAB_WORDS];
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  xyzz_store(acc + (size_t)i * XYZZ_WORDS, scan_mul_lane(W, aff_load(pts + (size_t)i * 16), tab, threadIdx.x));
}
__global__ void __launch_bounds__(64) k_test_scan_affine(uint32_t n, const uint32_t *__restrict__ acc, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) scan_affine_lane(acc + (size_t)i * XYZZ_WORDS, out + (size_t)i * 16);
}
}  // namespace bppp
extern "C" int bppp_test_rp_scan_mul(bppp_rp *rp, size_t n, const uint64_t scalar[4], const void *d_points_xy, void *d_out_xy) {
  if (!rp || !n || n >= (1u << 24) || !scalar || !d_points_xy || !d_out_xy) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  ScanWalk W;
  if (!scan_recode(scalar, W)) return bppp::fail(ctx, BPPP_ERR_ARG, "test_rp_scan_mul: the scalar's halves do not fit the walk");
  hipSetDevice(ctx->device);
  uint32_t *acc = nullptr;
  BPPP_HIP(ctx, hipMalloc(&acc, n * XYZZ_WORDS * 4));
  const dim3 grid((unsigned)((n + 63) / 64));
  k_test_scan_mul<<<grid, dim3(64), 0, ctx->stream>>>((uint32_t)n, W, (const uint32_t *)d_points_xy, acc);
  k_test_scan_affine<<<grid, dim3(64), 0, ctx->stream>>>((uint32_t)n, acc, (uint32_t *)d_out_xy);
  const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
  hipFree(acc);
  return ok ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_rp_scan_mul: kernel failed");
}
// the host recoding that walk is driven by: words [0, 9) the two-bit digits, word 9 their number, word 10 the signs of the halves.  Host only.
extern "C" int bppp_test_rp_scan_recode(const uint64_t scalar[4], uint32_t out[11]) {
  ScanWalk W;
  if (!scalar || !out || !scan_recode(scalar, W)) return BPPP_ERR_ARG;
  for (uint32_t k = 0; k < SCAN_DIGIT_WORDS; k++) out[k] = W.d[k];
  out[SCAN_DIGIT_WORDS] = W.nbits; out[SCAN_DIGIT_WORDS + 1] = W.neg;
  return BPPP_OK;
}

// the multi-key walk of bppp_rp_scan_keys alone: the kernels of csrc/rpscan_keys.hip.h themselves — the table of every point once, then per tile of
// keys one walk launch and one launch of the batched affine conversion, which writes the tile's rows of d_out_xy
namespace {
int scan_keys_mul_hook(bppp_rp *rp, size_t nkeys, const uint64_t *scalars, size_t n, const void *d_points_xy, void *d_out_xy) {
  if (!rp || !nkeys || nkeys > BPPP_RP_SCAN_MAX_KEYS || !n || n >= (1u << 24) || !scalars || !d_points_xy || !d_out_xy) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  std::vector<ScanKeyRec> recs(nkeys);
  for (size_t k = 0; k < nkeys; k++)
    if (!scan_keys_recode(scalars + 4 * k, recs[k])) return bppp::fail(ctx, BPPP_ERR_ARG, "test_rp_scan_keys_mul: the scalar's halves do not fit the walk");
  const size_t kt = scan_keys_geometry(rpp_flat_chunk(rp), rp->D.nr, n, nkeys).kt;
  hipSetDevice(ctx->device);
  uint32_t *tab = nullptr, *acc = nullptr, *keys = nullptr;
  bool ok = hipMalloc(&tab, (n + 63) / 64 * 64 * SCANK_TAB_WORDS * 4) == hipSuccess && hipMalloc(&acc, kt * n * XYZZ_WORDS * 4) == hipSuccess &&
            hipMalloc(&keys, kt * sizeof(ScanKeyRec)) == hipSuccess;
  ok = ok && scan_keys_mul_launch(ctx->stream, (uint32_t)n, recs.data(), nkeys, kt, (const uint32_t *)d_points_xy, tab, acc, keys, (uint32_t *)d_out_xy) == hipSuccess;
  ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
  hipFree(tab); hipFree(acc); hipFree(keys);
  return ok ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_rp_scan_keys_mul: kernel failed");
}
}  // namespace
extern "C" int bppp_test_rp_scan_keys_mul(bppp_rp *rp, size_t nkeys, const uint64_t *scalars, size_t n, const void *d_points_xy, void *d_out_xy) {
  return scan_keys_mul_hook(rp, nkeys, scalars, n, d_points_xy, d_out_xy);
}
extern "C" int bppp_test_rp_scan_keys_recode(const uint64_t scalar[4], uint32_t out[36]) {
  ScanKeyRec W;
  if (!scalar || !out || !scan_keys_recode(scalar, W)) return BPPP_ERR_ARG;
  memcpy(out, &W, sizeof W);
  return BPPP_OK;
}
extern "C" int bppp_test_rp_scan_keys_geometry(bppp_rp *rp, size_t rows, size_t nkeys, uint64_t out[3]) {
  if (!rp || !out) return BPPP_ERR_ARG;
  const ScanKeysGeom g = scan_keys_geometry(rpp_flat_chunk(rp), rp->D.nr, rows, nkeys);
  out[0] = g.rows_pass; out[1] = g.kt; out[2] = g.open_chunk;
  return BPPP_OK;
}

extern "C" int bppp_test_rp_witness_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds, const void *d_public_amounts,
                                           uint64_t *in_sc, uint32_t *dig, uint32_t *mul, uint32_t *mss, uint32_t *status) {
  if (!rp || !batch || !d_amounts || !d_blinds || !in_sc || !dig || !status) return BPPP_ERR_ARG;
  const bool binary = rp->st.kind == 1;
  if (!binary && (!d_types || !mul || !mss)) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  hipSetDevice(ctx->device);
  const size_t nr = rp->st.rds.size(), nlen = rp->st.nlen, nmss = binary ? 0 : rp->st.llen - 6, nlive = rp->st.nlive;
  const size_t w_sc = batch * nr * 24, w_dig = batch * nlen, w_mss = batch * nmss + 1, b_bits = batch * nlive + 16;
  uint32_t *d = nullptr;
  BPPP_HIP(ctx, hipMalloc(&d, (w_sc + 2 * w_dig + w_mss + batch) * 4 + b_bits));
  uint32_t *d_sc = d, *d_dig = d_sc + w_sc, *d_mul = d_dig + w_dig, *d_mss = d_mul + w_dig, *d_st = d_mss + w_mss;
  uint8_t *d_bits = (uint8_t *)(d_st + batch);
  std::vector<uint8_t> bits(batch * nlive);
  int rc = wit_launch(rp, batch, d_amounts, d_types, d_blinds, (const uint32_t *)d_public_amounts, d_sc, d_dig, d_mul, d_mss, d_bits, d_st);
  hipStream_t st = ctx->stream;
  bool ok = !rc && hipMemcpyAsync(in_sc, d_sc, w_sc * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
            hipMemcpyAsync(status, d_st, batch * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (ok && binary) ok = !bits.size() || hipMemcpyAsync(bits.data(), d_bits, bits.size(), hipMemcpyDeviceToHost, st) == hipSuccess;
  else if (ok) ok = hipMemcpyAsync(dig, d_dig, w_dig * 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipMemcpyAsync(mul, d_mul, w_dig * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
                    (!nmss || hipMemcpyAsync(mss, d_mss, batch * nmss * 4, hipMemcpyDeviceToHost, st) == hipSuccess);
  if (hipStreamSynchronize(st) != hipSuccess) ok = false;
  if (!rc && !ok) rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_rp_witness_device: kernel or copy failed");
  if (!rc && binary) for (size_t i = 0; i < bits.size(); i++) dig[i] = bits[i];
  hipFree(d);
  return rc;
}

extern "C" int bppp_test_rp_decode_device(bppp_rp *rp, size_t batch, const uint8_t *coms, const uint8_t *proofs, uint64_t *init_pts, uint64_t *resp_pts, uint64_t *wit_norm,
                                          uint64_t *wit_lin, uint32_t *bad, uint32_t *any_bad) {
  if (!rp || !batch || batch >= (1u << 20) || !coms || !proofs || !init_pts || !resp_pts || !wit_norm || !wit_lin || !bad || !any_bad) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const RpDims D = rp->D;
  const size_t B = batch, b_coms = B * D.coms_bytes, b_prf = B * D.proof_bytes, b_init = B * (D.nrp + D.nr) * 64, b_resp = B * 2 * D.k * 64, b_wn = B * D.fn * 32,
               b_wl = B * D.fl * 32, b_bad = (B + 1) * 4;
  auto up256 = [](size_t n) { return (n + 255) & ~(size_t)255; };
  uint8_t *d = nullptr;                      // coms | proofs | init | resp | wit_norm | wit_lin | bad, any_bad  (each 256-byte aligned)
  BPPP_HIP(ctx, hipMalloc(&d, up256(b_coms) + up256(b_prf) + up256(b_init) + up256(b_resp) + up256(b_wn) + up256(b_wl) + up256(b_bad) + 256));
  uint8_t *d_coms = d, *d_prf = d_coms + up256(b_coms), *d_init = d_prf + up256(b_prf), *d_resp = d_init + up256(b_init), *d_wn = d_resp + up256(b_resp),
          *d_wl = d_wn + up256(b_wn), *d_bad = d_wl + up256(b_wl);
  bool ok = hipMemcpyAsync(d_coms, coms, b_coms, hipMemcpyHostToDevice, st) == hipSuccess && hipMemcpyAsync(d_prf, proofs, b_prf, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemsetAsync(d_init, 0xA5, (size_t)(d_bad - d_init), st) == hipSuccess && hipMemsetAsync(d_bad, 0, b_bad, st) == hipSuccess;
  if (ok) {
    rp_decode_launch(D, B, d_coms, d_prf, (uint32_t *)d_init, (uint32_t *)d_resp, (uint32_t *)d_wn, (uint32_t *)d_wl, (uint32_t *)d_bad, (uint32_t *)d_bad + B, st);
    ok = hipGetLastError() == hipSuccess;
  }
  auto down = [&](void *h, const void *dv, size_t n) { return !n || hipMemcpyAsync(h, dv, n, hipMemcpyDeviceToHost, st) == hipSuccess; };
  ok = ok && down(init_pts, d_init, b_init) && down(resp_pts, d_resp, b_resp) && down(wit_norm, d_wn, b_wn) && down(wit_lin, d_wl, b_wl) && down(bad, d_bad, B * 4) &&
       down(any_bad, d_bad + B * 4, 4);
  if (hipStreamSynchronize(st) != hipSuccess) ok = false;
  hipFree(d);
  return ok ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_rp_decode_device: kernel or copy failed");
}

extern "C" int bppp_test_points_from_seed_chunked(bppp_ctx *ctx, const uint8_t *seed, size_t seed_len, uint64_t first_candidate, size_t count, size_t chunk,
                                                  uint64_t *points_xy, uint64_t *next_candidate) {
  if (!ctx || (seed_len && !seed) || seed_len > SEED_MAX_LEN || !count || !points_xy || !chunk || chunk > SEED_CHUNK_MAX || count >= (1u << 24)) return BPPP_ERR_ARG;
  hipSetDevice(ctx->device);
  SeedMsg M;
  seed_msg_init(M, seed, seed_len);
  void *scratch = nullptr, *d_out = nullptr;
  if (hipMalloc(&scratch, seed_scratch_bytes(chunk)) != hipSuccess || hipMalloc(&d_out, count * 64) != hipSuccess) { hipFree(scratch); return bppp::fail(ctx, BPPP_ERR_HIP, "test_points_from_seed_chunked: hipMalloc"); }
  int rc = seed_points_run(ctx, M, first_candidate, count, chunk, scratch, d_out, next_candidate);
  if (!rc && (hipMemcpyAsync(points_xy, d_out, count * 64, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess))
    rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_points_from_seed_chunked: copy failed");
  hipFree(scratch); hipFree(d_out);
  return rc;
}

namespace bppp {
__global__ void __launch_bounds__(64) k_test_seed_lift(const uint32_t *__restrict__ h, uint32_t n, uint32_t *__restrict__ x, uint32_t *__restrict__ is_point, uint32_t *__restrict__ pts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t d[8];
  for (int k = 0; k < 8; k++) d[k] = h[(size_t)i * 8 + k];
  fe xe; aff pt;
  const bool ok = seed_lift_digest(d, xe, pt);
  if (!ok) pt = aff_inf();
  fe_store(x + (size_t)i * 8, xe);
  is_point[i] = ok ? 1u : 0u;
  aff_store(pts + (size_t)i * 16, pt);
}
}  // namespace bppp
extern "C" int bppp_test_seed_lift_digests(bppp_ctx *ctx, const uint8_t *digests, size_t n, uint64_t *x, uint32_t *is_point, uint64_t *points_xy) {
  if (!ctx || !digests || !n || !x || !is_point || !points_xy || n >= (1u << 20)) return BPPP_ERR_ARG;
  hipSetDevice(ctx->device);
  std::vector<uint32_t> h(n * 8);
  for (size_t i = 0; i < n * 8; i++) h[i] = ((uint32_t)digests[4 * i] << 24) | ((uint32_t)digests[4 * i + 1] << 16) | ((uint32_t)digests[4 * i + 2] << 8) | digests[4 * i + 3];
  uint32_t *d = nullptr;                     // digests | x | points | flags
  BPPP_HIP(ctx, hipMalloc(&d, n * (32 + 32 + 64 + 4)));
  uint32_t *d_x = d + n * 8, *d_p = d_x + n * 8, *d_f = d_p + n * 16;
  hipStream_t st = ctx->stream;
  bool ok = hipMemcpyAsync(d, h.data(), n * 32, hipMemcpyHostToDevice, st) == hipSuccess;
  if (ok) bppp::k_test_seed_lift<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st>>>(d, (uint32_t)n, d_x, d_f, d_p);
  ok = ok && hipMemcpyAsync(x, d_x, n * 32, hipMemcpyDeviceToHost, st) == hipSuccess && hipMemcpyAsync(points_xy, d_p, n * 64, hipMemcpyDeviceToHost, st) == hipSuccess &&
       hipMemcpyAsync(is_point, d_f, n * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (hipStreamSynchronize(st) != hipSuccess) ok = false;
  hipFree(d);
  return ok ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_seed_lift_digests: kernel or copy failed");
}

// ---- the fixed-base comb's launchers (csrc/comb.hip.h) on a table of the test's own: every route of comb_msm, comb_groups, comb_lanes
struct bppp_test_comb { bppp::CombTable t; };

extern "C" int bppp_test_comb_create(bppp_ctx *ctx, const void *d_points, size_t T, int window_bits, bppp_test_comb **out) {
  if (!ctx || !d_points || !T || !out || T >= (1u << 24)) return BPPP_ERR_ARG;
  if (window_bits < 4 || window_bits > 18) return bppp::fail(ctx, BPPP_ERR_ARG, "test_comb_create: window_bits must be in [4,18]");
  hipSetDevice(ctx->device);
  bppp_test_comb *h = new bppp_test_comb();
  CombTable &t = h->t;
  const int c = window_bits;
  t.ctx = ctx; t.T = T; t.c = c; t.W = (257 + c - 1) / c; t.D = 1 << (c - 1); t.tab = nullptr; t.bytes = comb_table_bytes(c, T);
  const std::string err = comb_fill(&t, (const uint32_t *)d_points);
  if (!err.empty()) { (void)hipGetLastError(); delete h; return bppp::fail(ctx, BPPP_ERR_HIP, err); }
  *out = h;
  return BPPP_OK;
}
extern "C" void bppp_test_comb_destroy(bppp_test_comb *h) {
  if (!h) return;
  hipSetDevice(h->t.ctx->device);
  hipStreamSynchronize(h->t.ctx->stream);
  if (h->t.tab) hipFree(h->t.tab);
  delete h;
}
// out (host, `words` uint64): uploaded, handed to `launch` as the device result array, downloaded again
template <typename F> static int comb_hook_run(bppp_ctx *ctx, uint64_t *out, size_t words, size_t scratch_bytes, const char *what, F launch) {
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  uint32_t *d_out = nullptr, *d_scratch = nullptr;
  if (hipMalloc(&d_out, words * 8) != hipSuccess || (scratch_bytes && hipMalloc(&d_scratch, scratch_bytes) != hipSuccess)) {
    (void)hipGetLastError(); hipFree(d_out);
    return bppp::fail(ctx, BPPP_ERR_HIP, std::string(what) + ": hipMalloc failed");
  }
  int rc = hipMemcpyAsync(d_out, out, words * 8, hipMemcpyHostToDevice, st) == hipSuccess ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, std::string(what) + ": upload failed");
  if (!rc) rc = launch(d_out, d_scratch, st);
  if (!rc && hipMemcpyAsync(out, d_out, words * 8, hipMemcpyDeviceToHost, st) != hipSuccess) rc = bppp::fail(ctx, BPPP_ERR_HIP, std::string(what) + ": download failed");
  if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = bppp::fail(ctx, BPPP_ERR_HIP, std::string(what) + ": kernel or copy failed");
  hipFree(d_out); hipFree(d_scratch);
  return rc;
}
extern "C" int bppp_test_comb_msm(bppp_test_comb *h, const void *d_scalars, size_t ninst, size_t nterms, int rows_hint, size_t scratch_bytes, uint64_t *out) {
  if (!h || !d_scalars || !out || !ninst || ninst >= (1u << 31) || nterms > h->t.T || rows_hint < COMB_ROWS_ANY || rows_hint > COMB_ROWS_DENSE) return BPPP_ERR_ARG;
  return comb_hook_run(h->t.ctx, out, ninst * 8, scratch_bytes, "test_comb_msm", [&](uint32_t *d_out, uint32_t *d_scratch, hipStream_t st) {
    return comb_msm_launch(&h->t, (const uint32_t *)d_scalars, ninst, d_out, st, rows_hint, nterms, d_scratch, scratch_bytes);
  });
}
extern "C" int bppp_test_comb_groups(bppp_test_comb *h, const void *d_scalars, size_t ninst, size_t l0, size_t n0, int L, size_t out_stride, uint64_t *out) {
  if (!h || !d_scalars || !out || !ninst || ninst >= (1u << 24) || !out_stride || out_stride >= (1u << 24)) return BPPP_ERR_ARG;
  return comb_hook_run(h->t.ctx, out, ninst * out_stride * 8, 0, "test_comb_groups", [&](uint32_t *d_out, uint32_t *, hipStream_t st) {
    return comb_groups_launch(&h->t, (const uint32_t *)d_scalars, ninst, l0, n0, L, d_out, out_stride, st);
  });
}
extern "C" int bppp_test_comb_lanes(bppp_test_comb *h, const void *d_scalars, size_t nterms, size_t ninst, uint64_t *out) {
  if (!h || !d_scalars || !out || !ninst || ninst >= (1u << 31) || !nterms || nterms > h->t.T) return BPPP_ERR_ARG;
  return comb_hook_run(h->t.ctx, out, ninst * 8, 0, "test_comb_lanes", [&](uint32_t *d_out, uint32_t *, hipStream_t st) {
    return comb_lanes_launch(&h->t, (const uint32_t *)d_scalars, nterms, ninst, d_out, st);
  });
}
extern "C" int bppp_test_last_comb_msm(bppp_ctx *ctx, bppp_test_comb_report *r) {
  if (!ctx || !r) return BPPP_ERR_ARG;
  const CombLast &l = ctx->last_comb;
  r->route = l.route; r->heavy_first = l.heavy_first; r->parts = l.parts; r->tparts = l.tparts; r->wsplit = l.wsplit;
  r->chunks = l.chunks; r->clen = l.clen; r->join_lanes = l.join_lanes;
  return BPPP_OK;
}

extern "C" int bppp_test_last_reduce(bppp_ctx *ctx, bppp_test_reduce_report *r) {
  if (!ctx || !r) return BPPP_ERR_ARG;
  const ReduceLast &l = ctx->last_reduce;
  r->route = l.route; r->combine = l.combine; r->c = l.c; r->W = l.W; r->M = l.M; r->RG = l.RG; r->Lw = l.Lw; r->WPW = l.WPW;
  r->a = l.a; r->LO = l.LO; r->HI = l.HI; r->PR = l.PR; r->PC = l.PC; r->SR = l.SR; r->SC = l.SC; r->TR = l.TR; r->TC = l.TC; r->S = l.S;
  return BPPP_OK;
}

extern "C" int bppp_test_rp_last_text_kernel(bppp_rp *rp, int *lds) {
  if (!rp || !lds) return BPPP_ERR_ARG;
  *lds = rp->last_text_kernel;
  return BPPP_OK;
}

// ---- the size classes of the range-proof layer: the launches' own planning functions (csrc/rpprove_dev.hpp, csrc/trrp.hpp), and what last ran
extern "C" int bppp_test_rp_lds_plan(int kernel, size_t max_base, size_t nranges, size_t nsyms, size_t batch, bppp_test_rp_lds_plan_report *r) {
  if (!r || nranges >= (1u << 24) || nsyms >= (1u << 24) || max_base >= (1u << 24)) return BPPP_ERR_ARG;
  memset(r, 0, sizeof *r);
  if (kernel == BPPP_TEST_RP_K_PHASE2 || kernel == BPPP_TEST_RP_K_PHASE3) {
    const uint32_t maxb = rpp_table_class((uint32_t)max_base);      // the function rpp_maxb rounds with
    r->table = maxb; r->lanes = 64;
    r->lds_bytes = kernel == BPPP_TEST_RP_K_PHASE2 ? rpp_phase2_lds_bytes(maxb, nranges) : rpp_phase3_lds_bytes(nranges);
    r->fits = r->lds_bytes <= LDS_MAX_BYTES;
    return BPPP_OK;
  }
  if (kernel != BPPP_TEST_RP_K_PUBLIC || !batch) return BPPP_ERR_ARG;
  const TrrpPublicPlan p = trrp_public_plan(nsyms, nranges, batch);
  r->lanes = (uint32_t)p.G; r->lds_bytes = p.lds; r->fits = p.lds <= LDS_MAX_BYTES; r->split = p.split ? 1u : 0u;
  return BPPP_OK;
}
extern "C" int bppp_test_rp_last_prove(bppp_rp *rp, bppp_test_rp_prove_report *r) {
  if (!rp || !r) return BPPP_ERR_ARG;
  r->route = rp->last_prove_route; r->table = rp->st.kind == 0 ? rpp_maxb(rp->st) : 0; r->lds2_bytes = rp->last_lds2; r->lds3_bytes = rp->last_lds3;
  return BPPP_OK;
}
extern "C" int bppp_test_trrp_last_public(bppp_trrp *t, bppp_test_rp_public_report *r) {
  if (!t || !r) return BPPP_ERR_ARG;
  r->route = t->last_route; r->lanes = t->last_lanes; r->lds_bytes = t->last_lds;
  return BPPP_OK;
}
extern "C" int bppp_test_rp_last_public(bppp_rp *rp, bppp_test_rp_public_report *r) {
  if (!rp || !r || !rp->tabs) return BPPP_ERR_ARG;
  return bppp_test_trrp_last_public(rp->tabs, r);
}

// ---- the provers' transcript and randomness (csrc/rpp_transcript.hip) alone.  That file and csrc/rpbind.hip are linked into this library as they
// are (bulletproofspp_amd/_build.py); of what they call, only the host oracle of RppTranscript::call lives elsewhere (csrc/rpprove.hip), and the
// hook runs device mode alone: it is never reached.
namespace bppp {
void rpp_host_oracle(const std::string &, std::vector<std::string> &, size_t &, const uint64_t *, size_t, int, uint64_t *) { abort(); }
}  // namespace bppp

extern "C" int bppp_test_rpp_transcript(bppp_rp *rp, size_t batch, const bppp_test_rpp_call *calls, size_t ncalls, const uint64_t *points, const uint8_t *bindings,
                                        uint64_t *challenges) {
  if (!rp || !batch || batch >= (1u << 16) || !calls || !ncalls || ncalls > 64 || !points || !challenges) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t B = batch, stride = rp->D.text_stride;
  std::vector<RppCall> plan;
  size_t total = 0, mmax = 0;
  for (size_t c = 0; c < ncalls; c++) {
    const bppp_test_rpp_call &k = calls[c];
    if (!k.points || k.count < 1 || k.count > 3 || (k.first_slot < 7 ? k.first_slot + k.count > 7 : (k.first_slot != 7 || k.count != 1)))
      return bppp::fail(ctx, BPPP_ERR_ARG, "test_rpp_transcript: a call has points, 1 .. 3 outputs in slots 0 .. 6, or one output in slot 7");
    plan.push_back(RppCall{k.points, k.count, k.first_slot});
    total += k.points; mmax = std::max<size_t>(mmax, k.points);
  }
  // the text buffer of a proof holds the handle's own transcript: npts points of 2 x 78 digits
  if (total > rp_npts(rp->D)) return bppp::fail(ctx, BPPP_ERR_ARG, "test_rpp_transcript: more points than the handle's text buffer holds");
  auto up256 = [](size_t n) { return (n + 255) & ~(size_t)255; };
  const size_t b_ts = up256(B * 4), b_ch = up256(B * 7 * 32), b_es = up256(B * 32), b_hdr = up256(RppTranscript::hdr_bytes(ncalls) + 16), b_pts = up256(B * mmax * 64),
               b_text = up256(B * stride + 64);                 // the text last and 64 bytes longer, as the provers carve it; never first
  uint8_t *d = nullptr;
  BPPP_HIP(ctx, hipMalloc(&d, b_ts + b_ch + b_es + b_hdr + b_pts + b_text));
  uint32_t *d_ts = (uint32_t *)d, *d_ch = (uint32_t *)(d + b_ts), *d_es = (uint32_t *)(d + b_ts + b_ch);
  uint8_t *d_hdr = d + b_ts + b_ch + b_es, *d_pts = d_hdr + b_hdr, *d_text = d_pts + b_pts;
  int rc = rp_bind_begin(rp, bindings, false, B, "test_rpp_transcript");
  RpBindGuard guard{rp};
  if (!rc && hipMemsetAsync(d_ch, 0xA5, b_ch + b_es, st) != hipSuccess) rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_rpp_transcript: memset");
  RppTranscript tr;
  if (!rc) rc = tr.begin(rp, B, plan, 0, false, d_text, d_ts, d_hdr, d_ch, d_es);
  std::vector<uint64_t> hch(B * 28), hes(B * 4);
  for (size_t c = 0; c < ncalls && !rc; c++) {
    const size_t m = calls[c].points;
    if (hipMemcpyAsync(d_pts, points, B * m * 64, hipMemcpyHostToDevice, st) != hipSuccess) { rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_rpp_transcript: upload"); break; }
    points += B * m * 8;
    rc = tr.call((const uint32_t *)d_pts, c);
    if (rc) break;
    if (hipMemcpyAsync(hch.data(), d_ch, B * 7 * 32, hipMemcpyDeviceToHost, st) != hipSuccess || hipMemcpyAsync(hes.data(), d_es, B * 32, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_rpp_transcript: kernel or copy failed"); break; }
    for (size_t b = 0; b < B; b++) {
      uint64_t *out = challenges + (c * B + b) * 12;
      memset(out, 0, 12 * 8);
      if (calls[c].first_slot == 7) memcpy(out, &hes[b * 4], 32);
      else memcpy(out, &hch[b * 28 + calls[c].first_slot * 4], (size_t)calls[c].count * 32);
    }
  }
  hipStreamSynchronize(st);
  hipFree(d);
  return rc;
}

extern "C" int bppp_test_rpp_draws(bppp_ctx *ctx, const uint8_t *prefixes, size_t prefix_len, size_t batch, size_t nd, uint64_t *out) {
  if (!ctx || (prefix_len && !prefixes) || !batch || !nd || !out || prefix_len >= (1u << 20) || (uint64_t)batch * nd >= (1u << 24)) return BPPP_ERR_ARG;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t b_pre = (batch * prefix_len + 16 + 255) & ~(size_t)255, n = batch * nd;
  uint8_t *d = nullptr;
  BPPP_HIP(ctx, hipMalloc(&d, b_pre + n * 32));
  uint32_t *d_rnd = (uint32_t *)(d + b_pre);
  bool ok = hipMemsetAsync(d_rnd, 0xA5, n * 32, st) == hipSuccess && (!prefix_len || hipMemcpyAsync(d, prefixes, batch * prefix_len, hipMemcpyHostToDevice, st) == hipSuccess);
  int rc = ok ? rpp_draws(ctx, d, prefix_len, batch, nd, d_rnd) : bppp::fail(ctx, BPPP_ERR_HIP, "test_rpp_draws: upload failed");
  if (!rc && (hipMemcpyAsync(out, d_rnd, n * 32, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
    rc = bppp::fail(ctx, BPPP_ERR_HIP, "test_rpp_draws: kernel or copy failed");
  hipStreamSynchronize(st);
  hipFree(d);
  return rc;
}

// ---- poison: every scratch buffer of a context / a range-proof handle filled with one byte at its current capacity, so that the next call cannot
// rest on what an earlier one left (include/bppp_test.h states which buffers are scratch and which are persistent)
namespace {
struct Poison {
  bppp_ctx *ctx; int byte; uint64_t total = 0; bool ok = true;
  void hbm(void *p, size_t n) {
    if (!p || !n) return;
    if (hipMemsetAsync(p, byte, n, ctx->stream) != hipSuccess) ok = false;
    total += n;
  }
  void host(void *p, size_t n) {
    if (!p || !n) return;
    memset(p, byte, n);
    total += n;
  }
  bool wait() { return hipStreamSynchronize(ctx->stream) == hipSuccess && ok; }
};
int ctx_poison(bppp_ctx *ctx, int byte, uint64_t *total) {
  hipSetDevice(ctx->device);
  ctx_drain(ctx);
  Poison P{ctx, byte};
  P.hbm(ctx->ws, ctx->ws_bytes);
  P.hbm(ctx->ws2, ctx->ws2_bytes);
  P.hbm(ctx->mix, ctx->mix_bytes);
  P.host(ctx->pinned, ctx->pinned_bytes);
  ctx->last_msm_valid = false;                   // the read-back hooks would copy poison
  *total += P.total;
  return P.wait() ? BPPP_OK : bppp::fail(ctx, BPPP_ERR_HIP, "test_ctx_poison: fill failed");
}
int rp_poison(bppp_rp *rp, int byte, uint64_t *total) {
  bppp_ctx *ctx = rp->ctx;
  hipSetDevice(ctx->device);
  ctx_drain(ctx);
  Poison P{ctx, byte};
  P.hbm(rp->pwork, rp->pwork_bytes);
  P.hbm(rp->awork, rp->awork_bytes);
  P.hbm(rp->work, rp->work_bytes);
  P.hbm(rp->stage, rp->stage_bytes);
  P.hbm(rp->ework, rp->ework_bytes);
  P.hbm(rp->d_pub, rp->d_pub_bytes);
  P.hbm(rp->d_sel, rp->d_sel_bytes);
  P.hbm(rp->d_bind, rp->d_bind_bytes);
  P.hbm(rp->d_bhdr, rp->d_bhdr_bytes);
  P.hbm(rp->d_comb_out, rp->comb_out_rows * 64);
  P.host(rp->hpin, rp->hpin_bytes);
  P.host(rp->hstage, rp->hstage_bytes);
  P.host(rp->hflag, 64);
  *total += P.total;
  if (!P.wait()) return bppp::fail(ctx, BPPP_ERR_HIP, "test_rp_poison: fill failed");
  if (rp->twin) {
    if (int rc = rp_poison(rp->twin, byte, total)) return rc;
    if (rp->twin_ctx && !ctx_closed(rp->twin_ctx)) return ctx_poison(rp->twin_ctx, byte, total);
  }
  return BPPP_OK;
}
}  // namespace

extern "C" int bppp_test_ctx_poison(bppp_ctx *ctx, int byte, uint64_t *bytes_poisoned) {
  if (!ctx || ctx_closed(ctx) || !bytes_poisoned || byte < 0 || byte > 255) return BPPP_ERR_ARG;
  *bytes_poisoned = 0;
  return ctx_poison(ctx, byte, bytes_poisoned);
}
extern "C" int bppp_test_rp_poison(bppp_rp *rp, int byte, uint64_t *bytes_poisoned) {
  if (!rp || !rp->ctx || ctx_closed(rp->ctx) || !bytes_poisoned || byte < 0 || byte > 255) return BPPP_ERR_ARG;
  *bytes_poisoned = 0;
  return rp_poison(rp, byte, bytes_poisoned);
}
