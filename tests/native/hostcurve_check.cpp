// The host window combine on lazy 5 x 52-bit limbs (csrc/hostcurve.hpp) against hostmath.hpp's generic path, which shares no code with it:
// every reference value below comes from mmul / madd / msub / mpow over FQ(), the point formulas and the Horner loop are restated here
// on that path.  Field routines at the largest magnitude their contract allows, the curve routines in every special case, and the whole
// combine in the layouts the MSM routes use.
#include <cstdio>
#include <random>
#include <vector>
#include "hostcurve.hpp"
using namespace bppp_host;

static std::mt19937_64 g(2024);
static int bad = 0;
static void fail(const char *what, int i) { if (bad < 12) printf("MISMATCH %s (case %d)\n", what, i); bad++; }

// ---- the generic reference
static const Mod &M = FQ();
static U256 rmul(const U256 &a, const U256 &b) { return mmul(a, b, M); }
static U256 radd(const U256 &a, const U256 &b) { return madd(a, b, M); }
static U256 rsub(const U256 &a, const U256 &b) { return msub(a, b, M); }
static U256 rinv(const U256 &a) { U256 e; sub_raw(e, M.m, U256::from_u64(2)); return mpow(a, e, M); }
static U256 rnd_fq() { for (;;) { U256 r = {{g(), g(), g(), g()}}; if (cmp(r, M.m) < 0) return r; } }
static U256 pm1() { U256 r; sub_raw(r, M.m, U256::one()); return r; }
// sum limb[i] 2^(bits i) mod p by Horner's rule; limbs of any size
static U256 ref_limbs(const uint64_t *n, int count, int bits) {
  U256 acc = U256::zero(), radix = U256::from_u64(1ull << bits);
  for (int i = count - 1; i >= 0; i--) acc = radd(rmul(acc, radix), mmul(U256::from_u64(n[i]), U256::one(), M));
  return acc;
}
static U256 ref_f52(const F52 &a) { return ref_limbs(a.n, 5, 52); }
static U256 ref_l26(const uint32_t *q) { uint64_t n[10]; for (int i = 0; i < 10; i++) n[i] = q[i]; return ref_limbs(n, 10, 26); }

struct RJ { U256 X, Y, Z; bool inf() const { return Z.is_zero(); } };
static RJ rj_inf() { return {U256::one(), U256::one(), U256::zero()}; }
static RJ rj_dbl(const RJ &p) {     // dbl-2007-bl with a = 0
  if (p.inf() || p.Y.is_zero()) return rj_inf();
  U256 A = rmul(p.X, p.X), B = rmul(p.Y, p.Y), C = rmul(B, B);
  U256 t = radd(p.X, B); t = rsub(rsub(rmul(t, t), A), C);
  U256 D = radd(t, t), E = radd(radd(A, A), A), F = rmul(E, E);
  RJ r;
  r.X = rsub(rsub(F, D), D);
  U256 c8 = radd(C, C); c8 = radd(c8, c8); c8 = radd(c8, c8);
  r.Y = rsub(rmul(E, rsub(D, r.X)), c8);
  r.Z = rmul(p.Y, p.Z); r.Z = radd(r.Z, r.Z);
  return r;
}
static RJ rj_add(const RJ &p, const RJ &q) {
  if (p.inf()) return q;
  if (q.inf()) return p;
  U256 z1z1 = rmul(p.Z, p.Z), z2z2 = rmul(q.Z, q.Z);
  U256 u1 = rmul(p.X, z2z2), u2 = rmul(q.X, z1z1);
  U256 s1 = rmul(rmul(p.Y, q.Z), z2z2), s2 = rmul(rmul(q.Y, p.Z), z1z1);
  U256 h = rsub(u2, u1), r = rsub(s2, s1);
  if (h.is_zero()) return r.is_zero() ? rj_dbl(p) : rj_inf();
  U256 hh = rmul(h, h), hhh = rmul(h, hh), v = rmul(u1, hh);
  RJ o;
  o.X = rsub(rsub(rsub(rmul(r, r), hhh), v), v);
  o.Y = rsub(rmul(r, rsub(v, o.X)), rmul(s1, hhh));
  o.Z = rmul(rmul(p.Z, q.Z), h);
  return o;
}
struct RA { U256 x, y; };
static RA rj_aff(const RJ &p) {
  if (p.inf()) return {U256::zero(), U256::zero()};
  U256 zi = rinv(p.Z), zi2 = rmul(zi, zi);
  return {rmul(p.X, zi2), rmul(p.Y, rmul(zi2, zi))};
}
static RJ rj_from_xyzz(const U256 &X, const U256 &Y, const U256 &ZZ, const U256 &ZZZ) {
  if (ZZ.is_zero()) return rj_inf();
  return {rmul(X, ZZ), rmul(Y, ZZZ), ZZ};
}
// a random curve point: y = (x^3 + 7)^((p + 1) / 4) where that is a square root
static RA rnd_point() {
  U256 e; add_raw(e, M.m, U256::one());
  for (int i = 0; i < 4; i++) e.w[i] = (e.w[i] >> 2) | (i < 3 ? e.w[i + 1] << 62 : 0);
  for (;;) {
    U256 x = rnd_fq(), rhs = radd(rmul(rmul(x, x), x), U256::from_u64(7)), y = mpow(rhs, e, M);
    if (rmul(y, y) == rhs && !y.is_zero()) return {x, (g() & 1) ? y : mneg(y, M)};
  }
}
static RA ra_neg(const RA &a) { return {a.x, mneg(a.y, M)}; }

// ---- device encodings
static void limbs26_of(const U256 &v, uint32_t *q) {      // canonical 10 x 26
  for (int i = 0; i < 10; i++) {
    const int bit = 26 * i, k = bit >> 6, sh = bit & 63;
    uint64_t x = v.w[k] >> sh;
    if (sh > 38 && k < 3) x |= v.w[k + 1] << (64 - sh);
    q[i] = (uint32_t)(x & 0x3FFFFFF);
  }
}
// v at device magnitude m: the limb-wise sum of 2 m canonical values that add up to v; every limb <= 2 m (2^26 - 1)
static void limbs26_mag(const U256 &v, int m, uint32_t *q) {
  U256 rest = v;
  for (int i = 0; i < 10; i++) q[i] = 0;
  for (int j = 0; j < 2 * m; j++) {
    const U256 part = j == 2 * m - 1 ? rest : j == 1 ? pm1() : rnd_fq();     // one summand with every limb full
    rest = rsub(rest, part);
    uint32_t t[10]; limbs26_of(part, t);
    for (int i = 0; i < 10; i++) q[i] += t[i];
  }
}
// the affine point a as a device XYZZ point with a random denominator, at the magnitudes the reduce kernels state (X <= 5, Y <= 3, ZZ, ZZZ = 1)
static void xyzz_of(const RA &a, uint32_t *q, bool lazy) {
  U256 z = rnd_fq(); if (z.is_zero()) z = U256::one();
  U256 zz = rmul(z, z), zzz = rmul(zz, z);
  limbs26_mag(rmul(a.x, zz), lazy ? 5 : 1, q);
  limbs26_mag(rmul(a.y, zzz), lazy ? 3 : 1, q + 10);
  limbs26_mag(zz, 1, q + 20);
  limbs26_mag(zzz, 1, q + 30);
}
// infinity: ZZ = 0, written as 0, as p or as 2 p (limb-wise), the other coordinates arbitrary
static void xyzz_inf(uint32_t *q, int form) {
  for (int i = 0; i < 40; i++) q[i] = (uint32_t)g() & 0x3FFFFFF;
  q[19] &= 0x3FFFFF; q[9] &= 0x3FFFFF; q[39] &= 0x3FFFFF;
  uint32_t p26[10]; limbs26_of(M.m, p26);
  for (int i = 0; i < 10; i++) q[20 + i] = p26[i] * (uint32_t)form;
}
static RJ rj_of_device(const uint32_t *q) { return rj_from_xyzz(ref_l26(q), ref_l26(q + 10), ref_l26(q + 20), ref_l26(q + 30)); }

// the Horner combine as msm.hip had it, on the generic path
static RA ref_combine(const uint32_t *ws, int W, int c, int acnt, bool marg, int a) {
  RJ r = rj_inf();
  for (int w = W - 1; w >= 0; w--) {
    const int cw = w < acnt ? c : c - 1;
    if (marg) {
      const uint32_t *q = ws + (size_t)w * 80;
      for (int k = 0; k < cw - a; k++) r = rj_dbl(r);
      r = rj_add(r, rj_of_device(q));
      for (int k = 0; k < a; k++) r = rj_dbl(r);
      r = rj_add(r, rj_of_device(q + 40));
    } else {
      for (int k = 0; k < cw; k++) r = rj_dbl(r);
      r = rj_add(r, rj_of_device(ws + (size_t)w * 40));
    }
  }
  return rj_aff(r);
}
static bool same(const RA &a, const uint64_t *xy) { return a.x == U256::load(xy) && a.y == U256::load(xy + 4); }
static bool fj_is(const FJac &p, const RA &a) { uint64_t xy[8]; fj_to_affine(p, xy); return same(a, xy); }
static FJac fj_of_aff(const RA &a) {     // through the addition to infinity, the only way the combine makes one
  uint32_t q[40]; xyzz_of(a, q, true);
  return fj_add_xyzz(fj_inf(), fx_from_device(q));
}

// a field element with limbs up to the bound of magnitude m: kind 0 random below the bound, 1 the bound itself, 2 canonical limbs
static F52 f52_at(int m, int kind) {
  F52 r;
  for (int i = 0; i < 5; i++) {
    const uint64_t top = 2 * (uint64_t)m * (i < 4 ? F52_M52 : F52_M48);
    r.n[i] = kind == 1 ? top : kind == 2 ? g() & (i < 4 ? F52_M52 : F52_M48) : g() % (top + 1);
  }
  return r;
}

static void field_cases() {
  const U256 specials[4] = {U256::zero(), U256::one(), pm1(), U256::from_u64(0x1000003D1ULL)};
  // conversions
  for (int it = 0; it < 20000; it++) {
    const U256 a = it < 4 ? specials[it] : rnd_fq();
    if (!(f52_to_u256(f52_from_u256(a)) == a) || !(ref_f52(f52_from_u256(a)) == a)) fail("u256 round trip", it);
    uint32_t q[10];
    for (int i = 0; i < 10; i++) q[i] = (it & 1) ? (uint32_t)g() : 0xFFFFFFFFu;
    if (it == 5) limbs26_of(M.m, q);                        // p itself -> 0
    if (it >= 6 && it < 2000) limbs26_mag(a, 1 + it % 8, q);
    F52 f = f52_from_limbs26(q);
    if (!(ref_f52(f) == ref_l26(q))) fail("from_limbs26 value", it);
    f52_weak(f);
    for (int i = 0; i < 5; i++) if (f.n[i] > 2 * (i < 4 ? F52_M52 : F52_M48)) fail("weak magnitude", it);
    if (!(f52_to_u256(f) == ref_l26(q)) || !(from_limbs26(q) == ref_l26(q))) fail("from_limbs26 -> weak -> u256", it);
  }
  // mul, sqr: canonical specials, random, and both operands at magnitude 8 (random limbs below the bound, and the bound itself)
  for (int it = 0; it < 60000; it++) {
    F52 a, b;
    if (it < 16) { a = f52_from_u256(specials[it & 3]); b = f52_from_u256(specials[it >> 2]); }
    else if (it < 32) { a = f52_at(8, (it >> 0) & 1); b = f52_at(8, (it >> 1) & 1); if (it & 4) a = f52_at(1 + it % 8, 1); }
    else { const int ma = 1 + (int)(g() % 8), mb = 1 + (int)(g() % 8); a = f52_at(ma, (it & 7) == 0 ? 2 : 0); b = f52_at(mb, (it & 15) == 0 ? 2 : 0); }
    const U256 ra = ref_f52(a), rb = ref_f52(b);
    const F52 pr = f52_mul(a, b), sq = f52_sqr(a);
    for (int i = 0; i < 5; i++) if (pr.n[i] > 2 * (i < 4 ? F52_M52 : F52_M48) || sq.n[i] > 2 * (i < 4 ? F52_M52 : F52_M48)) fail("mul/sqr result magnitude", it);
    if (!(f52_to_u256(pr) == rmul(ra, rb))) fail("mul", it);
    if (!(f52_to_u256(sq) == rmul(ra, ra))) fail("sqr", it);
  }
  // add, small multiples, negation, normalize at the contract's bounds
  for (int it = 0; it < 60000; it++) {
    const int m = 1 + it % 7, kind = (it / 7) % 3;
    const F52 a = f52_at(m, kind), b = f52_at(8 - m, (it / 21) % 3);
    const U256 ra = ref_f52(a), rb = ref_f52(b);
    if (!(f52_to_u256(f52_add(a, b)) == radd(ra, rb))) fail("add", it);                               // magnitude 8
    const F52 ng = f52_neg(a, m);                                                                     // magnitude m + 1 <= 8
    for (int i = 0; i < 5; i++) if (ng.n[i] > 2 * (uint64_t)(m + 1) * (i < 4 ? F52_M52 : F52_M48)) fail("neg magnitude", it);
    if (!(f52_to_u256(ng) == mneg(ra, M))) fail("neg", it);
    if (!f52_is_zero(f52_add(a, ng))) fail("a + (-a) is zero", it);                                   // magnitude 2 m + 1 <= 15
    const uint64_t k = 1 + (uint64_t)(it % (16 / m));                                                 // k m <= 16
    if (!(f52_to_u256(f52_mul_int(a, k)) == rmul(ra, U256::from_u64(k)))) fail("mul_int", it);
    const F52 big = f52_at(16, kind);
    F52 nz = big; f52_normalize(nz);
    if (!(f52_to_u256(big) == ref_f52(big)) || cmp(f52_to_u256(big), M.m) >= 0 || !(ref_f52(nz) == ref_f52(big))) fail("normalize at magnitude 16", it);
    for (int i = 0; i < 5; i++) if (nz.n[i] > (i < 4 ? F52_M52 : F52_M48)) fail("normalize leaves canonical limbs", it);
  }
  // every multiple k p, k <= 32 (limb-wise, magnitude 16), is zero; k p + 1 and k p - 1 are not
  for (int k = 0; k <= 32; k++) {
    F52 kp = f52_mul_int(F52{{F52_P0, F52_M52, F52_M52, F52_M52, F52_M48}}, (uint64_t)k);
    if (!f52_is_zero(kp) || !f52_to_u256(kp).is_zero()) fail("k p is zero", k);
    F52 up = kp; up.n[0] += 1;
    if (f52_is_zero(up) || !(f52_to_u256(up) == U256::one())) fail("k p + 1", k);
    if (k) { F52 dn = kp; dn.n[0] -= 1; if (f52_is_zero(dn) || !(f52_to_u256(dn) == pm1())) fail("k p - 1", k); }
  }
  // inversion: 0 -> 0, 1, p - 1, random, lazy input
  for (int it = 0; it < 300; it++) {
    const F52 a = it < 4 ? f52_from_u256(specials[it]) : it < 8 ? f52_at(8, it & 1) : it & 1 ? f52_at(1 + it % 8, 0) : f52_from_u256(rnd_fq());
    const U256 ra = ref_f52(a), want = rinv(ra);
    if (!(f52_to_u256(f52_inv(a)) == want)) fail("inv", it);
    if (it == 0 && !want.is_zero()) fail("reference inverse of 0", it);
    if (!ra.is_zero() && !(rmul(want, ra) == U256::one())) fail("reference inverse", it);
  }
  // hostmath's fqinv and fqmul keep their semantics
  for (int it = 0; it < 50; it++) {
    const U256 a = it < 4 ? specials[it] : rnd_fq(), b = rnd_fq();
    if (!(fqinv(a) == rinv(a)) || !(fqmul(a, b) == rmul(a, b))) fail("fqinv / fqmul", it);
  }
}

static void point_cases() {
  for (int it = 0; it < 300; it++) {
    const RA P = rnd_point(), Q = rnd_point();
    const RJ rP = {P.x, P.y, U256::one()}, rQ = {Q.x, Q.y, U256::one()};
    uint32_t q[40], qi[40];
    xyzz_of(Q, q, it & 1);
    xyzz_inf(qi, it % 3);
    const FXyzz fQ = fx_from_device(q), fI = fx_from_device(qi);
    if (fQ.inf || !fI.inf) fail("infinity flag of a device point", it);
    // an accumulator with Z != 1 and lazy coordinates: 2 (P + Q) - ... built both ways
    FJac acc = fj_of_aff(P);
    RJ racc = rP;
    if (!fj_is(acc, P)) fail("infinity + P", it);
    if (!fj_is(fj_add_xyzz(acc, fI), P)) fail("P + infinity", it);
    if (!fj_add_xyzz(fj_inf(), fI).inf || !fj_is(fj_add_xyzz(fj_inf(), fI), RA{U256::zero(), U256::zero()})) fail("infinity + infinity", it);
    if (!fj_dbl(fj_inf()).inf) fail("2 infinity", it);
    for (int k = 0; k < 1 + it % 3; k++) { acc = fj_dbl(acc); racc = rj_dbl(racc); }
    if (!fj_is(acc, rj_aff(racc))) fail("doubling", it);
    acc = fj_add_xyzz(acc, fQ); racc = rj_add(racc, rQ);
    if (!fj_is(acc, rj_aff(racc))) fail("addition", it);
    acc = fj_dbl(acc); racc = rj_dbl(racc);                   // doubling after an addition (Z != 1, magnitudes 1)
    acc = fj_dbl(acc); racc = rj_dbl(racc);                   // and after a doubling (X 6, Y 4, Z 2)
    const RA A = rj_aff(racc);
    if (!fj_is(acc, A)) fail("doubling of a sum", it);
    // the accumulator's own point through the addition: P + P, then P + (-P)
    uint32_t qa[40];
    xyzz_of(A, qa, it & 2);
    if (!fj_is(fj_add_xyzz(acc, fx_from_device(qa)), rj_aff(rj_dbl(racc)))) fail("P + P through the addition", it);
    xyzz_of(ra_neg(A), qa, it & 2);
    const FJac z = fj_add_xyzz(acc, fx_from_device(qa));
    if (!z.inf || !fj_is(z, RA{U256::zero(), U256::zero()})) fail("P + (-P)", it);
  }
}

struct Layout { int c, W, acnt; };
static Layout balanced(int c) { const int W = (256 + c - 1) / c; return {c, W, 256 - W * (c - 1)}; }     // as window_layout (msm.hip)

static void combine_cases() {
  int idx = 0;
  const int cs[3] = {6, 13, 16};
  for (int ci = 0; ci < 3; ci++) for (int marg = 0; marg < 2; marg++) for (int batch = 1; batch <= 4; batch += 3) for (int variant = 0; variant < 6; variant++, idx++) {
    const Layout L = balanced(cs[ci]);
    const int c = L.c, W = L.W, per = marg ? 2 : 1, a = marg ? (variant & 1 ? c / 2 : c - 1 - variant % 3) : 0;
    // variant 5: every window c wide (acnt = W: a flat table, or a width that divides 256)
    const int acnt = variant == 5 ? W : L.acnt;
    std::vector<uint32_t> ws((size_t)batch * W * per * 40);
    for (int b = 0; b < batch; b++) {
      uint32_t *base = ws.data() + (size_t)b * W * per * 40;
      for (int s = 0; s < W * per; s++) {
        const int w = s / per;
        const bool inf = variant == 1 ? true                                 // every window sum infinity
                         : variant == 2 ? w >= 2                             // only the lowest windows hold points (scalars < 2^(2 c))
                         : variant == 3 ? (g() % 3 == 0) : false;
        if (inf) xyzz_inf(base + (size_t)s * 40, (int)(g() % 3)); else xyzz_of(rnd_point(), base + (size_t)s * 40, variant != 4);
      }
      if (variant == 0 || variant == 3) {
        // slot `hit` holds minus the accumulator that reaches it, so the accumulator passes through infinity mid-Horner and goes on
        const int hit = (int)(g() % (unsigned)(W * per - 2)) + 1;             // counted from the top; at least one slot before and after
        RJ r = rj_inf();
        int slot = 0;
        for (int w = W - 1; w >= 0 && slot <= hit; w--) {
          const int cw = w < acnt ? c : c - 1;
          for (int h = 0; h < per && slot <= hit; h++, slot++) {
            const int nd = !marg ? cw : h == 0 ? cw - a : a;
            for (int k = 0; k < nd; k++) r = rj_dbl(r);
            uint32_t *q = base + ((size_t)w * per + h) * 40;
            if (slot == hit) { RA m = rj_aff(r); if (m.x.is_zero() && m.y.is_zero()) xyzz_inf(q, 0); else xyzz_of(ra_neg(m), q, true); }
            r = rj_add(r, rj_of_device(q));
            if (slot == hit && !r.inf()) fail("test construction: accumulator is not infinity at the chosen slot", idx);
          }
        }
      }
    }
    for (int b = 0; b < batch; b++) {
      const uint32_t *base = ws.data() + (size_t)b * W * per * 40;
      uint64_t xy[8];
      for (int i = 0; i < 8; i++) xy[i] = ~0ull;
      window_combine_host(base, W, c, acnt, marg != 0, a, xy);
      const RA want = ref_combine(base, W, c, acnt, marg != 0, a);
      if (!same(want, xy)) fail("window_combine_host", idx);
      if (variant == 1 && !(want.x.is_zero() && want.y.is_zero())) fail("all-infinity reference", idx);
      if (variant == 1) for (int i = 0; i < 8; i++) if (xy[i]) fail("all-infinity combine is (0, 0)", idx);
    }
  }
  // one window (a flat table: Wc = 1), and W = 1 with a point at the device's largest stated limbs
  for (int it = 0; it < 8; it++) {
    uint32_t q[80];
    xyzz_of(rnd_point(), q, true); xyzz_of(rnd_point(), q + 40, true);
    if (it & 4) xyzz_inf(q, it & 3);
    uint64_t xy[8];
    window_combine_host(q, 1, 16, 1, (it & 1) != 0, (it & 1) ? 8 : 0, xy);
    if (!same(ref_combine(q, 1, 16, 1, (it & 1) != 0, (it & 1) ? 8 : 0), xy)) fail("single window", it);
  }
}

int main() {
  field_cases();
  point_cases();
  combine_cases();
  if (bad) printf("FAILED (%d)\n", bad); else printf("ok\n");
  return bad ? 1 : 0;
}
