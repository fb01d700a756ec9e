// Host-only timing of the MSM's final window combine (no GPU): the Horner loop over device window sums that msm_run_ex runs on one core
// after the stream has drained.
//
//   g++ -O3 -std=c++17 -I bulletproofspp_amd/csrc -o benchmarks/host_combine_timing benchmarks/host_combine_timing.cpp && benchmarks/host_combine_timing
//
// Two shapes: the marginal layout of the large MSM (c = 16, 16 windows of (W1, W2), a = 8) and the one-launch small route (c = 6, 43 windows,
// balanced widths).  "u256" is the loop on hostmath.hpp's canonical U256 routines (hj_dbl / hj_add / hj_to_aff, as msm.hip had it); "f52" is
// window_combine_host (csrc/hostcurve.hpp).  Built in a tree without hostcurve.hpp the program times the u256 loop alone, so the same file
// gives the figure of an older commit.  The last block compares field layouts on dependent chains: fqmul (4 x 64, canonical), a branch-free
// lazy 4 x 64 (values < 2^256, not canonical) and the lazy 5 x 52, each as multiply, square and one a = 0 doubling (3 M + 4 S and its
// additions), which is what decides the layout: the combine is 256 doublings long.
// Prints one JSON line per figure: nanoseconds per call, median and minimum over the repetitions.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <random>
#include <vector>
#include "hostmath.hpp"
#if __has_include("hostcurve.hpp")
#include "hostcurve.hpp"
#define HAVE_F52 1
#else
#define HAVE_F52 0
#endif
using namespace bppp_host;

static std::mt19937_64 g(7);
static U256 rnd_fq() { for (;;) { U256 r = {{g(), g(), g(), g()}}; if (cmp(r, FQ().m) < 0) return r; } }
static void limbs26_of(const U256 &v, uint32_t *q) {
  for (int i = 0; i < 10; i++) {
    const int bit = 26 * i, k = bit >> 6, sh = bit & 63;
    uint64_t x = v.w[k] >> sh;
    if (sh > 38 && k < 3) x |= v.w[k + 1] << (64 - sh);
    q[i] = (uint32_t)(x & 0x3FFFFFF);
  }
}
// `count` curve points as device XYZZ values with random denominators: multiples of the generator
static std::vector<uint32_t> window_sums(int count) {
  const U256 gx = {{0x59F2815B16F81798ULL, 0x029BFCDB2DCE28D9ULL, 0x55A06295CE870B07ULL, 0x79BE667EF9DCBBACULL}};
  const U256 gy = {{0x9C47D08FFB10D4B8ULL, 0xFD17B448A6855419ULL, 0x5DA4FBFC0E1108A8ULL, 0x483ADA7726A3C465ULL}};
  std::vector<uint32_t> ws((size_t)count * 40);
  HJac p = hj_from_aff(HAff{gx, gy});
  for (int i = 0; i < count; i++) {
    for (int k = 0; k < 3; k++) p = hj_dbl(p);
    p = hj_add(p, hj_from_aff(HAff{gx, gy}));
    const HAff a = hj_to_aff(p);
    const U256 z = rnd_fq(), zz = fqmul(z, z), zzz = fqmul(zz, z);
    limbs26_of(fqmul(a.x, zz), &ws[(size_t)i * 40]); limbs26_of(fqmul(a.y, zzz), &ws[(size_t)i * 40 + 10]);
    limbs26_of(zz, &ws[(size_t)i * 40 + 20]); limbs26_of(zzz, &ws[(size_t)i * 40 + 30]);
  }
  return ws;
}

// the loop of msm_run_ex before hostcurve.hpp
static void combine_u256(const uint32_t *ws, int W, int c, int acnt, bool marg, int a, uint64_t *out_xy) {
  HJac r = hj_inf();
  auto pt = [&](const uint32_t *q) { return hj_from_xyzz(from_limbs26(q), from_limbs26(q + 10), from_limbs26(q + 20), from_limbs26(q + 30)); };
  for (int w = W - 1; w >= 0; w--) {
    const int cw = w < acnt ? c : c - 1;
    if (marg) {
      const uint32_t *q = ws + (size_t)w * 80;
      for (int k = 0; k < cw - a; k++) r = hj_dbl(r);
      r = hj_add(r, pt(q));
      for (int k = 0; k < a; k++) r = hj_dbl(r);
      r = hj_add(r, pt(q + 40));
    } else {
      for (int k = 0; k < cw; k++) r = hj_dbl(r);
      r = hj_add(r, pt(ws + (size_t)w * 40));
    }
  }
  HAff o = hj_to_aff(r);
  o.x.store(out_xy); o.y.store(out_xy + 4);
}

static volatile uint64_t sink;
template <class F> static void report(const char *name, int inner, F f) {
  std::vector<double> ns;
  for (int rep = 0; rep < 41; rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < inner; i++) f();
    const auto t1 = std::chrono::steady_clock::now();
    ns.push_back(std::chrono::duration<double, std::nano>(t1 - t0).count() / inner);
  }
  std::sort(ns.begin(), ns.end());
  printf("{\"name\": \"%s\", \"ns_median\": %.1f, \"ns_min\": %.1f}\n", name, ns[ns.size() / 2], ns[0]);
}

// ---- a branch-free lazy 4 x 64 field for the layout comparison only: values < 2^256, not canonical
struct L4 { uint64_t w[4]; };
static inline L4 l4_fold(const uint64_t t[4], uint64_t hi) {       // t + hi * R, twice: the second carry cannot carry again
  const uint64_t R = 0x1000003D1ULL;
  u128 c = (u128)hi * R;
  L4 o;
  for (int i = 0; i < 4; i++) { c += t[i]; o.w[i] = (uint64_t)c; c >>= 64; }
  c = (u128)(uint64_t)c * R;
  for (int i = 0; i < 4; i++) { c += o.w[i]; o.w[i] = (uint64_t)c; c >>= 64; }
  return o;
}
static inline L4 l4_mul(const L4 &a, const L4 &b) {
  uint64_t t[8] = {0};
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) { c += (u128)a.w[i] * b.w[j] + t[i + j]; t[i + j] = (uint64_t)c; c >>= 64; }
    t[i + 4] = (uint64_t)c;
  }
  const uint64_t R = 0x1000003D1ULL;
  uint64_t r[4];
  u128 c = 0;
  for (int i = 0; i < 4; i++) { c += (u128)t[4 + i] * R + t[i]; r[i] = (uint64_t)c; c >>= 64; }
  return l4_fold(r, (uint64_t)c);
}
static inline L4 l4_add(const L4 &a, const L4 &b) {
  uint64_t t[4]; u128 c = 0;
  for (int i = 0; i < 4; i++) { c += (u128)a.w[i] + b.w[i]; t[i] = (uint64_t)c; c >>= 64; }
  return l4_fold(t, (uint64_t)c);
}
static inline L4 l4_sub(const L4 &a, const L4 &b) {                // a + (2^256 - 1 - b) + 1 - 2^256: the carry out is 1 unless a < b, when R is taken off
  const uint64_t R = 0x1000003D1ULL;
  uint64_t t[4], br = 0;
  for (int i = 0; i < 4; i++) { u128 d = (u128)a.w[i] - b.w[i] - br; t[i] = (uint64_t)d; br = (uint64_t)(d >> 64) & 1; }
  for (int pass = 0; pass < 2; pass++) {
    uint64_t sub = br * R; br = 0;
    for (int i = 0; i < 4; i++) { u128 d = (u128)t[i] - sub - br; t[i] = (uint64_t)d; br = (uint64_t)(d >> 64) & 1; sub = 0; }
  }
  return L4{{t[0], t[1], t[2], t[3]}};
}
struct L4J { L4 X, Y, Z; };
static inline L4J l4_dbl(const L4J &p) {                            // the same 3 M + 4 S doubling as fj_dbl
  L4J r;
  L4 yz = l4_mul(p.Y, p.Z); r.Z = l4_add(yz, yz);
  L4 xx = l4_mul(p.X, p.X), L = l4_add(l4_add(xx, xx), xx), LL = l4_mul(L, L);
  L4 yy = l4_mul(p.Y, p.Y), T = l4_add(yy, yy), tt = l4_mul(T, T), TT2 = l4_add(tt, tt);
  L4 XT = l4_mul(T, p.X), XT2 = l4_add(XT, XT), XT4 = l4_add(XT2, XT2);
  r.X = l4_sub(LL, XT4);
  r.Y = l4_sub(l4_mul(L, l4_sub(l4_add(XT4, XT2), LL)), TT2);
  return r;
}

int main() {
  uint64_t xy[8];
  const std::vector<uint32_t> big = window_sums(32), small = window_sums(43);
  report("combine_u256_marg_c16_w16", 50, [&] { combine_u256(big.data(), 16, 16, 16, true, 8, xy); sink = xy[0]; });
  report("combine_u256_plain_c6_w43", 50, [&] { combine_u256(small.data(), 43, 6, 41, false, 0, xy); sink = xy[0]; });
#if HAVE_F52
  uint64_t xy2[8];
  report("combine_f52_marg_c16_w16", 50, [&] { window_combine_host(big.data(), 16, 16, 16, true, 8, xy2); sink = xy2[0]; });
  report("combine_f52_plain_c6_w43", 50, [&] { window_combine_host(small.data(), 43, 6, 41, false, 0, xy2); sink = xy2[0]; });
  combine_u256(big.data(), 16, 16, 16, true, 8, xy);
  window_combine_host(big.data(), 16, 16, 16, true, 8, xy2);
  printf("{\"name\": \"results_equal\", \"value\": %s}\n", memcmp(xy, xy2, 64) == 0 ? "true" : "false");
#endif
  // ---- field layouts on dependent chains
  {
    U256 a = rnd_fq(), b = rnd_fq();
    report("u256_fqmul", 20000, [&] { a = fqmul(a, b); });
    sink = a.w[0];
    HJac p = {rnd_fq(), rnd_fq(), rnd_fq()};
    report("u256_hj_dbl", 5000, [&] { p = hj_dbl(p); });
    sink = p.X.w[0];
    report("u256_fqinv", 50, [&] { a = fqinv(a); });
    sink = a.w[0];
  }
  {
    const U256 u = rnd_fq(), v = rnd_fq();
    L4 a = {{u.w[0], u.w[1], u.w[2], u.w[3]}}, b = {{v.w[0], v.w[1], v.w[2], v.w[3]}};
    report("lazy4x64_mul", 20000, [&] { a = l4_mul(a, b); });
    sink = a.w[0];
    L4J p = {a, b, a};
    report("lazy4x64_dbl", 5000, [&] { p = l4_dbl(p); });
    sink = p.X.w[0];
  }
#if HAVE_F52
  {
    F52 a = f52_from_u256(rnd_fq()), b = f52_from_u256(rnd_fq());
    report("f52_mul", 20000, [&] { a = f52_mul(a, b); });
    report("f52_sqr", 20000, [&] { a = f52_sqr(a); });
    sink = a.n[0];
    FJac p = {a, b, a, false};
    report("f52_dbl", 5000, [&] { p = fj_dbl(p); });
    sink = p.X.n[0];
    report("f52_inv", 50, [&] { a = f52_inv(a); });
    sink = a.n[0];
  }
#endif
  return 0;
}
