// fqmul_variants.hip — the forms of the Fq multiplication (csrc/fq26.hip.h, benchmarks/fqmul_variants.h) against each other: same results on
// random and worst-case-magnitude inputs, multiplications per second at 8 wavefronts per SIMD (the bppp_test_mulmod_rate shape: four
// independent chains per lane), and the 9 x 29-bit multiplication of csrc/fq29.hip.h in the same run; with the argument `chain`, dependent chains
// at 1 .. 8 wavefronts per SIMD.   hipcc -O3 --offload-arch=gfx950 -std=c++17 -o benchmarks/fqmul_variants benchmarks/fqmul_variants.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "fqmul_variants.h"
#include "../bulletproofspp_amd/csrc/ec_quad.hip.h"
#include "../bulletproofspp_amd/csrc/fq29.hip.h"
using namespace bppp;

template <int V> BPPP_DI fq mulv(const fq &a, const fq &b) {
  if (V == 1) return fq_mul(a, b);
  if (V == 2) return fq_mul_v2(a, b);
  if (V == 3) return fq_mul_v3(a, b);
  return fq_mul_cols(a, b);
}
template <int V> __global__ void __launch_bounds__(256) k_rate(const uint32_t *__restrict__ seed, int iters, uint32_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  fq a[4], b;
  for (int k = 0; k < 4; k++) a[k] = fq_from_fe(fe_load(seed + (size_t)((t + 17 * k) & 1023) * 8));
  b = fq_from_fe(fe_load(seed + (size_t)((t * 7 + 3) & 1023) * 8));
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = mulv<V>(a[k], b);
  }
  fq r = fq_add(fq_add(a[0], a[1]), fq_add(a[2], a[3]));
  fe_store(out + (size_t)t * 8, fq_to_fe(r));
}
// worst-case magnitudes: (8 a) * (-7 b)
template <int V> __global__ void k_mag(const uint32_t *__restrict__ seed, uint32_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const fq x = fq_from_fe(fe_load(seed + (size_t)(t & 1023) * 8)), y = fq_from_fe(fe_load(seed + (size_t)((t * 5 + 1) & 1023) * 8));
  fe_store(out + (size_t)t * 8, fq_to_fe(mulv<V>(fq_mul_int(x, 8), fq_neg<7>(fq_mul_int(y, 7)))));
}
template <int V> double run(const uint32_t *seed, uint32_t *out, std::vector<uint32_t> &res, std::vector<uint32_t> &mag) {
  const int blocks = 256 * 4 * 8 / 4 * 2, iters = 2000;
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  k_rate<V><<<blocks, 256>>>(seed, 8, out);
  hipEventRecord(e0);
  k_rate<V><<<blocks, 256>>>(seed, iters, out);
  hipEventRecord(e1); hipEventSynchronize(e1);
  float ms = 0; hipEventElapsedTime(&ms, e0, e1);
  res.resize((size_t)blocks * 256 * 8); hipMemcpy(res.data(), out, res.size() * 4, hipMemcpyDeviceToHost);
  k_mag<V><<<64, 256>>>(seed, out);
  mag.resize(64 * 256 * 8); hipMemcpy(mag.data(), out, mag.size() * 4, hipMemcpyDeviceToHost);
  return (double)blocks * 256.0 * 4.0 * iters / (ms * 1e-3);
}
// the same four chains per lane on 9 x 29-bit limbs (fq29_mul): same operands, so the canonical results equal k_rate's
__global__ void __launch_bounds__(256) k_rate29(const uint32_t *__restrict__ seed, int iters, uint32_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  fq29 a[4], b;
  for (int k = 0; k < 4; k++) a[k] = fq29_from_fe(fe_load(seed + (size_t)((t + 17 * k) & 1023) * 8));
  b = fq29_from_fe(fe_load(seed + (size_t)((t * 7 + 3) & 1023) * 8));
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = fq29_mul(a[k], b);
  }
  const fq29 r = fq29_add(fq29_add(a[0], a[1]), fq29_add(a[2], a[3]));       // magnitude 4
  fe_store(out + (size_t)t * 8, fq_to_fe(fq29_to_fq26(r)));
}
static double run29(const uint32_t *seed, uint32_t *out, std::vector<uint32_t> &res) {
  const int blocks = 256 * 4 * 8 / 4 * 2, iters = 2000;
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  k_rate29<<<blocks, 256>>>(seed, 8, out);
  hipEventRecord(e0);
  k_rate29<<<blocks, 256>>>(seed, iters, out);
  hipEventRecord(e1); hipEventSynchronize(e1);
  float ms = 0; hipEventElapsedTime(&ms, e0, e1);
  res.resize((size_t)blocks * 256 * 8); hipMemcpy(res.data(), out, res.size() * 4, hipMemcpyDeviceToHost);
  hipEventDestroy(e0); hipEventDestroy(e1);
  return (double)blocks * 256.0 * 4.0 * iters / (ms * 1e-3);
}
// dependent chains on 9 x 29-bit limbs.  MODE 0: r = fq29_mul(r, b)   1: r = fq29_sqr(r)
template <int MODE> __global__ void __launch_bounds__(256) k_chain29(const uint32_t *__restrict__ seed, int iters, uint32_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  fq29 r = fq29_from_fe(fe_load(seed + (size_t)((t + 40) & 1023) * 8));
  const fq29 b = fq29_from_fe(fe_load(seed + (size_t)((t * 7 + 3) & 1023) * 8));
  for (int i = 0; i < iters; i++) r = MODE == 0 ? fq29_mul(r, b) : fq29_sqr(r);
  fe_store(out + (size_t)t * 8, fq_to_fe(fq29_to_fq26(r)));
}
template <int MODE> void chain29_row(const char *name, const uint32_t *seed, uint32_t *out) {
  const int iters = 4000;
  printf("%-34s", name);
  for (int w = 1; w <= 8; w *= 2) {
    const int blocks = 256 * w;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    k_chain29<MODE><<<blocks, 256>>>(seed, 8, out);
    hipEventRecord(e0);
    k_chain29<MODE><<<blocks, 256>>>(seed, iters, out);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms = 0; hipEventElapsedTime(&ms, e0, e1);
    printf("  %7.1f", (double)ms * 1e6 / (double)iters);
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  printf("\n");
}
// ---- dependent-chain mode: what ONE chain per lane costs when 1, 2, 4 or 8 wavefronts share a SIMD (the bucket reduction's kernels run at 1).
// MODE 0: r = fq_mul(r, b)   1: (r, s) = fq_mul2(r, b, s, b): two chains per lane   2: r = fq_sqr(r)   3: (r, s) = fq_sqr2(r, s)
// MODE 4: acc = xyzz_add(acc, q)   5: acc = xyzz_add_chain(acc, q)   (14 products per step)
// MODE 6: r = fq_mul_lone(r, b)   7 / 8: acc = xyzz_add_quad(acc, q) on fq_mul / on fq_mul_lone (one addition per quad, 4 products deep)
template <int MODE> __global__ void __launch_bounds__(256) k_chain(const uint32_t *__restrict__ seed, int iters, uint32_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, e = MODE >= 7 ? t >> 2 : t;     // the lanes of a quad hold the same operands
  fq r = fq_from_fe(fe_load(seed + (size_t)((e + 40) & 1023) * 8)), s = fq_from_fe(fe_load(seed + (size_t)((e + 57) & 1023) * 8));
  const fq b = fq_from_fe(fe_load(seed + (size_t)((e * 7 + 3) & 1023) * 8));
  if (MODE == 6) {
    for (int i = 0; i < iters; i++) r = fq_mul_lone(r, b);
  } else if (MODE >= 4) {
    xyzz acc = { r, s, b, fq_add(b, r) }, q = { s, b, r, fq_add(s, s) };      // not on the curve: the formulas do not care, and x never repeats
    for (int i = 0; i < iters; i++) {
      if (MODE == 4) xyzz_add(acc, q); else if (MODE == 5) xyzz_add_chain(acc, q); else if (MODE == 7) xyzz_add_quad<false>(acc, q); else xyzz_add_quad<true>(acc, q);
    }
    r = fq_add(fq_add(acc.X, acc.Y), fq_add(acc.ZZ, acc.ZZZ)); s = fq_zero();
  } else {
    for (int i = 0; i < iters; i++) {
      fq x, y;
      if (MODE == 0) r = fq_mul(r, b);
      else if (MODE == 1) { fq_mul2(r, b, s, b, x, y); r = x; s = y; }
      else if (MODE == 2) r = fq_sqr(r);
      else { fq_sqr2(r, s, x, y); r = x; s = y; }
    }
  }
  fe_store(out + (size_t)t * 8, fq_to_fe(fq_add(r, s)));
}
template <int MODE> void chain_row(const char *name, const uint32_t *seed, uint32_t *out, int per_step, std::vector<uint32_t> *keep) {
  const int iters = MODE == 4 || MODE == 5 ? 400 : MODE >= 7 ? 1000 : 4000;
  printf("%-34s", name);
  for (int w = 1; w <= 8; w *= 2) {
    const int blocks = 256 * w;                   // workgroups of four wavefronts, one per SIMD of a CU: w wavefronts per SIMD on 256 CUs
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    k_chain<MODE><<<blocks, 256>>>(seed, 8, out);
    hipEventRecord(e0);
    k_chain<MODE><<<blocks, 256>>>(seed, iters, out);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms = 0; hipEventElapsedTime(&ms, e0, e1);
    printf("  %7.1f", (double)ms * 1e6 / ((double)iters * per_step));
    if (w == 1 && keep) { keep->resize(256 * 256 * 8); hipMemcpy(keep->data(), out, keep->size() * 4, hipMemcpyDeviceToHost); }
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  printf("\n");
}
static int chain_mode(const uint32_t *seed, uint32_t *out) {
  printf("dependent chains: ns per product per wavefront-chain step (time / (steps x products per step)), at wavefronts per SIMD\n");
  printf("%-34s  %7s  %7s  %7s  %7s\n", "", "1", "2", "4", "8");
  std::vector<uint32_t> a4, a5, a7, a8;
  chain_row<0>("fq_mul   one chain per lane", seed, out, 1, nullptr);
  chain_row<1>("fq_mul2  two chains per lane", seed, out, 2, nullptr);
  chain_row<2>("fq_sqr   one chain per lane", seed, out, 1, nullptr);
  chain_row<3>("fq_sqr2  two chains per lane", seed, out, 2, nullptr);
  chain_row<4>("xyzz_add        (14 products)", seed, out, 14, &a4);
  chain_row<5>("xyzz_add_chain  (14 products)", seed, out, 14, &a5);
  chain_row<6>("fq_mul_lone  one chain per lane", seed, out, 1, nullptr);
  chain_row<7>("xyzz_add_quad on fq_mul  (4 deep)", seed, out, 4, &a7);
  chain_row<8>("xyzz_add_quad on fq_mul_lone", seed, out, 4, &a8);
  chain29_row<0>("fq29_mul one chain per lane", seed, out);
  chain29_row<1>("fq29_sqr one chain per lane", seed, out);
  printf("xyzz_add_chain results %s, xyzz_add_quad on fq_mul_lone %s\n", a4 == a5 ? "equal" : "DIFFER", a7 == a8 ? "equal" : "DIFFER");
  return a4 == a5 && a7 == a8 ? 0 : 1;
}
int main(int argc, char **argv) {
  uint32_t *seed, *out;
  hipMalloc(&seed, 1024 * 32); hipMalloc(&out, (size_t)16384 * 256 * 32);
  std::vector<uint32_t> h(1024 * 8);
  uint64_t z = 0x9E3779B97F4A7C15ull;
  for (auto &w : h) { z ^= z << 13; z ^= z >> 7; z ^= z << 17; w = (uint32_t)(z >> 16); }
  for (int i = 0; i < 1024; i++) h[8 * i + 7] &= 0x7FFFFFFFu;
  for (int k = 0; k < 8; k++) { h[k] = k < 7 ? 0xFFFFFFFFu : 0x7FFFFFFFu; h[8 + k] = 0; }     // edge operands
  h[16] = 0xFFFFFC2Eu; h[17] = 0xFFFFFFFEu; for (int k = 2; k < 8; k++) h[16 + k] = 0xFFFFFFFFu;   // p - 1
  hipMemcpy(seed, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  if (argc > 1 && std::string(argv[1]) == "chain") return chain_mode(seed, out);
  std::vector<uint32_t> r0, r1, r2, m0, m1, m2, r3, m3;
  const double g0 = run<0>(seed, out, r0, m0), g1 = run<1>(seed, out, r1, m1), g2 = run<2>(seed, out, r2, m2), g3 = run<3>(seed, out, r3, m3);
  printf("fq_mul_cols (rounds 1-3) %.1f G mulmod/s\n", g0 / 1e9);
  printf("fq_mul (two chains)      %.1f G mulmod/s  results %s, magnitude-8 %s\n", g1 / 1e9, r1 == r0 ? "equal" : "DIFFER", m1 == m0 ? "equal" : "DIFFER");
  printf("v2 (register R0, R1)     %.1f G mulmod/s  results %s, magnitude-8 %s\n", g2 / 1e9, r2 == r0 ? "equal" : "DIFFER", m2 == m0 ? "equal" : "DIFFER");
  printf("v3 (H chain + free low)   %.1f G mulmod/s  results %s, magnitude-8 %s\n", g3 / 1e9, r3 == r0 ? "equal" : "DIFFER", m3 == m0 ? "equal" : "DIFFER");
  std::vector<uint32_t> r29;
  const double g29 = run29(seed, out, r29);
  printf("fq29_mul (9 x 29 limbs)  %.1f G mulmod/s  results %s\n", g29 / 1e9, r29 == r0 ? "equal" : "DIFFER");
  if (r29 != r0) return 1;
  return (r3 == r0 && m3 == m0 && r1 == r0 && r2 == r0 && m1 == m0 && m2 == m0) ? 0 : 1;
}
