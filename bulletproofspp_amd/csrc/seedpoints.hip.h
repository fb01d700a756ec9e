// seedpoints.hip.h — getPoints (app/Main.hs:68-72) on the device: the basis stream h : g : hs ++ gs of a setup from its basisSeed.
//
// Candidate n of seed s is x = decode (SHA-256 (s <> show n)) mod p (decode = Binary (Prime p), src/Encoding.hs:75-79); it is a point
// iff x^3 + 7 is a square, with the even root as y (the choice of bppp_lift_x_device), and the stream is `catMaybes` over n = 0, 1, ...:
// the k-th point is the k-th candidate that lifts.  That is an ORDERED compaction, done here in passes over a chunk of candidates:
//
//   k_seed_candidates  one lane per candidate: the message tail (seed bytes after its last full block, digits of n, padding), one or
//                      two compressions from the seed's midstate, decode, reduce, x^3 + 7, fq_sqrt_candidate, the check, the even
//                      root; the point — or 64 zero bytes — goes to slot i of the pass's scratch, the workgroup's count to cnt[block]
//   k_seed_scan        ONE workgroup: exclusive scan of the workgroup counts, and the pass's record (points taken)
//   k_seed_scatter     one lane per candidate again: ballot + popcount inside the wavefront, LDS across the four wavefronts, the scanned
//                      offset of the workgroup: the lane's slot is the number of accepted candidates before it; plain vector stores;
//                      the lane that fills the last wanted slot writes its own index + 1 into the record
//
// No atomics, no dependence on scheduling: the same call writes the same bytes.  The host reads the 16-byte record after each pass and
// launches another only when the stream came up short.  The message building and hashing (seed_candidate_limbs) is one BPPP_HD
// function: bppp_seed_candidate_x runs it on the host, the CPU tier tests it there.
#pragma once
#include <stdint.h>
#include <string.h>
#include "ctx.hpp"
#include "ec.hip.h"
#include "sha256.hip.h"

namespace bppp {

// the seed as every candidate's message starts: state after its full 64-byte blocks, the rest (under 64 bytes) as big-endian words
struct SeedMsg {
  uint32_t mid[8];
  uint32_t tail[16];       // bytes past tail_len are zero
  uint32_t tail_len;       // seed_len & 63
  uint32_t seed_len;       // <= SEED_MAX_LEN
};
static constexpr size_t SEED_MAX_LEN = 4096;

inline void seed_msg_init(SeedMsg &M, const uint8_t *seed, size_t seed_len) {
  sha256_init(M.mid);
  size_t off = 0;
  for (; off + 64 <= seed_len; off += 64) {
    uint32_t w[16];
    for (int i = 0; i < 16; i++) {
      const uint8_t *p = seed + off + 4 * i;
      w[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
    sha256_compress(M.mid, w);
  }
  for (int i = 0; i < 16; i++) M.tail[i] = 0;
  M.tail_len = (uint32_t)(seed_len - off);
  M.seed_len = (uint32_t)seed_len;
  for (uint32_t j = 0; j < M.tail_len; j++) M.tail[j >> 2] |= (uint32_t)seed[off + j] << (24 - 8 * (j & 3));
}

// SHA-256 (seed <> decimal n), as the state words h[8]
BPPP_HD void seed_candidate_digest(const SeedMsg &M, uint64_t n, uint32_t h[8]) {
  uint32_t w[32];
  for (int i = 0; i < 16; i++) { w[i] = M.tail[i]; w[16 + i] = 0; }
  uint8_t dig[20];
  uint32_t nd = 0;
  do { dig[nd++] = (uint8_t)('0' + (uint32_t)(n % 10)); n /= 10; } while (n);
  uint32_t pos = M.tail_len;
  for (uint32_t k = 0; k < nd; k++, pos++) w[pos >> 2] |= (uint32_t)dig[nd - 1 - k] << (24 - 8 * (pos & 3));
  w[pos >> 2] |= 0x80u << (24 - 8 * (pos & 3));
  const bool two = pos + 9 > 64;                       // 0x80 and the 8 length bytes do not fit the first block
  w[two ? 31 : 15] = (M.seed_len + nd) * 8;            // < 2^32: the high length word stays zero
  for (int i = 0; i < 8; i++) h[i] = M.mid[i];
  sha256_compress(h, w);
  if (two) sha256_compress(h, w + 16);
}

// v (8 little-endian 32-bit limbs, < 2^256 < 2 p) mod p: one conditional subtraction
BPPP_HD void seed_reduce_p(uint32_t v[8]) {
  const uint32_t P0 = 0xFFFFFC2Fu, P1 = 0xFFFFFFFEu;
  uint32_t t[8];
  uint64_t borrow = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)v[i] - (i == 0 ? P0 : i == 1 ? P1 : 0xFFFFFFFFu) - borrow;
    t[i] = (uint32_t)d;
    borrow = (d >> 32) & 1;
  }
  if (!borrow) for (int i = 0; i < 8; i++) v[i] = t[i];
}

// x of candidate n, canonical, 8 x 32-bit limbs
BPPP_HD void seed_candidate_limbs(const SeedMsg &M, uint64_t n, uint32_t x[8]) {
  uint32_t h[8];
  seed_candidate_digest(M, n, h);
  sha256_digest_to_limbs(h, x);
  seed_reduce_p(x);
}

// pointX on a digest: decode, reduce, y = even root of x^3 + 7 if there is one
BPPP_DI bool seed_lift_digest(const uint32_t h[8], fe &xe, aff &pt) {
  sha256_digest_to_limbs(h, xe.v);
  seed_reduce_p(xe.v);
  const fq x = fq_from_fe(xe);
  fq seven = fq_zero(); seven.n[0] = 7;
  const fq rhs = fq_add(fq_mul(fq_sqr(x), x), seven);        // magnitude 2
  const fq acc = fq_sqrt_candidate(rhs);
  const bool ok = fq_normalizes_to_zero(fq_sub<2>(fq_sqr(acc), rhs));
  fq y = fq_normalize(acc);
  if (y.n[0] & 1u) y = fq_normalize(fq_neg<1>(y));
  pt.x = x; pt.y = y;
  return ok;
}

static constexpr uint32_t SEED_WG = 256;                     // lanes per workgroup of the candidate and scatter kernels
static constexpr uint32_t SEED_SCAN_WG = 1024;
static constexpr uint64_t SEED_CHUNK_MAX = 1u << 20;         // candidates per pass: 64 MB of scratch at 64 B each

// exclusive prefix of `v` over the workgroup's lanes (WG / 64 wavefronts; `part` has one word per wavefront); total = the sum
template <uint32_t WG> BPPP_DI uint32_t seed_wg_exclusive(uint32_t v, uint32_t *part, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(inc, d, 64); if ((int)lane >= d) inc += u; }
  __syncthreads();                                           // `part` may still be read from an earlier call
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  uint32_t before = 0; total = 0;
#pragma unroll
  for (uint32_t k = 0; k < WG / 64; k++) { const uint32_t c = part[k]; if (k < wave) before += c; total += c; }
  return before + inc - v;
}
// the same for one accept flag per lane: ballot and popcount in place of the shuffles
BPPP_DI uint32_t seed_wg_rank(bool ok, uint32_t *part, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(ok);
  __syncthreads();
  if (lane == 0) part[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0; total = 0;
#pragma unroll
  for (uint32_t k = 0; k < SEED_WG / 64; k++) { const uint32_t c = part[k]; if (k < wave) before += c; total += c; }
  return before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(SEED_WG) k_seed_candidates(SeedMsg M, uint64_t first, uint32_t chunk, uint32_t *__restrict__ scratch, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t part[SEED_WG / 64];
  const uint32_t i = blockIdx.x * SEED_WG + threadIdx.x;
  bool ok = false;
  if (i < chunk) {
    uint32_t h[8];
    seed_candidate_digest(M, first + i, h);
    fe xe; aff pt;
    ok = seed_lift_digest(h, xe, pt);
    if (!ok) pt = aff_inf();
    aff_store(scratch + (size_t)i * 16, pt);
  }
  uint32_t total;
  seed_wg_rank(ok, part, total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// rec[0] = points this pass takes (min(accepted, want)), rec[1] = candidates consumed (the whole chunk unless the scatter finds the last wanted slot)
__global__ void __launch_bounds__(SEED_SCAN_WG) k_seed_scan(const uint32_t *__restrict__ cnt, uint32_t nblk, uint32_t chunk, uint64_t want, uint32_t *__restrict__ offs,
                                                           uint64_t *__restrict__ rec) {
  __shared__ uint32_t part[SEED_SCAN_WG / 64];
  const uint32_t per = (nblk + SEED_SCAN_WG - 1) / SEED_SCAN_WG, lo = threadIdx.x * per, hi = lo + per < nblk ? lo + per : nblk;
  uint32_t s = 0;
  for (uint32_t b = lo; b < hi; b++) s += cnt[b];
  uint32_t total;
  uint32_t run = seed_wg_exclusive<SEED_SCAN_WG>(s, part, total);
  for (uint32_t b = lo; b < hi; b++) { offs[b] = run; run += cnt[b]; }
  if (threadIdx.x == 0) { rec[0] = total < want ? total : want; rec[1] = chunk; }
}

__global__ void __launch_bounds__(SEED_WG) k_seed_scatter(const uint32_t *__restrict__ scratch, const uint32_t *__restrict__ offs, uint32_t chunk, uint64_t want,
                                                          uint32_t *__restrict__ out, uint64_t *__restrict__ rec) {
  __shared__ uint32_t part[SEED_WG / 64];
  const uint32_t i = blockIdx.x * SEED_WG + threadIdx.x;
  uint4 v[4];
  bool ok = false;
  if (i < chunk) {
    const uint4 *p = reinterpret_cast<const uint4 *>(scratch + (size_t)i * 16);
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = p[k];
    ok = (v[0].x | v[0].y | v[0].z | v[0].w | v[1].x | v[1].y | v[1].z | v[1].w | v[2].x | v[2].y | v[2].z | v[2].w | v[3].x | v[3].y | v[3].z | v[3].w) != 0;
  }
  uint32_t total;
  const uint64_t slot = (uint64_t)offs[blockIdx.x] + seed_wg_rank(ok, part, total);
  if (ok && slot < want) {
    uint4 *q = reinterpret_cast<uint4 *>(out + (size_t)slot * 16);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = v[k];
    if (slot + 1 == want) rec[1] = (uint64_t)i + 1;          // one lane at most
  }
}

// candidates of one pass for `want` more points: every second candidate lifts, so 2 want plus four standard deviations and a little
inline uint64_t seed_chunk_for(uint64_t want) {
  if (want >= SEED_CHUNK_MAX) return SEED_CHUNK_MAX;
  uint64_t r = 1;
  while (r * r < 2 * want) r++;
  const uint64_t c = 2 * want + 4 * r + 64;
  return c < SEED_CHUNK_MAX ? c : SEED_CHUNK_MAX;
}
inline size_t seed_scratch_bytes(uint64_t chunk) {            // points | counts | offsets | record
  const size_t nblk = (size_t)((chunk + SEED_WG - 1) / SEED_WG);
  return (size_t)chunk * 64 + 2 * ((nblk * 4 + 255) & ~(size_t)255) + 256;
}

// `count` points of the stream from candidate `first` into d_out ([count][16] words); *next = the candidate after the last one taken.
// chunk_forced = 0: passes sized by seed_chunk_for, else that many candidates per pass (tests); `scratch` holds seed_scratch_bytes of the
// largest pass.  The stream ends with candidate 2^64 - 2, so that *next always names a candidate: BPPP_ERR_ARG if it ends first.
inline int seed_points_run(bppp_ctx *ctx, const SeedMsg &M, uint64_t first, size_t count, uint64_t chunk_forced, void *scratch, void *d_out, uint64_t *next) {
  hipStream_t st = ctx->stream;
  uint64_t cur = first, done = 0;
  while (done < count) {
    const uint64_t want = count - done, avail = UINT64_MAX - cur;
    if (!avail) return fail(ctx, BPPP_ERR_ARG, "points_from_seed: the stream ends at candidate 2^64 - 2 before the points asked for");
    uint64_t chunk = chunk_forced ? chunk_forced : seed_chunk_for(want);
    if (chunk > avail) chunk = avail;
    const uint32_t nblk = (uint32_t)((chunk + SEED_WG - 1) / SEED_WG);
    const size_t words = ((size_t)nblk * 4 + 255) & ~(size_t)255;
    uint32_t *pts = (uint32_t *)scratch, *cnt = (uint32_t *)((char *)scratch + (size_t)chunk * 64), *offs = (uint32_t *)((char *)cnt + words);
    uint64_t *rec = (uint64_t *)((char *)offs + words);
    uint32_t *out = (uint32_t *)d_out + (size_t)done * 16;
    k_seed_candidates<<<dim3(nblk), dim3(SEED_WG), 0, st>>>(M, cur, (uint32_t)chunk, pts, cnt);
    k_seed_scan<<<dim3(1), dim3(SEED_SCAN_WG), 0, st>>>(cnt, nblk, (uint32_t)chunk, want, offs, rec);
    k_seed_scatter<<<dim3(nblk), dim3(SEED_WG), 0, st>>>(pts, offs, (uint32_t)chunk, want, out, rec);
    BPPP_HIP(ctx, hipGetLastError());
    uint64_t h_rec[2] = {0, 0};
    BPPP_HIP(ctx, hipMemcpyAsync(h_rec, rec, 16, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
    if (h_rec[0] > want || h_rec[1] > chunk || !h_rec[1]) return fail(ctx, BPPP_ERR_HIP, "points_from_seed: bad pass record");
    done += h_rec[0];
    cur += h_rec[1];
  }
  if (next) *next = cur;
  return BPPP_OK;
}
}  // namespace bppp
