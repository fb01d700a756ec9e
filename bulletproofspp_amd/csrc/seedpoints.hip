// seedpoints.hip — the C ABI of getPoints (app/Main.hs:68-72): bppp_seed_candidate_x on the host, bppp_points_from_seed{,_device} on the
// GPU.  The kernels and the pass loop: csrc/seedpoints.hip.h.
#include <vector>
#include "seedpoints.hip.h"

using namespace bppp;

static bool seed_args_ok(const uint8_t *seed, size_t seed_len) { return (seed || !seed_len) && seed_len <= SEED_MAX_LEN; }

namespace bppp {
// `count` points from candidate `first` into HBM; the pass scratch is the context's second workspace
int seed_points_device(bppp_ctx *ctx, const uint8_t *seed, size_t seed_len, uint64_t first, size_t count, void *d_points_xy, uint64_t *next) {
  if (!seed_args_ok(seed, seed_len)) return fail(ctx, BPPP_ERR_ARG, "points_from_seed: seed must be at most 4096 bytes (NULL only when empty)");
  if (!count) { if (next) *next = first; return BPPP_OK; }
  if (!d_points_xy) return fail(ctx, BPPP_ERR_ARG, "points_from_seed: null output");
  if (count > UINT64_MAX - first) return fail(ctx, BPPP_ERR_ARG, "points_from_seed: the stream ends at candidate 2^64 - 2 before the points asked for");
  SeedMsg M;
  seed_msg_init(M, seed, seed_len);
  { int rc = ensure_scratch(ctx, seed_scratch_bytes(seed_chunk_for(count))); if (rc) return rc; }
  return seed_points_run(ctx, M, first, count, 0, ctx->ws2, d_points_xy, next);
}
}  // namespace bppp

extern "C" {

int bppp_seed_candidate_x(const uint8_t *seed, size_t seed_len, uint64_t n, uint64_t out_x[4]) {
  if (!seed_args_ok(seed, seed_len) || !out_x) return BPPP_ERR_ARG;
  SeedMsg M;
  seed_msg_init(M, seed, seed_len);
  uint32_t x[8];
  seed_candidate_limbs(M, n, x);
  for (int i = 0; i < 4; i++) out_x[i] = ((uint64_t)x[2 * i + 1] << 32) | x[2 * i];
  return BPPP_OK;
}

int bppp_points_from_seed_device(bppp_ctx *ctx, const uint8_t *seed, size_t seed_len, uint64_t first_candidate, size_t count, void *d_points_xy,
                                 uint64_t *next_candidate) {
  if (!ctx || ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, BPPP_ERR_HIP, "hipSetDevice failed");
  return seed_points_device(ctx, seed, seed_len, first_candidate, count, d_points_xy, next_candidate);
}

int bppp_points_from_seed(bppp_ctx *ctx, const uint8_t *seed, size_t seed_len, uint64_t first_candidate, size_t count, uint64_t *points_xy,
                          uint64_t *next_candidate) {
  if (!ctx || ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, BPPP_ERR_HIP, "hipSetDevice failed");
  if (count && !points_xy) return fail(ctx, BPPP_ERR_ARG, "points_from_seed: null output");
  if (count >= ((size_t)1 << 40)) return fail(ctx, BPPP_ERR_ARG, "points_from_seed: too many points");
  void *d = nullptr;
  if (count) BPPP_HIP(ctx, hipMalloc(&d, count * 64));
  int rc = seed_points_device(ctx, seed, seed_len, first_candidate, count, d, next_candidate);
  if (!rc && count && (hipMemcpyAsync(points_xy, d, count * 64, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess))
    rc = fail(ctx, BPPP_ERR_HIP, "points_from_seed: download failed");
  if (d) hipFree(d);
  return rc;
}

}  // extern "C"
