// ctx.hpp — the library context: one GPU, one stream, a grow-only HBM workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <string>
#include <vector>
#include "../../include/bppp.h"
#include "msm_plan.hpp"   // MsmTune, Carver

// What the last comb_msm launch on a context did (csrc/comb.hip.h; read by bppp_test_last_comb_msm): the kernel it took and how it split the work
struct CombLast {
  int route = -1;                    // -1 none yet, 0 k_comb_msm (wavefront per instance), 1 / 2 k_comb_msm_packed<8 / 16>, 3 k_comb_msm_rows, 4 the same with pairs
  int heavy_first = 0;               // k_comb_msm: the heavy instances of the pairs dispatched first
  uint32_t parts = 0, tparts = 0, wsplit = 0;         // k_comb_msm: wavefronts per instance = term parts x window ranges
  uint32_t chunks = 0, clen = 0, join_lanes = 0;      // rows: partial sums per instance, terms of each, lanes per instance of k_comb_join_rows
};

// What the bucket reduction of the last MSM on a context launched (csrc/msm.hip: msm_reduce, msm_small, msm_finish; read by bppp_test_last_reduce)
struct ReduceLast {
  int route = -1;                    // -1 none yet, 0 the small route (k_msm_small's own tail, k_msm_small_join), 1 k_reduce_groups, 2 k_reduce_marg + k_reduce_tail_quad, 3 k_reduce1 + k_reduce2
  int combine = -1;                  // 1: the windows were combined by k_window_combine, 0: on the host
  int c = 0, W = 0, M = 0;           // window width, windows left for the combine (1 for a registered basis), buckets per window
  int RG = 0, Lw = 0, WPW = 0;       // groups: lanes per window and buckets per lane; wavefront route: buckets per lane, wavefronts per window
  int a = 0, LO = 0, HI = 0, PR = 0, PC = 0, SR = 0, SC = 0, TR = 0, TC = 0;   // marginal route: MargGeom (msm_plan.hpp)
  int S = 0;                         // small route: slices
};

struct bppp_ctx {
  MsmTune tune;
  // Lifetime: the caller's handle holds one reference, every child handle (bppp_nl, bppp_nlb, bppp_ip, bppp_trrp, bppp_basis,
  // bppp_rp) one more.  bppp_ctx_destroy marks the context closed and drops the caller's reference; the stream, the
  // workspaces and the struct itself go when the LAST reference goes, so a child destroyed after its context (a finaliser
  // running in any order) never touches freed memory.  Calls on a child of a closed context fail with BPPP_ERR_ARG.
  std::atomic<int> refs{1};
  std::atomic<bool> closed{false};
  int device = 0;
  hipStream_t stream = nullptr;      // stream all work is issued on
  hipStream_t own_stream = nullptr;  // created by the context (used unless the caller binds its own)
  // second stream + fork / join events, made on first use (ctx_aux): independent halves of ONE call run side by side — the verifier's
  // round-challenge hashing beside its public-scalar kernel (csrc/rp.hip)
  hipStream_t aux_stream = nullptr;
  hipEvent_t aux_fork = nullptr, aux_join = nullptr;
  std::string err;
  // grow-only device workspace, carved per call (no hipMalloc on the steady-state path).  The contract of ws, ws2, mix and pinned, and of the
  // scratch buffers of a range-proof handle (csrc/rp_internal.hpp): no entry point reads a workspace word that the same call has not written;
  // tests/test_gpu_poisoned_workspace.py holds it.
  void *ws = nullptr;
  size_t ws_bytes = 0;
  // second grow-only device buffer for callers that also run an MSM (which carves `ws`)
  void *ws2 = nullptr;
  size_t ws2_bytes = 0;
  // one-shot hook run by msm_run right before the accumulate kernel (the first consumer of the points): bppp_msm uploads the
  // points there, so the 64 B/pair host copy overlaps the digit and sort kernels that need only the scalars
  int (*pre_acc)(void *) = nullptr;
  void *pre_acc_arg = nullptr;
  // pinned host staging for small results
  void *pinned = nullptr;
  size_t pinned_bytes = 0;
  // profiling
  bool profile = false;
  double stage_ms[BPPP_NUM_STAGES] = {0, 0, 0, 0, 0, 0};
  uint64_t calls = 0;
  hipEvent_t ev[BPPP_NUM_STAGES + 1] = {};
  bool ev_ready = false;
  // grow-only device buffer of the multi-setup verifier (csrc/rpmixed.hip): the one MSM's input and every group's shared scalars, which
  // must outlive the next group's assembly in ws2
  void *mix = nullptr;
  size_t mix_bytes = 0;
  uint64_t last_mixed_terms = 0;     // terms of the last multi-setup MSM (bppp_test_last_mixed_msm_terms)
  int last_sort_ranges = -1;         // bucket ranges Q of the last general-pipeline MSM's scatter: 0 k_scatter, 2 / 4 k_scatter_ranges (bppp_test_last_sort_ranges)
  int last_scatter_one_read = -1;    // 1: the last general-pipeline MSM's scatter was k_scatter_one_read, 0: any other (bppp_test_last_scatter_one_read)
  int last_hist16 = -1;              // 1: the last general-pipeline MSM's sort kept 16-bit per-chunk counts and prefixes (MsmPlan::hist16), 0: 32-bit words (bppp_test_last_hist16)
  int last_acc_sized = -1;           // 1: the last general-pipeline MSM accumulated whole buckets by size (k_order, k_acc_points_sized), 0: slices (bppp_test_last_acc_sized)
  int last_acc_fq29 = -1;            // 1: the last general-pipeline MSM ran k_acc_points_sized29 or k_acc_points_sized29_fast (fq29 accumulator), 0: any other accumulate kernel (bppp_test_last_acc_fq29)
  int last_windows = -1;             // digit rows W per scalar of the last MSM's plan, either route (bppp_test_last_windows)
  CombLast last_comb;                // the last comb_msm launch (bppp_test_last_comb_msm)
  ReduceLast last_reduce;            // the last MSM's bucket reduction and window combine (bppp_test_last_reduce)
  // The last general-pipeline MSM (msm_run_ex; read by bppp_test_last_msm_layout / _copy, which carve the workspace again from the plan and read
  // the stages back): valid until a call that lays `ws` out differently — the small route clears it, the tests read directly after their MSM
  bool last_msm_valid = false;
  bppp::MsmPlan last_msm_plan{};
  size_t last_msm_n = 0, last_msm_batch = 0, last_msm_table_stride = 0;
  int last_msm_shared_points = 0;
  size_t sort_lds_set = 0;           // largest dynamic-LDS size set on the MSM's sort kernels (hipFuncSetAttribute once, not per call)
};

namespace bppp {

inline int fail(bppp_ctx *ctx, int code, const std::string &msg) {
  if (ctx) ctx->err = msg;
  return code;
}
#define BPPP_HIP(ctx, call)                                                                    \
  do {                                                                                         \
    hipError_t _e = (call);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return bppp::fail(ctx, BPPP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
  } while (0)

void ctx_retain(bppp_ctx *ctx);
void ctx_release(bppp_ctx *ctx);          // the last release tears the context down
inline bool ctx_closed(const bppp_ctx *ctx) { return !ctx || ctx->closed.load(); }
int ctx_aux(bppp_ctx *ctx);               // creates aux_stream and its two events if needed
// nothing of a call is in flight once it has returned: both streams drained (the verifier's sliced uploads of host files run on the
// second) and the runtime's last-error slot cleared; a no-op on a closed context
inline void ctx_drain(bppp_ctx *ctx) {
  if (ctx_closed(ctx)) return;
  hipStreamSynchronize(ctx->stream);
  if (ctx->aux_stream) hipStreamSynchronize(ctx->aux_stream);
  (void)hipGetLastError();
}
int ensure_workspace(bppp_ctx *ctx, size_t bytes);
int ensure_pinned(bppp_ctx *ctx, size_t bytes);
int ensure_scratch(bppp_ctx *ctx, size_t bytes);
void prof_mark(bppp_ctx *ctx, int idx);   // record event idx on the stream when profiling
void prof_collect(bppp_ctx *ctx, int nmarks);

}  // namespace bppp
