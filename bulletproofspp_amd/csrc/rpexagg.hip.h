// rpexagg.hip.h — what the half-aggregate (csrc/rpexagg.hip, which defines it) lends to the block call (csrc/rpblock.hip): the hash tree over the
// whole job, the scalars that follow from its root, and the two MSM terms of a key under the aggregation coefficients.  Host declarations only;
// everything is queued on the context's stream.
#pragma once
#include "msm_plan.hpp"
#include "rpexcess_shared.hip.h"

namespace bppp {
namespace exagg {

static constexpr uint32_t AGG_ROW = BPPP_RP_EXCESS_KEY_BYTES;     // an R row of the aggregate: the 33 bytes a signature holds
static constexpr uint32_t TREE_TILE = 256;                        // leaves one workgroup of k_rp_exagg_tree reduces (DESIGN.md says why)

// the arrays of one job: leaves [nkeys][8] (digests as big-endian words), the tree's two levels in flight, s_agg as a scalar (zero when it is
// >= n, which raises flag[0]), rho [2][8] (rho_A and rho_A s_agg: the block call alone) and sigx [chunk][65], the R rows of a pass as signatures
// with s = 0 for the stage the 65-byte signatures take (exkeys::key_stage).  root: where the tree left its last node.
struct AggWork {
  uint32_t *leaves, *lvl[2], *sagg, *rho, *flag;
  uint8_t *sigx;
  const uint32_t *root;
};
void agg_carve(Carver &cv, size_t nkeys, size_t chunk, AggWork &W);
// leaf_i over (rrows + i * rstride, the canonical bytes of key i, msg i) for the whole job, then the tree: W.root
int commit_tree(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *rrows, uint32_t rstride, AggWork &W);
// W.sagg and W.flag from the 32 bytes behind the aggregate's rows
int sagg_launch(bppp_ctx *ctx, const uint8_t *s32, const AggWork &W);
// W.rho: rho_A over (seed in HBM, nkeys, root, the 32 bytes as they stand), and rho_A s_agg; after commit_tree and sagg_launch
int rho_launch(bppp_ctx *ctx, const uint8_t *d_seed, size_t nkeys, const uint8_t *s32, const AggWork &W);
// sigx [n][65] = row || put (0)
int expand_launch(bppp_ctx *ctx, size_t n, const uint8_t *rrows, uint8_t *sigx);
// keys [i0, i0 + n) of a job of ntotal after exkeys::key_stage: z_i (times rho when not NULL), terms 2t and 2t + 1 in k_rp_excess_weights' layout
// (sc, pt; both NULL: none), the product column - z_i s_i (prods; NULL: none); any[0] is raised by a key whose verdict is already taken
int weights_launch(bppp_rp *rp, size_t n, uint64_t i0, uint64_t ntotal, const uint32_t *root, const uint32_t *rho, const uint32_t *X, const uint32_t *pre, const uint32_t *c,
                   const uint32_t *sp, const uint32_t *R, uint32_t *prods, uint32_t *sc, uint32_t *pt, uint32_t *any);
// bppp_rp_excess_halfagg_verify_device after its argument checks; every buffer in HBM, accept / status / combined_xy on the host (the last two may be NULL)
int verify_run(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *agg, int *accept, uint32_t *status, uint64_t *combined_xy);

}  // namespace exagg
}  // namespace bppp
