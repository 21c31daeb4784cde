// mht_kbest_hypotheses (include/mht_amd.h): the K best global hypotheses of a batch of clusters -- per cluster a depth-first branch
// and bound over "one column per target, no row twice" (mht_kbest.h).  The clusters do not depend on each other, so ONE launch handles
// all of them, ONE CLUSTER PER WORKGROUP and a workgroup is one wavefront: 64 sibling columns are tested per step, the walk itself is
// uniform, and there is no workgroup barrier inside the data-dependent loops.  The cluster's costs, rows, ranking and the per-level
// stack are dynamic LDS.  The seam's index arrays live on the device, so the host cannot size the LDS by the launch's largest cluster
// as the GOSPA launch does: it is sized by the launch's arguments, min(nHyp, 1024) columns and min(nT, 32) targets (45.8 KB at the
// limits, under what a kernel has without raising its limit).  No scratch (tests/test_kbest_resources.py).  A cluster's outputs do
// not depend on its place in the batch.
#include "mht_common.h"
#include "mht_kbest.h"

namespace mht {

__global__ void __launch_bounds__(64) kbest_kernel(const KbestArgs a) {
    extern __shared__ __attribute__((aligned(16))) char kbest_lds[];
    kbest_cluster(a, kbest_carve(kbest_lds, a.max_t, a.max_col, a.depth < MHT_KBEST_MAX_DEPTH ? a.depth : MHT_KBEST_MAX_DEPTH), (int)blockIdx.x);
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_kbest_work_bytes(int32_t nHyp, int32_t nT, int32_t nC, int32_t depth, int32_t K) {
    if (nHyp < 0 || nT < 0 || nC < 0 || depth < 0 || K < 1 || K > MHT_KBEST_MAX_K) return 0;
    return kbest_work_bytes(nT, K);
}

extern "C" int mht_kbest_hypotheses(mht_ctx* ctx, int32_t nHyp, int32_t nT, int32_t nC, int32_t depth, int32_t K, int32_t node_limit,
                                    const int32_t* group_ptr, const int32_t* rows, const double* cost, const int32_t* cluster_ptr,
                                    const int32_t* cluster_targets, int32_t* count, int32_t* status, int32_t* nodes, double* hyp_cost,
                                    double* hyp_prob, int32_t* hyp_sel, double* marginal, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx, "mht_kbest_hypotheses: null context");
    MHT_REQUIRE(nHyp >= 1 && nT >= 1 && nC >= 1, "mht_kbest_hypotheses: %d columns, %d targets, %d clusters: one of each at least", nHyp, nT, nC);
    MHT_REQUIRE(depth >= 0, "mht_kbest_hypotheses: negative depth (%d)", depth);
    MHT_REQUIRE(K >= 1 && K <= MHT_KBEST_MAX_K, "mht_kbest_hypotheses: K is 1 .. %d (got %d)", MHT_KBEST_MAX_K, K);
    MHT_REQUIRE(node_limit >= 1, "mht_kbest_hypotheses: node_limit must be positive (got %d)", node_limit);
    MHT_REQUIRE(group_ptr && cost && cluster_ptr && cluster_targets && (rows || depth == 0), "mht_kbest_hypotheses: null input array");
    MHT_REQUIRE(count && status && nodes && hyp_cost && hyp_prob && hyp_sel && marginal && work, "mht_kbest_hypotheses: null output array");
    MHT_REQUIRE(work_bytes >= kbest_work_bytes(nT, K), "mht_kbest_hypotheses: the workspace has %zu bytes, %zu are needed (mht_kbest_work_bytes)",
                work_bytes, kbest_work_bytes(nT, K));
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    KbestArgs a = {};
    a.nHyp = nHyp; a.nT = nT; a.nC = nC; a.depth = depth; a.K = K; a.node_limit = node_limit;
    a.max_t = nT < MHT_KBEST_MAX_TARGETS ? nT : MHT_KBEST_MAX_TARGETS;
    a.max_col = nHyp < MHT_KBEST_MAX_COLUMNS ? nHyp : MHT_KBEST_MAX_COLUMNS;
    a.group_ptr = group_ptr; a.rows = rows; a.cost = cost; a.cluster_ptr = cluster_ptr; a.cluster_targets = cluster_targets;
    a.count = count; a.status = status; a.nodes = nodes; a.hyp_cost = hyp_cost; a.hyp_prob = hyp_prob; a.hyp_sel = hyp_sel;
    a.marginal = marginal; a.tuples = static_cast<uint16_t*>(work);
    // what no cluster writes: no column for a target beyond count or in no cluster, marginal 0 for a column in no listed hypothesis
    MHT_HIP_CHECK(hipMemsetAsync(hyp_sel, 0xFF, (size_t)K * nT * sizeof(int32_t), ctx->stream));
    MHT_HIP_CHECK(hipMemsetAsync(marginal, 0, (size_t)nHyp * sizeof(double), ctx->stream));
    const int d = depth < MHT_KBEST_MAX_DEPTH ? depth : MHT_KBEST_MAX_DEPTH;
    return launch_kernel(ctx, K_KBEST, kbest_kernel, dim3(nC), dim3(64), kbest_table_bytes(a.max_t, a.max_col, d), false, a);
}
