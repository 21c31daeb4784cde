// TEST-ONLY host build of csrc/mht_kbest.h: kbest_cluster itself -- the code the wavefront of kbest_kernel (mht_kbest.hip) runs for its
// cluster, with the 64 lanes as a loop -- compiled for the CPU and run over the clusters of one call in turn, so that the search, its
// bound, its limits and its outputs are checked against tests/kbest_ref.py without a GPU (tests/test_kbest_cpu.py), and so that it
// defines what the device must give bit for bit: costs, tuples, count, status and nodes, a node limit's partial list included.  The
// seam's own checks and fills are made here as mht_kbest_hypotheses makes them.  With KBEST_HOST_MAIN: a stand-alone program over
// built-in cases, for a sanitizer build.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../pymht_amd/csrc/mht_kbest.h"

using namespace mht;

// The seam with host arrays.  Returns 0, or -1 for what the seam refuses (nothing is written).
extern "C" int kbest_host(int32_t nHyp, int32_t nT, int32_t nC, int32_t depth, int32_t K, int32_t node_limit, const int32_t* group_ptr,
                          const int32_t* rows, const double* cost, const int32_t* cluster_ptr, const int32_t* cluster_targets, int32_t* count,
                          int32_t* status, int32_t* nodes, double* hyp_cost, double* hyp_prob, int32_t* hyp_sel, double* marginal) {
    if (nHyp < 1 || nT < 1 || nC < 1 || depth < 0 || K < 1 || K > MHT_KBEST_MAX_K || node_limit < 1) return -1;
    if (!group_ptr || !cost || !cluster_ptr || !cluster_targets || (!rows && depth) || !count || !status || !nodes || !hyp_cost || !hyp_prob ||
        !hyp_sel || !marginal)
        return -1;
    KbestArgs a = {};
    a.nHyp = nHyp; a.nT = nT; a.nC = nC; a.depth = depth; a.K = K; a.node_limit = node_limit;
    a.max_t = nT < MHT_KBEST_MAX_TARGETS ? nT : MHT_KBEST_MAX_TARGETS;
    a.max_col = nHyp < MHT_KBEST_MAX_COLUMNS ? nHyp : MHT_KBEST_MAX_COLUMNS;
    a.group_ptr = group_ptr; a.rows = rows; a.cost = cost; a.cluster_ptr = cluster_ptr; a.cluster_targets = cluster_targets;
    a.count = count; a.status = status; a.nodes = nodes; a.hyp_cost = hyp_cost; a.hyp_prob = hyp_prob; a.hyp_sel = hyp_sel;
    a.marginal = marginal;
    std::vector<uint16_t> tuples(kbest_work_bytes(nT, K) / 2);
    a.tuples = tuples.data();
    memset(hyp_sel, 0xFF, (size_t)K * nT * sizeof(int32_t));
    memset(marginal, 0, (size_t)nHyp * sizeof(double));
    const int d = depth < MHT_KBEST_MAX_DEPTH ? depth : MHT_KBEST_MAX_DEPTH;
    // (exactly the bytes the launch gets: a carve that overruns them is an error a sanitizer build sees)
    std::vector<char> lds(kbest_table_bytes(a.max_t, a.max_col, d));
    for (int c = 0; c < nC; ++c) kbest_cluster(a, kbest_carve(lds.data(), a.max_t, a.max_col, d), c);
    return 0;
}

extern "C" uint64_t kbest_table_bytes_host(int32_t max_t, int32_t max_col, int32_t depth) { return kbest_table_bytes(max_t, max_col, depth); }
extern "C" uint64_t kbest_work_bytes_host(int32_t nT, int32_t K) { return kbest_work_bytes(nT, K); }

#ifdef KBEST_HOST_MAIN
#include <cstdio>
#include <random>
// Random clusters of every shape class the tests use (group sizes around the wavefront, equal costs, non-finite costs, empty columns,
// limits + 1, bad rows, a tight node limit), run for their memory accesses; prints a checksum.
int main() {
    std::mt19937 rng(7);
    long long sum = 0;
    for (int it = 0; it < 400; ++it) {
        const int sizes_pool[] = {1, 2, 3, 5, 63, 64, 65, 130};
        int nC = 1 + (int)(rng() % 4), depth = (int)(rng() % 5), K = it % 3 == 0 ? 64 : 1 + (int)(rng() % 64);
        if (it % 50 == 49) depth = MHT_KBEST_MAX_DEPTH + 1;
        std::vector<int32_t> gp{0}, cp{0}, ct;
        for (int c = 0; c < nC; ++c) {
            int n = 1 + (int)(rng() % 4);
            if (it % 40 == 39 && c == 0) n = MHT_KBEST_MAX_TARGETS + 1;
            if (it % 40 == 38 && c == 0) n = MHT_KBEST_MAX_TARGETS;
            for (int j = 0; j < n; ++j) {
                int s = n > 8 ? 2 : sizes_pool[rng() % 8];
                if (it % 40 == 37 && c == 0 && j == 0) s = MHT_KBEST_MAX_COLUMNS + 1;
                if (it % 40 == 36 && c == 0 && j == 0) s = 0;
                ct.push_back((int32_t)gp.size() - 1);
                gp.push_back(gp.back() + s);
            }
            cp.push_back((int32_t)ct.size());
        }
        const int nT = (int)ct.size(), nHyp = gp.back() > 0 ? gp.back() : 1;
        std::vector<double> cost(nHyp);
        std::vector<int32_t> rows((size_t)(depth ? depth : 1) * nHyp, -1);
        for (int i = 0; i < nHyp; ++i) {
            cost[i] = it % 4 == 0 ? (double)(rng() % 3) : (double)(rng() % 100000) / 977.0 - 20.0;
            if (rng() % 37 == 0) cost[i] = rng() % 2 ? NAN : HUGE_VAL;
            for (int d = 0; d < depth; ++d)
                if (rng() % 3) rows[(size_t)d * nHyp + i] = (int32_t)(rng() % (it % 7 == 0 ? MHT_KBEST_MAX_ROWS : 12));
            if (depth && it % 45 == 44 && i == nHyp / 2) rows[i] = rng() % 2 ? MHT_KBEST_MAX_ROWS : -2;
        }
        std::vector<int32_t> count(nC), status(nC), nodes(nC), sel((size_t)K * nT);
        std::vector<double> hc((size_t)K * nC), hp((size_t)K * nC), mg(nHyp);
        const int limit = it % 9 == 0 ? 1 + (int)(rng() % 200) : 1 << 20;
        if (kbest_host(nHyp, nT, nC, depth, K, limit, gp.data(), rows.data(), cost.data(), cp.data(), ct.data(), count.data(), status.data(),
                       nodes.data(), hc.data(), hp.data(), sel.data(), mg.data()) != 0)
            return 1;
        for (int c = 0; c < nC; ++c) sum += count[c] + 7 * status[c] + nodes[c];
    }
    printf("kbest_host: 400 calls, checksum %lld\n", sum);
    return 0;
}
#endif
