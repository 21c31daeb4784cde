// mht_gospa_steps (include/mht_amd.h): GOSPA of a batch of steps against ground truth -- per step one distance between the set of
// estimates and the set of true positions, split into localisation error, missed targets and false tracks.  A step is an optimal
// partial assignment (mht_gospa.h); the steps do not depend on each other, so ONE launch handles all of them, ONE STEP PER WORKGROUP
// and a workgroup is one wavefront: the sweep over the columns is strided over the lanes, its arg-min is a wavefront reduction, and
// there is no workgroup barrier inside the data-dependent loops.  The prices and the search tables are dynamic LDS sized by the
// launch's largest step (56 KB at 2048 x 2048, raised through launch_kernel under K_GOSPA); the positions stay in global memory (a
// sweep reads one row and a strided run of columns).  No scratch (tests/test_gospa_resources.py).  A step's outputs do not depend on
// its place in the batch.
#include "mht_common.h"
#include "mht_gospa.h"

namespace mht {

struct GospaArgs {
    const int32_t* est_off;      // dev [n_steps + 1]
    const int32_t* tru_off;      // dev [n_steps + 1]
    const double* est_xy;
    const double* tru_xy;
    double cp, lim;
    int32_t p, max_rows, max_cols;
    double* step_out;
    int32_t* count_out;
    int32_t* match_out;
};

__global__ void __launch_bounds__(64) gospa_kernel(const GospaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char gospa_lds[];
    const int step = blockIdx.x;
    const int e0 = a.est_off[step], n = a.est_off[step + 1] - e0;
    const int t0 = a.tru_off[step], m = a.tru_off[step + 1] - t0;
    const bool rows_are_est = n <= m;      // the smaller side are the rows
    const double* est = a.est_xy + 2 * (size_t)e0;
    const double* tru = a.tru_xy + 2 * (size_t)t0;
    GospaStep s;
    s.row_xy = rows_are_est ? est : tru;
    s.col_xy = rows_are_est ? tru : est;
    s.n_rows = rows_are_est ? n : m;
    s.n_cols = rows_are_est ? m : n;
    s.p = a.p;
    s.cp = a.cp;
    s.lim = a.lim;
    gospa_step(s, gospa_carve(gospa_lds, a.max_rows, a.max_cols), rows_are_est, a.step_out + 2 * (size_t)step, a.count_out + 3 * (size_t)step,
               a.match_out + e0, nullptr);
}

static size_t gospa_work_bytes(int32_t n_steps) {      // the two offset arrays
    return n_steps == 0 ? 0 : (2 * ((size_t)n_steps + 1) * sizeof(int32_t) + 255) / 256 * 256;
}

static const char* gospa_bad_offsets(const int32_t* off, int32_t n_steps) {
    if (off[0] != 0) return "do not start at 0";
    for (int32_t s = 0; s < n_steps; ++s)
        if (off[s + 1] < off[s]) return "decrease";
    return nullptr;
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_gospa_work_bytes(int32_t n_steps, int32_t n_est_total, int32_t n_tru_total) {
    if (n_steps < 0 || n_est_total < 0 || n_tru_total < 0) return 0;
    return gospa_work_bytes(n_steps);
}

extern "C" int mht_gospa_steps(mht_ctx* ctx, int32_t n_steps, const int32_t* est_off, const double* est_xy, const int32_t* tru_off, const double* tru_xy,
                               double c, int32_t p, double* step_out, int32_t* count_out, int32_t* match_out, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx, "mht_gospa_steps: null context");
    MHT_REQUIRE(n_steps >= 0, "mht_gospa_steps: negative number of steps (%d)", n_steps);
    if (n_steps == 0) return MHT_OK;
    MHT_REQUIRE(est_off && tru_off && step_out && count_out && work, "mht_gospa_steps: null array");
    const char* bad = gospa_bad_offsets(est_off, n_steps);
    MHT_REQUIRE(!bad, "mht_gospa_steps: the estimates' offsets %s", bad);
    bad = gospa_bad_offsets(tru_off, n_steps);
    MHT_REQUIRE(!bad, "mht_gospa_steps: the truths' offsets %s", bad);
    const int32_t n_est = est_off[n_steps], n_tru = tru_off[n_steps];
    MHT_REQUIRE((est_xy && match_out) || n_est == 0, "mht_gospa_steps: %d estimates and a null array", n_est);
    MHT_REQUIRE(tru_xy || n_tru == 0, "mht_gospa_steps: %d truths and a null array", n_tru);
    MHT_REQUIRE(p == 1 || p == 2, "mht_gospa_steps: p must be 1 or 2 (got %d)", p);
    double cp = 0.0, lim = 0.0;
    MHT_REQUIRE(gospa_cutoff(c, p, &cp, &lim), "mht_gospa_steps: the cut-off c (%g) and c^p must be finite and positive", c);
    MHT_REQUIRE(work_bytes >= gospa_work_bytes(n_steps), "mht_gospa_steps: the workspace has %zu bytes, %zu are needed (mht_gospa_work_bytes)", work_bytes,
                gospa_work_bytes(n_steps));
    int32_t max_rows = 0, max_cols = 0;
    for (int32_t s = 0; s < n_steps; ++s) {
        const int32_t n = est_off[s + 1] - est_off[s], m = tru_off[s + 1] - tru_off[s];
        if (n > GOSPA_MAX_SET || m > GOSPA_MAX_SET) {
            set_error("mht_gospa_steps: step %d has %d estimates and %d truths, at most %d a side fit", s, n, m, GOSPA_MAX_SET);
            return MHT_E_CAPACITY;
        }
        max_rows = n < m ? (n > max_rows ? n : max_rows) : (m > max_rows ? m : max_rows);
        max_cols = n < m ? (m > max_cols ? m : max_cols) : (n > max_cols ? n : max_cols);
    }
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    GospaArgs a = {};
    a.est_off = static_cast<const int32_t*>(work);
    a.tru_off = a.est_off + (n_steps + 1);
    a.est_xy = est_xy; a.tru_xy = tru_xy;
    a.cp = cp; a.lim = lim;
    a.p = p; a.max_rows = max_rows; a.max_cols = max_cols;
    a.step_out = step_out; a.count_out = count_out; a.match_out = match_out;
    const size_t off_bytes = ((size_t)n_steps + 1) * sizeof(int32_t);
    MHT_HIP_CHECK(hipMemcpyAsync(work, est_off, off_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipError_t e = hipMemcpyAsync(static_cast<char*>(work) + off_bytes, tru_off, off_bytes, hipMemcpyHostToDevice, ctx->stream);
    int rc = MHT_OK;
    if (e != hipSuccess) {
        set_error("mht_gospa_steps: copying the offsets failed: %s", hipGetErrorString(e));
        rc = MHT_E_HIP;
    } else {
        rc = launch_kernel(ctx, K_GOSPA, gospa_kernel, dim3(n_steps), dim3(64), gospa_table_bytes(max_rows, max_cols), false, a);
    }
    if (rc != MHT_OK) {      // (the copies read the caller's arrays: they are waited for before the error goes back)
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
