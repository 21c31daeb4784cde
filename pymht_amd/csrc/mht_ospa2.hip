// mht_ospa2_windows (include/mht_amd.h): OSPA(2) of a batch of windows -- per window one distance between the set of tracks and the set
// of truth trajectories whose base distance is the time-averaged cut-off distance of a (track, trajectory) pair over the window
// (mht_ospa2.h).  Three launches per batch, all on the context's stream:
//   ospa2_members_kernel   one wavefront per (window, side): who is present in the window, compacted in index order (ballot + popcount),
//                          the member counts, and match_out's -1 / -2
//   ospa2_base_kernel      THE HOT PATH, O(windows x tracks x truths x window length): the matrix of base distances of the members,
//                          [row = smaller side][column = larger side].  One thread per column, OSPA2_ROWS rows per thread: a column's
//                          position (one coalesced 16-byte load per step) serves all of them, the rows' own positions are the same for
//                          the whole wavefront.  Accumulators in registers, no LDS, no scratch (tests/test_ospa2_resources.py).
//   ospa2_assign_kernel    one window per workgroup of one wavefront: the search of mht_gospa.h on the window's matrix, the tables in
//                          dynamic LDS (K_OSPA2), then the closing formula and the matches
// The member counts are known on the device only, so the grid and the tables are sized by what the batch can hold at most: min(n_trk,
// n_tru) rows, max(n_trk, n_tru) columns; workgroups past a window's own counts leave at once.  A window's outputs do not depend on
// its place in the batch.
#include "mht_common.h"
#include "mht_ospa2.h"

namespace mht {

constexpr int OSPA2_ROWS = 8;             // rows a thread of ospa2_base_kernel carries
constexpr int OSPA2_SUB = 32768;          // windows per launch (a grid dimension holds 2^31 / 64 workgroups of 64 threads at 32 column tiles)

struct Ospa2Args {
    const double* trk_xy;       // dev [n_steps][n_trk][2]
    const uint8_t* trk_on;      // dev [n_steps][n_trk]
    const double* tru_xy;
    const uint8_t* tru_on;
    int32_t n_trk, n_tru;
    const int32_t* win_lo;      // dev [n_win]
    const int32_t* win_hi;
    int32_t* cnt;               // dev [n_win][2]: n_w, m_w
    int32_t* trk_idx;           // dev [n_win][n_trk]: the member tracks of the window, ascending
    int32_t* tru_idx;           // dev [n_win][n_tru]
    double* D;                  // dev [n_win][n_trk * n_tru]: the window's matrix at the start of its slot
    double c, cp;
    int32_t p, max_rows, max_cols;
    double* win_out;
    int32_t* count_out;
    int32_t* match_out;
};

__global__ void __launch_bounds__(64) ospa2_members_kernel(const Ospa2Args a, const int w0) {
    const int w = w0 + (int)blockIdx.x;
    const bool tru = blockIdx.y != 0;
    const int n = tru ? a.n_tru : a.n_trk;
    const uint8_t* on = tru ? a.tru_on : a.trk_on;
    int32_t* idx = tru ? a.tru_idx + (size_t)w * a.n_tru : a.trk_idx + (size_t)w * a.n_trk;
    const int lo = a.win_lo[w], hi = a.win_hi[w];
    const int lane = (int)threadIdx.x;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool mem = i < n && ospa2_member(on, n, i, lo, hi);
        const unsigned long long mask = __ballot(mem);
        if (mem) idx[base + __popcll(mask & ((1ull << lane) - 1ull))] = i;
        if (!tru && i < n) a.match_out[(size_t)w * n + i] = mem ? -1 : -2;
        base += __popcll(mask);
    }
    if (lane == 0) a.cnt[2 * (size_t)w + (tru ? 1 : 0)] = base;
}

__global__ void __launch_bounds__(64) ospa2_base_kernel(const Ospa2Args a, const int w0, const int col_tiles) {
    const int w = w0 + (int)blockIdx.x / col_tiles, ct = (int)blockIdx.x % col_tiles;
    const int n_w = a.cnt[2 * (size_t)w], m_w = a.cnt[2 * (size_t)w + 1];
    const bool rows_are_trk = n_w <= m_w;      // the smaller side are the rows
    const int nr = rows_are_trk ? n_w : m_w, nc = rows_are_trk ? m_w : n_w;
    const int r0 = (int)blockIdx.y * OSPA2_ROWS, j = ct * 64 + (int)threadIdx.x;
    if (r0 >= nr || ct * 64 >= nc) return;
    const int r_n = rows_are_trk ? a.n_trk : a.n_tru, c_n = rows_are_trk ? a.n_tru : a.n_trk;
    const double2* r_xy = reinterpret_cast<const double2*>(rows_are_trk ? a.trk_xy : a.tru_xy);
    const double2* c_xy = reinterpret_cast<const double2*>(rows_are_trk ? a.tru_xy : a.trk_xy);
    const uint8_t* r_on = rows_are_trk ? a.trk_on : a.tru_on;
    const uint8_t* c_on = rows_are_trk ? a.tru_on : a.trk_on;
    const int32_t* r_idx = rows_are_trk ? a.trk_idx + (size_t)w * a.n_trk : a.tru_idx + (size_t)w * a.n_tru;
    const int32_t* c_idx = rows_are_trk ? a.tru_idx + (size_t)w * a.n_tru : a.trk_idx + (size_t)w * a.n_trk;
    const bool live = j < nc;
    const int cj = c_idx[live ? j : nc - 1];      // (a lane past the last column computes that column again and stores nothing)
    int ri[OSPA2_ROWS];
    Ospa2Acc acc[OSPA2_ROWS];
#pragma unroll
    for (int k = 0; k < OSPA2_ROWS; ++k) {
        ri[k] = r_idx[r0 + k < nr ? r0 + k : nr - 1];
        acc[k].sum = 0.0;
        acc[k].n_near = 0;
        acc[k].n_any = 0;
    }
    const int lo = a.win_lo[w], hi = a.win_hi[w];
    for (int t = lo; t <= hi; ++t) {
        const double2 cpos = c_xy[(size_t)t * c_n + cj];
        const bool c_here = c_on[(size_t)t * c_n + cj] != 0;
#pragma unroll
        for (int k = 0; k < OSPA2_ROWS; ++k) {
            const double2 rp = r_xy[(size_t)t * r_n + ri[k]];
            ospa2_add(acc[k], r_on[(size_t)t * r_n + ri[k]] != 0, rp.x, rp.y, c_here, cpos.x, cpos.y, a.c);
        }
    }
    if (!live) return;
    double* D = a.D + (size_t)w * a.n_trk * a.n_tru;
#pragma unroll
    for (int k = 0; k < OSPA2_ROWS; ++k)
        if (r0 + k < nr) D[(size_t)(r0 + k) * nc + j] = ospa2_close(acc[k], a.c);
}

__global__ void __launch_bounds__(64) ospa2_assign_kernel(const Ospa2Args a, const int w0) {
    extern __shared__ __attribute__((aligned(16))) char ospa2_lds[];
    const int w = w0 + (int)blockIdx.x;
    const int n_w = a.cnt[2 * (size_t)w], m_w = a.cnt[2 * (size_t)w + 1];
    Ospa2Window win;
    win.rows_are_trk = n_w <= m_w;
    win.n_rows = win.rows_are_trk ? n_w : m_w;
    win.n_cols = win.rows_are_trk ? m_w : n_w;
    win.D = a.D + (size_t)w * a.n_trk * a.n_tru;
    const int32_t* trk_idx = a.trk_idx + (size_t)w * a.n_trk;
    const int32_t* tru_idx = a.tru_idx + (size_t)w * a.n_tru;
    win.row_idx = win.rows_are_trk ? trk_idx : tru_idx;
    win.col_idx = win.rows_are_trk ? tru_idx : trk_idx;
    win.p = a.p;
    win.c = a.c;
    win.cp = a.cp;
    ospa2_window(win, gospa_carve(ospa2_lds, a.max_rows, a.max_cols), a.win_out + 2 * (size_t)w, a.count_out + 3 * (size_t)w,
                 a.match_out + (size_t)w * a.n_trk, nullptr);
}

static size_t ospa2_round256(size_t b) { return (b + 255) / 256 * 256; }

// The workspace: lo and hi, the member counts, the two index lists, the matrices
struct Ospa2Layout {
    size_t win, cnt, trk_idx, tru_idx, D, total;
};
static Ospa2Layout ospa2_layout(int32_t n_trk, int32_t n_tru, int32_t n_win) {
    Ospa2Layout l;
    const size_t w = (size_t)n_win;
    l.win = 0;
    l.cnt = l.win + ospa2_round256(2 * w * sizeof(int32_t));
    l.trk_idx = l.cnt + ospa2_round256(2 * w * sizeof(int32_t));
    l.tru_idx = l.trk_idx + ospa2_round256(w * (size_t)n_trk * sizeof(int32_t));
    l.D = l.tru_idx + ospa2_round256(w * (size_t)n_tru * sizeof(int32_t));
    l.total = l.D + ospa2_round256(w * (size_t)n_trk * (size_t)n_tru * sizeof(double));
    return l;
}

// the seam's stage timing (tools/ospa2_cost.py): off unless switched on, per process
static bool ospa2_timing = false;
static float ospa2_ms[3] = {0.f, 0.f, 0.f};

}  // namespace mht

using namespace mht;

extern "C" size_t mht_ospa2_work_bytes(int32_t n_trk, int32_t n_tru, int32_t n_steps, int32_t n_win) {
    if (n_trk < 0 || n_tru < 0 || n_steps < 0 || n_win < 0 || n_trk > GOSPA_MAX_SET || n_tru > GOSPA_MAX_SET) return 0;
    if (n_win == 0 || n_steps == 0) return 0;
    return ospa2_layout(n_trk, n_tru, n_win).total;
}

extern "C" void mht_ospa2_set_timing(int32_t on) { ospa2_timing = on != 0; }
extern "C" void mht_ospa2_stage_times(float* ms) {
    for (int k = 0; k < 3; ++k) ms[k] = ospa2_ms[k];
}

extern "C" int mht_ospa2_windows(mht_ctx* ctx, int32_t n_steps, int32_t n_trk, const double* trk_xy, const uint8_t* trk_on, int32_t n_tru,
                                 const double* tru_xy, const uint8_t* tru_on, int32_t n_win, const int32_t* win_lo, const int32_t* win_hi, double c,
                                 int32_t p, double* win_out, int32_t* count_out, int32_t* match_out, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx, "mht_ospa2_windows: null context");
    MHT_REQUIRE(n_steps >= 0 && n_trk >= 0 && n_tru >= 0 && n_win >= 0, "mht_ospa2_windows: negative count (%d steps, %d tracks, %d truths, %d windows)",
                n_steps, n_trk, n_tru, n_win);
    if (n_win == 0 || n_steps == 0) return MHT_OK;
    MHT_REQUIRE(win_lo && win_hi && win_out && count_out && work, "mht_ospa2_windows: null array");
    MHT_REQUIRE((trk_xy && trk_on && match_out) || n_trk == 0, "mht_ospa2_windows: %d tracks and a null array", n_trk);
    MHT_REQUIRE((tru_xy && tru_on) || n_tru == 0, "mht_ospa2_windows: %d truths and a null array", n_tru);
    MHT_REQUIRE(((uintptr_t)trk_xy | (uintptr_t)tru_xy) % 16 == 0, "mht_ospa2_windows: the positions must be aligned to 16 bytes");
    MHT_REQUIRE(p == 1 || p == 2, "mht_ospa2_windows: p must be 1 or 2 (got %d)", p);
    double cp = 0.0, lim = 0.0;
    MHT_REQUIRE(gospa_cutoff(c, p, &cp, &lim), "mht_ospa2_windows: the cut-off c (%g) and c^p must be finite and positive", c);
    for (int32_t w = 0; w < n_win; ++w)
        MHT_REQUIRE(win_lo[w] >= 0 && win_hi[w] < n_steps && win_lo[w] <= win_hi[w], "mht_ospa2_windows: window %d is [%d, %d], the run has steps 0 .. %d", w,
                    win_lo[w], win_hi[w], n_steps - 1);
    if (n_trk > GOSPA_MAX_SET || n_tru > GOSPA_MAX_SET) {
        set_error("mht_ospa2_windows: %d tracks and %d truths, at most %d a side fit", n_trk, n_tru, GOSPA_MAX_SET);
        return MHT_E_CAPACITY;
    }
    const Ospa2Layout l = ospa2_layout(n_trk, n_tru, n_win);
    MHT_REQUIRE(work_bytes >= l.total, "mht_ospa2_windows: the workspace has %zu bytes, %zu are needed (mht_ospa2_work_bytes)", work_bytes, l.total);
    MHT_REQUIRE((uintptr_t)work % 16 == 0, "mht_ospa2_windows: the workspace must be aligned to 16 bytes");
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    char* base = static_cast<char*>(work);
    Ospa2Args a = {};
    a.trk_xy = trk_xy; a.trk_on = trk_on; a.tru_xy = tru_xy; a.tru_on = tru_on;
    a.n_trk = n_trk; a.n_tru = n_tru;
    a.win_lo = reinterpret_cast<const int32_t*>(base + l.win);
    a.win_hi = a.win_lo + n_win;
    a.cnt = reinterpret_cast<int32_t*>(base + l.cnt);
    a.trk_idx = reinterpret_cast<int32_t*>(base + l.trk_idx);
    a.tru_idx = reinterpret_cast<int32_t*>(base + l.tru_idx);
    a.D = reinterpret_cast<double*>(base + l.D);
    a.c = c; a.cp = cp; a.p = p;
    a.max_rows = n_trk < n_tru ? n_trk : n_tru;      // (no window can have more: the counts themselves stay on the device)
    a.max_cols = n_trk < n_tru ? n_tru : n_trk;
    a.win_out = win_out; a.count_out = count_out; a.match_out = match_out;
    const int col_tiles = (a.max_cols + 63) / 64, row_tiles = (a.max_rows + OSPA2_ROWS - 1) / OSPA2_ROWS;
    const size_t win_bytes = (size_t)n_win * sizeof(int32_t);
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    const bool timed = ospa2_timing && n_win <= OSPA2_SUB;
    if (timed)
        for (int k = 0; k < 4; ++k) MHT_HIP_CHECK(hipEventCreate(&ev[k]));
    int rc = MHT_OK;
    hipError_t e = hipMemcpyAsync(base + l.win, win_lo, win_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(base + l.win + win_bytes, win_hi, win_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        set_error("mht_ospa2_windows: copying the windows failed: %s", hipGetErrorString(e));
        rc = MHT_E_HIP;
    }
    for (int32_t w0 = 0; w0 < n_win && rc == MHT_OK; w0 += OSPA2_SUB) {
        const int n_sub = n_win - w0 < OSPA2_SUB ? n_win - w0 : OSPA2_SUB;
        if (timed) (void)hipEventRecord(ev[0], ctx->stream);
        rc = launch_kernel(ctx, K_OSPA2, ospa2_members_kernel, dim3(n_sub, 2), dim3(64), 0, false, a, w0);
        if (timed) (void)hipEventRecord(ev[1], ctx->stream);
        if (rc == MHT_OK && row_tiles > 0)
            rc = launch_kernel(ctx, K_OSPA2, ospa2_base_kernel, dim3((unsigned)n_sub * col_tiles, row_tiles), dim3(64), 0, false, a, w0, col_tiles);
        if (timed) (void)hipEventRecord(ev[2], ctx->stream);
        if (rc == MHT_OK)
            rc = launch_kernel(ctx, K_OSPA2, ospa2_assign_kernel, dim3(n_sub), dim3(64), gospa_table_bytes(a.max_rows, a.max_cols), false, a, w0);
        if (timed) (void)hipEventRecord(ev[3], ctx->stream);
    }
    if (rc != MHT_OK) {      // (the copies read the caller's arrays: they are waited for before the error goes back)
        (void)hipStreamSynchronize(ctx->stream);
    } else {
        e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            set_error("mht_ospa2_windows: hipStreamSynchronize failed: %s", hipGetErrorString(e));
            rc = MHT_E_HIP;
        }
    }
    if (timed) {
        if (rc == MHT_OK)
            for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&ospa2_ms[k], ev[k], ev[k + 1]);
        for (int k = 0; k < 4; ++k) (void)hipEventDestroy(ev[k]);
    }
    return rc;
}
