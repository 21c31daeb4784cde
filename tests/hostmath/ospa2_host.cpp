// TEST-ONLY host build of csrc/mht_ospa2.h (and with it csrc/mht_gospa.h): the base distance (ospa2_add, ospa2_close) and the window's
// search and closing formula (ospa2_window) -- the code the kernels of mht_ospa2.hip run -- compiled for the CPU and run one window at
// a time, so that they are checked against tests/ospa2_ref.py without a GPU (tests/test_ospa2_cpu.py).  Membership, the choice of the
// rows (the smaller side) and the matrix layout are made here as the device makes them.
#include <cstdint>
#include <vector>
#include "../../pymht_amd/csrc/mht_ospa2.h"

using namespace mht;

// D of one (track i, truth j) pair over the steps lo .. hi (both must be members, or the result is c)
extern "C" double ospa2_base_host(int32_t n_trk, const double* trk_xy, const uint8_t* trk_on, int32_t i, int32_t n_tru, const double* tru_xy,
                                  const uint8_t* tru_on, int32_t j, int32_t lo, int32_t hi, double c) {
    Ospa2Acc a = {0.0, 0, 0};
    for (int32_t t = lo; t <= hi; ++t) {
        const size_t ti = (size_t)t * n_trk + i, tj = (size_t)t * n_tru + j;
        ospa2_add(a, trk_on[ti] != 0, trk_xy[2 * ti], trk_xy[2 * ti + 1], tru_on[tj] != 0, tru_xy[2 * tj], tru_xy[2 * tj + 1], c);
    }
    return ospa2_close(a, c);
}

// trk_xy [n_steps][n_trk][2], trk_on [n_steps][n_trk], the truths alike; win_out [2], count_out [3], match_out [n_trk], sweeps [1].
// Returns 0, -1 for a bad c, p or window, -3 for a side above GOSPA_MAX_SET (nothing is written).
extern "C" int ospa2_window_host(int32_t n_steps, int32_t n_trk, const double* trk_xy, const uint8_t* trk_on, int32_t n_tru, const double* tru_xy,
                                 const uint8_t* tru_on, int32_t lo, int32_t hi, double c, int32_t p, double* win_out, int32_t* count_out,
                                 int32_t* match_out, int32_t* sweeps) {
    Ospa2Window w;
    double lim;
    if (n_steps < 0 || n_trk < 0 || n_tru < 0 || (p != 1 && p != 2) || !gospa_cutoff(c, p, &w.cp, &lim)) return -1;
    if (lo < 0 || hi >= n_steps || lo > hi) return -1;
    if (n_trk > GOSPA_MAX_SET || n_tru > GOSPA_MAX_SET) return -3;
    std::vector<int32_t> trk_idx, tru_idx;
    for (int32_t i = 0; i < n_trk; ++i) {
        const bool mem = ospa2_member(trk_on, n_trk, i, lo, hi);
        match_out[i] = mem ? -1 : -2;
        if (mem) trk_idx.push_back(i);
    }
    for (int32_t j = 0; j < n_tru; ++j)
        if (ospa2_member(tru_on, n_tru, j, lo, hi)) tru_idx.push_back(j);
    const int32_t n_w = (int32_t)trk_idx.size(), m_w = (int32_t)tru_idx.size();
    w.rows_are_trk = n_w <= m_w;
    w.n_rows = w.rows_are_trk ? n_w : m_w;
    w.n_cols = w.rows_are_trk ? m_w : n_w;
    w.row_idx = w.rows_are_trk ? trk_idx.data() : tru_idx.data();
    w.col_idx = w.rows_are_trk ? tru_idx.data() : trk_idx.data();
    w.p = p;
    w.c = c;
    std::vector<double> D((size_t)w.n_rows * w.n_cols + 1);
    for (int32_t r = 0; r < w.n_rows; ++r)
        for (int32_t k = 0; k < w.n_cols; ++k) {
            const int32_t i = w.rows_are_trk ? w.row_idx[r] : w.col_idx[k], j = w.rows_are_trk ? w.col_idx[k] : w.row_idx[r];
            D[(size_t)r * w.n_cols + k] = ospa2_base_host(n_trk, trk_xy, trk_on, i, n_tru, tru_xy, tru_on, j, lo, hi, c);
        }
    w.D = D.data();
    std::vector<double> lds(gospa_table_bytes(w.n_rows, w.n_cols) / 8 + 2);
    ospa2_window(w, gospa_carve(reinterpret_cast<char*>(lds.data()), w.n_rows, w.n_cols), win_out, count_out, match_out, sweeps);
    return 0;
}
