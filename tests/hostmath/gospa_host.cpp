// TEST-ONLY host build of csrc/mht_gospa.h: gospa_step itself -- the code the wavefront of gospa_kernel (mht_gospa.hip) runs for its
// step, with the 64 lanes of a sweep as a loop -- compiled for the CPU and run one step at a time, so that the search, its bounds and
// its outputs are checked against tests/gospa_ref.py without a GPU (tests/test_gospa_cpu.py).  The seam's own choice of the rows (the
// smaller side) and of the cut-off figures (gospa_cutoff) is made here as mht_gospa_steps makes it.
#include <cstdint>
#include <vector>
#include "../../pymht_amd/csrc/mht_gospa.h"

using namespace mht;

// est_xy [n][2], tru_xy [m][2]; step_out [2], count_out [3], match_out [n], sweeps [1]: the column sweeps the search made.
// Returns 0, -1 for a bad c or p, -3 for a set above GOSPA_MAX_SET (nothing is written).
extern "C" int gospa_step_host(int32_t n, const double* est_xy, int32_t m, const double* tru_xy, double c, int32_t p, double* step_out,
                               int32_t* count_out, int32_t* match_out, int32_t* sweeps) {
    GospaStep s;
    if (n < 0 || m < 0 || (p != 1 && p != 2) || !gospa_cutoff(c, p, &s.cp, &s.lim)) return -1;
    if (n > GOSPA_MAX_SET || m > GOSPA_MAX_SET) return -3;
    const bool rows_are_est = n <= m;
    s.row_xy = rows_are_est ? est_xy : tru_xy;
    s.col_xy = rows_are_est ? tru_xy : est_xy;
    s.n_rows = rows_are_est ? n : m;
    s.n_cols = rows_are_est ? m : n;
    s.p = p;
    std::vector<double> lds(gospa_table_bytes(s.n_rows, s.n_cols) / 8 + 2);
    gospa_step(s, gospa_carve(reinterpret_cast<char*>(lds.data()), s.n_rows, s.n_cols), rows_are_est, step_out, count_out, match_out, sweeps);
    return 0;
}

extern "C" uint64_t gospa_table_bytes_host(int32_t rows, int32_t cols) { return gospa_table_bytes(rows, cols); }
