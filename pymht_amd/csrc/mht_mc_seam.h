// INTERNAL: what the Monte-Carlo seams share across translation units.  mht_mc.hip holds the factor and the fold kernels, the layout of
// a call's work buffer and the checks every seam makes, and DEFINES what is declared here; mht_mc_zone.hip and mht_mc_domain.hip launch through these
// declarations, so the kernels of mht_mc.hip stay in their unit (tests/test_mc_resources.py pins that unit's nine kernels).  The two
// device helpers every walk kernel starts with are here as inline code.
#pragma once
#include <vector>
#include "mht_common.h"
#include "mht_mc.h"

namespace mht {

constexpr int MC_MAX_BLOCKS = 2048;
constexpr int MC_WAVES = MC_THREADS / 64;
constexpr int MC_ROW = MC_MAX_STEPS + 1;            // words of a row of steps in LDS, whatever K is

struct McFoldArgs {
    int32_t items, words, chunks, S;
    const uint32_t* part;        // [chunks][words][items]
    const int32_t* istatus;      // [items]
    uint32_t *out0, *out1, *out2;      // words 0 .. end0 - 1, end0 .. end1 - 1 and end1 .. words - 1, each [..][items]
    int32_t end0, end1;
    uint32_t* valid;             // [items]
    int32_t* status;             // [items]
};

// The work buffer of a call over `items` targets or pairs of `words` words each
struct McLayout {
    size_t Lw, part, cstatus, istatus, bytes;      // offsets in bytes, and their total
    McSplit split;
};

McLayout mc_layout(int32_t nx, int32_t nComp, int32_t items, int32_t words, int32_t S);
bool mc_sizes_fit(int32_t nx, int32_t nComp, int32_t T, int32_t K, int32_t S);
// The factor launch of the build's N = nx (4 or 6, checked by the seam)
int mc_launch_factor(mht_ctx* ctx, int32_t nx, int32_t nComp, const double* x, const double* P, const double* cdf, double* Lw, int32_t* cstatus);
int mc_launch_fold(mht_ctx* ctx, const McFoldArgs& ga);
int mc_seam_checks(const char* who, mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t steps, int32_t particles, double dt,
                   double radius, const double* Phi, const double* Q, const int32_t* first, const int32_t* also, size_t n, std::vector<int32_t>& alsoHost);

#ifdef __HIPCC__
// The by-value arguments of a walk kernel into the workgroup's LDS, dword-wise (why: the head of mht_mc.hip)
template <class Args>
__device__ void mc_stage(Args& s, const Args& a, int tid) {
    static_assert(sizeof(Args) % 4 == 0, "the arguments are copied dword-wise");
    for (int i = tid; i < (int)(sizeof(Args) / 4); i += MC_THREADS) reinterpret_cast<uint32_t*>(&s)[i] = reinterpret_cast<const uint32_t*>(&a)[i];
}

// A lane's share of the status of target t's components (mc_target_status, strided over the workgroup); the caller ORs over the lanes
__device__ inline void mc_target_flags(const int32_t* first, const int32_t* cstatus, int t, int tid, int& nan, int& indefinite) {
    for (int c = first[t] + tid; c < first[t + 1]; c += MC_THREADS) {
        const int st = cstatus[c];
        nan |= st == 1;
        indefinite |= st == 2;
    }
}
#endif

}  // namespace mht
