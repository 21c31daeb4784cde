// mht_smooth_tracks, mht_smooth_tracks_ct, mht_smooth_tracks_ais: fixed-interval Rauch-Tung-Striebel smoothing of a batch of track histories
// (include/mht_amd.h).  One walk (smooth_walk, mht_smooth_walk.h) with a step policy per model, one kernel per model and one host path
// (mht_smooth_seam.h, shared with every other seam over track histories);
// the arithmetic is mht_smooth_math.h, mht_smooth_ct_math.h and mht_smooth_ais_math.h.
//
// mht_smooth_tracks: what the reference does per track with pykalman at the end of a run (Target.getSmoothTrack, pyTarget.py:580-609,
// behind every exported <Track>, pyTarget.py:745-802), for ALL tracks of an export in one launch.
//
// Mapping: ONE TRACK PER LANE.  A track is a serial chain of small matrix steps and the tracks are independent, so a lane walks its track
// forward (filter) and then backward (smoother) with every matrix in registers, and everything the lanes touch in memory is laid out
// track-minor -- [node][element][track] -- so that one load or store instruction of a wavefront covers 64 consecutive doubles.  The forward
// pass leaves the filtered mean and covariance (packed symmetric) of every node in the caller's workspace; the backward pass reads them
// back (each lane its own column: no synchronisation) and recomputes the prediction from them, which costs one 6 x 6 x 6 product less than it
// sounds because G needs A Pf anyway.  Tracks have different lengths: a lane stops at its own, so a wavefront runs as long as its longest
// track and shorter lanes idle -- callers that care put tracks of similar length next to each other (pymht_amd.smoothing sorts by length);
// no lane reads or writes anything of another -- no LDS, no atomic, no barrier -- so the result of a track does not depend on where in the
// batch it sits.
// Registers: one wavefront per workgroup and __launch_bounds__(64) give a lane the whole 512-entry file; the six-state covariance
// kernel needs most of a backward step's matrices live at once (Pf, A Pf, U, G, Ps - Pp) and must not spill (tests/test_smooth_resources.py).
// A batch is a few dozen wavefronts, far fewer than the device has SIMDs: occupancy is not what bounds it, the chain's latency is.
//
// mht_smooth_tracks_ct: the constant-turn model, whose transition A_k = Phi(T, w) is rebuilt per lane and per node from the filtered turn
// rate (mht_smooth_ct_math.h).  The backward pass RECOMPUTES sin / cos from the xf_k[4] it reads back anyway instead of keeping sw, cw,
// c, s in the workspace: the same function of the same bits gives the A_k the forward pass predicted with, the workspace stays that of
// the linear six-state smoother (27 doubles a node, not 31, and four loads fewer on the chain), and float64 sin / cos cost about 30
// registers and no scratch, which the kernel has to spare because A_k is four numbers and not a matrix
// (tests/test_smooth_ct_resources.py).  What the recomputation costs in time is measured by tools/smooth_cost.py --ct
// (profiles/smooth_ct_cost.txt).
//
// mht_smooth_tracks_ais: AIS-aided histories with the model the forest filtered them with, four states, opt-in: nothing routes here
// unless the caller asks (ais=True in the Python API).  What a node is comes from two bytes a lane reads per node: has_z (a radar
// update, as in mht_smooth_tracks) and kind (>= 2: the node took an AIS message and steps over two legs instead of one period).  Lanes
// of a wavefront disagree about it, so a wavefront with AIS nodes in some lanes runs both paths; the plain path is the linear kernel's,
// call for call.
// The legs' matrices are NOT wave-uniform: (dT1, dT2) belongs to the message.  They come from a small table of one entry per distinct
// (dT1, dT2) of the batch, 52 doubles each, which a lane indexes with leg[node][track]: a GATHER, the one access here that does not
// coalesce.  That is accepted: messages are made at a few instants inside a radar period, so the table is a handful of entries (a few
// hundred bytes to a few KiB) that stay in cache, neighbouring lanes mostly point at the same entry, and an entry is read once per leg
// and pass -- against a step's several hundred dependent float64 operations.  tools/smooth_cost.py --ais measures what it costs.
//
// Workspace: the lengths, then the filtered slots of every node, [node][slot][element][track].  One slot, the filtered state at the
// scan's time, for the linear and the constant-turn model; two for the AIS model: slot 1 is the filtered state at the message's time,
// written for AIS nodes only.
//
// mht_smooth_tracks_em, the linear model with Q and R learned per track first, is a translation unit of its own: mht_smooth_em.hip.
#include "mht_common.h"
#include "mht_smooth_seam.h"

namespace mht {

template <int N, bool COV>
__global__ void __launch_bounds__(64) smooth_rts_kernel(const SmoothArgs<N, LinearSteps<N>> a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < a.n) smooth_walk<N, COV>(a, t);
}

template <bool COV>
__global__ void __launch_bounds__(64) smooth_rts_ct_kernel(const SmoothArgs<6, ConstantTurnSteps> a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < a.n) smooth_walk<6, COV>(a, t);
}

template <bool COV>
__global__ void __launch_bounds__(64) smooth_ais_kernel(const SmoothArgs<4, AisSteps> a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < a.n) smooth_walk<4, COV>(a, t);
}

// An empty batch is done; any other is checked, then the lengths go to the workspace; then one launch (with_cov, or means_only without
// Ps) and a wait
template <int N, typename Steps>
static int run_smooth(mht_ctx* ctx, const char* seam, const char* sizer, const Steps& steps, bool extras, const SmoothBatch& b,
                      void (*with_cov)(SmoothArgs<N, Steps>), void (*means_only)(SmoothArgs<N, Steps>)) {
    if (b.n == 0) return MHT_OK;
    const int rc = check_batch(seam, b, extras && b.xs, smooth_work_bytes(N, Steps::SLOTS, b.n, b.L_max), sizer, MHT_E_CAPACITY);
    if (rc != MHT_OK) return rc;
    SmoothArgs<N, Steps> a;
    smooth_args<N>(steps, b, a);
    return run_over_lengths(ctx, seam, b, nullptr, 0,
                            [&] { return launch_kernel(ctx, K_SMOOTH_SCORE, b.Ps ? with_cov : means_only, dim3((b.n + 63) / 64), dim3(64), 0, false, a); });
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_smooth_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max) {
    if ((nx != 4 && nx != 6) || n_tracks < 0 || L_max < 0) return 0;
    return smooth_work_bytes(nx, 1, n_tracks, L_max);
}

extern "C" int mht_smooth_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                 const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* xs, double* Ps,
                                 void* work, size_t work_bytes) {
    const char *seam = "mht_smooth_tracks", *sizer = "mht_smooth_work_bytes";
    const int rc = check_linear(seam, ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const SmoothBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, xs, Ps};
    return model->nx == 4 ? run_smooth<4>(ctx, seam, sizer, linear_steps<4>(model), true, b, smooth_rts_kernel<4, true>, smooth_rts_kernel<4, false>)
                          : run_smooth<6>(ctx, seam, sizer, linear_steps<6>(model), true, b, smooth_rts_kernel<6, true>, smooth_rts_kernel<6, false>);
}

extern "C" size_t mht_smooth_ct_work_bytes(int32_t n_tracks, int32_t L_max) {
    if (n_tracks < 0 || L_max < 0) return 0;
    return smooth_work_bytes(6, 1, n_tracks, L_max);
}

extern "C" int mht_smooth_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                    const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* xs, double* Ps,
                                    void* work, size_t work_bytes) {
    const int rc = check_ct("mht_smooth_tracks_ct", ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const SmoothBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, xs, Ps};
    return run_smooth<6>(ctx, "mht_smooth_tracks_ct", "mht_smooth_ct_work_bytes", ct_steps(model), true, b, smooth_rts_ct_kernel<true>,
                         smooth_rts_ct_kernel<false>);
}

extern "C" size_t mht_smooth_ais_work_bytes(int32_t n_tracks, int32_t L_max) {
    if (n_tracks < 0 || L_max < 0) return 0;
    return smooth_work_bytes(4, AisSteps::SLOTS, n_tracks, L_max);
}

extern "C" int mht_smooth_tracks_ais(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                     const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                                     const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, int32_t n_legs,
                                     double* xs, double* Ps, void* work, size_t work_bytes) {
    const int rc = check_ais("mht_smooth_tracks_ais", ctx, model, n_tracks, L_max, n_legs);
    if (rc != MHT_OK) return rc;
    bool extras;
    const AisSteps steps = ais_steps(model, kind, ais_z, ais_r, leg, legs, n_legs, &extras);
    const SmoothBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, xs, Ps};
    return run_smooth<4>(ctx, "mht_smooth_tracks_ais", "mht_smooth_ais_work_bytes", steps, extras, b, smooth_ais_kernel<true>, smooth_ais_kernel<false>);
}
