/* mht_amd.h -- C ABI of libmht_amd.so: the MI355X (gfx950) implementation of pyMHT's per-scan hot path.
 *
 * The reference (erikliland/pyMHT) has NO native/FFI boundary: the path sits behind Python methods of
 * pymht/tracker.py.  The entry points below are what a ctypes binding on the reference side would call in
 * place of those methods (INTEGRATION.md shows the stub); each one cites the reference code it replaces
 * (file:line relative to the reference root).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / HIP types in the signatures.  `stream` arguments are
 *     a hipStream_t passed as void* (NULL = the default stream).
 *   - "dev" pointers are device (HBM) pointers, e.g. torch.Tensor.data_ptr(); "host" pointers are ordinary
 *     host memory.  The caller owns every buffer it passes; the library owns only its ctx and workspace.
 *   - every function returns MHT_OK (0) or a negative MHT_E_* code and never aborts; mht_last_error() gives
 *     the message of the last failure on the calling thread.  (The reference signals failure with `assert`,
 *     e.g. tracker.py:1212; the Python wrapper turns non-zero codes into AssertionError/RuntimeError.)
 *   - one ctx per Tracker, one HIP stream per ctx, calls on a ctx are serialised by the caller (the reference
 *     is single-threaded and non-reentrant); different ctxs may be used from different threads / GPUs.
 */
#ifndef MHT_AMD_H
#define MHT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHT_ABI_VERSION 6

/* State dimension of the library build the header is used with: 4 (libmht_amd.so: the reference's CV model, models/pv.py) or 6
 * (libmht_amd6.so: the same sources compiled with -DMHT_NX=6 for BASELINE config 5's six-state model).  It sizes the model matrices
 * and the state vectors / covariances of the forest's reports; the stateless seams mht_gate_scan (4 states), mht_gate_scan_x and
 * mht_smooth_tracks and mht_smooth_tracks_em (4 or 6 at run time), mht_smooth_tracks_ct (6) and mht_smooth_tracks_ais (4), and the mht_score_tracks*
 * and mht_trace_tracks* seams next to them, do not depend on it. */
#ifndef MHT_NX
#define MHT_NX 4
#endif

enum {
    MHT_OK = 0,
    MHT_E_INVALID = -1,    /* bad argument */
    MHT_E_HIP = -2,        /* a HIP runtime call failed */
    MHT_E_CAPACITY = -3,   /* an output buffer / pool is too small: grow and retry */
    MHT_E_INFEASIBLE = -4, /* 0-1 ILP without a feasible point (cannot happen for MHT trees) */
    MHT_E_LIMIT = -5,      /* branch-and-bound node limit hit: selection returned is feasible, not proven optimal */
    MHT_E_STATE = -6       /* call sequence error */
};

/* node flag bits (mht_nodes.flags) -- dtype bookkeeping of the reference */
#define MHT_F_STATE_F32 1u /* state chain is float32 (targets born from the initiator, m_of_n.py:353-358) */
#define MHT_F_SCORE_F32 2u /* cumulativeNLLR currently holds a float32 value */
#define MHT_F_DEAD 8u      /* forest only: taken out of the tree by similar-state pruning (never set in what mht_forest_leaves returns) */
#define MHT_F_COV_F64 16u  /* forest with MHT_FOREST_AIS only: the node's covariance is float64 -- an AIS-updated node (models/ais.py:4:
                            * ais.C is float64, so P_hat of tracker.py:451-487 is) or a child of a batch NumPy promoted because one of its
                            * members was (np.array of the leaves' P_0, tracker.py:859-870).  Such a node's state is float64 too. */

/* ILP status (mht_solve_blp / forest step) */
#define MHT_BLP_CERTIFIED 1   /* Lagrangian certificate: conflict-free minimisers + complementary slackness */
#define MHT_BLP_BRANCHED 2    /* proven optimal by branch and bound on the GPU */
#define MHT_BLP_NODE_LIMIT 3  /* node limit: best feasible point returned (MHT_E_LIMIT) */

typedef struct mht_ctx mht_ctx;

/* The linear-Gaussian model: what Tracker.__init__ reads off the model module (tracker.py:54-59, pv.py:7-34)
 * plus the two scalars the gate and the score need (tracker.py:107, :110).  Row-major float32. */
typedef struct mht_model {
    float A[MHT_NX * MHT_NX]; /* Phi(radarPeriod) */
    float Q[MHT_NX * MHT_NX]; /* Q(radarPeriod)   */
    float C[2 * MHT_NX];      /* C_RADAR (2 x nx) */
    float R[4];               /* R_RADAR() (2x2)  */
    double eta2;
    double lambda_ex;
    double default_pd;        /* Tracker.default_P_d; nodes whose pd equals it use default_miss_nllr */
    double default_miss_nllr; /* -log(1 - default_pd) evaluated by the host libm (pyTarget.py:326) */
} mht_model;

/* A layer of track hypotheses in HBM, structure of arrays (one hypothesis = one index i < cap).
 * Field meaning follows pyTarget.Target (pyTarget.py:16-40). */
typedef struct mht_nodes {
    double* x;       /* dev [4][cap]  : x[k*cap+i]  state x_0 (holds f32 values when MHT_F_STATE_F32) */
    double* cnllr;   /* dev [cap]     : cumulativeNLLR */
    double* pd;      /* dev [cap]     : P_d */
    int32_t* parent; /* dev [cap]     : index of the parent in the previous layer, -1 for a fresh root */
    int32_t* meas;   /* dev [cap]     : measurementNumber (1-based), 0 = missed detection */
    int32_t* cov;    /* dev [cap]     : column of P holding P_0 of this node */
    uint8_t* flags;  /* dev [cap]     : MHT_F_* */
    float* P;        /* dev [16][cap_cov] : P[e*cap_cov+j], e = 4*row+col.  Children of one parent share
                        two columns: 2*leaf = P_bar (miss child), 2*leaf+1 = P_hat (all hit children),
                        as the reference shares one ndarray between siblings (pyTarget.py:246) */
    int32_t cap, cap_cov;
} mht_nodes;

/* ---- lifetime ------------------------------------------------------------------------------------------- */
int mht_abi_version(void);
const char* mht_last_error(void);
/* device: HIP device ordinal; stream: hipStream_t as void* (NULL = default stream) */
int mht_create(mht_ctx** out, int device, void* stream);
int mht_destroy(mht_ctx* ctx);
int mht_synchronize(mht_ctx* ctx);

/* ---- seam (i): Tracker._processLeafNodes + Target.spawnNewNodes ------------------------------------------
 * Replaces tracker.py:383-398 (-> :861-889 predict/precalc, :804-859 gate/update/score) and the child
 * construction of pyTarget.py:227-258 / :319-328 for ALL leaves of ALL targets in one call.
 *
 * For leaf i (0 <= i < L, node leaf_src[i] of `in`, or node i if leaf_src == NULL) the children are written
 * to `out` at indices child_ptr[i] .. child_ptr[i+1]-1: first the missed-detection child (x_bar, P_bar,
 * cnllr - log(1-pd)), then one child per gated measurement in ascending measurement index (x_hat, P_hat,
 * cnllr + nllr, meas = index+1) -- the order of np.nonzero (tracker.py:832) and of getLeafNodes (pyTarget.py:461).
 *   z          dev (M,2) float32 row-major, the scan (MeasurementList.measurements)
 *   child_ptr  dev [L+1] int32 (output)
 *   nllr       dev [out->cap] double or NULL: per child score increment (kalman.py:14-22 / -log(1-pd))
 *   used       dev [(M+63)/64] uint64 or NULL: bit j set iff some leaf gated measurement j (tracker.py:331);
 *              OR-ed into, the caller zeroes it
 *   n_children host int* or NULL: total number of children (forces a stream synchronisation when non-NULL)
 * Returns MHT_E_CAPACITY (after synchronising) if out->cap / out->cap_cov are too small when n_children is
 * requested; otherwise capacity overflow is reported by the next synchronising call. */
int mht_gate_scan(mht_ctx* ctx, const mht_model* model, const mht_nodes* in, const int32_t* leaf_src, int32_t L,
                  const float* z, int32_t M, const mht_nodes* out, int32_t* child_ptr, double* nllr,
                  uint64_t* used, int32_t* n_children);

/* ---- seam (i), dimension-generic: a linear-Gaussian model with nx states (4 or 6) and 2 measurements -----------------------
 * BASELINE config 5 names a 6-state model; the reference ships none, but its kalman module is dimension-generic:
 * predict / precalc (pymht/utils/kalman.py:55-101), z_tilde / NIS / gate (kalman.py:25-40, tracker.py:829), numpyFilter
 * (kalman.py:43-52), nllr (kalman.py:14-22).  This is that module for L leaves x M measurements in one call, results in the
 * reference's evaluation order.  All arrays are device memory, structure-of-arrays:
 *   x [nx][L] f64, flags [L] (MHT_F_STATE_F32: the leaf's state chain is float32), P [nx*nx][L] f32, pd [L], z (M,2) f32
 *   x_bar [nx][L] f64, P_bar / P_hat [nx*nx][L], S / S_inv [4][L], K [2*nx][L]  (K row-major nx x 2)
 *   row_ptr [L+1], col_idx [cap] (gated measurement indices, ascending per leaf: np.nonzero, tracker.py:832),
 *   x_hat [nx][cap] f64 and nllr [cap] per gated pair.  n_pairs (host, may be NULL) = row_ptr[L].  Synchronises.
 * Returns MHT_E_CAPACITY if there are more gated pairs than cap. */
typedef struct mht_model_x {
    int32_t nx;             /* 4 or 6 */
    const float* A;         /* host [nx*nx] row-major state transition */
    const float* Q;         /* host [nx*nx] process noise */
    const float* C;         /* host [2*nx] measurement matrix */
    const float* R;         /* host [4] measurement noise */
    double eta2, lambda_ex;
    /* transition = 0: the linear model above (A for every leaf: kalman.predict, kalman.py:55-64).
     * transition = 1 (nx = 6 only; BASELINE config 5's constant-turn model, pymht_amd/models/ct.py): state = [x, y, vx, vy, w, a]; every
     * leaf gets its OWN A = Phi(period, w of the leaf) -- velocity rotated by w * period, the arc integrated, w += period * a; A above is
     * ignored -- and runs the reference's per-hypothesis form: kalman.predict_single (kalman.py:67-70), then kalman.precalc on a batch of
     * one (kalman.py:82-101), i.e. the matrix x vector products in BLAS gemv order. */
    int32_t transition;
    double period;
} mht_model_x;
int mht_gate_scan_x(mht_ctx* ctx, const mht_model_x* model, int32_t L, const double* x, const uint8_t* flags, const float* P,
                    const double* pd, const float* z, int32_t M, double* x_bar, float* P_bar, float* P_hat, float* S, float* S_inv,
                    float* K, int32_t* row_ptr, int32_t* col_idx, double* x_hat, double* nllr, int32_t cap, int32_t* n_pairs);


/* ---- seam (ii): Tracker._findClustersFromSets (tracker.py:961-974) -------------------------------------------
 * assoc  dev [T][words] uint64: bit b of row t set iff target t is associated with measurement node b
 *        (the reference's __associatedMeasurements__ sets; a node is a (scan, measurement) of the window)
 * label  dev [T] int32 out: smallest target index of the connected component of t.  Clusters ordered by label
 *        with ascending members are exactly the reference's cluster list. */
int mht_cluster(mht_ctx* ctx, int32_t T, int32_t words, const uint64_t* assoc, int32_t* label);

/* ---- seam (iii): Tracker._solveBLP_OR_TOOLS(A1, A2, f) (tracker.py:1155-1217) ---------------------------------
 * One 0-1 ILP:  min f.tau  s.t.  A1 tau <= 1, A2 tau = 1, tau binary, in the sparse form the tree gives it:
 *   group_ptr dev [nT+1] int32 : columns group_ptr[t] .. group_ptr[t+1]-1 belong to target t (A2, tracker.py:1115)
 *   rows      dev [depth][nHyp] int32 : rows[d*nHyp+h] = d-th measurement row of column h or -1 (A1 by columns)
 *   cost      dev [nHyp] double  (f = getScore()/N, tracker.py:1124-1136)
 *   selected  dev [nT] int32 out : chosen column per target (ascending = the reference's return list)
 *   objective/status/iterations/nodes : host out (status MHT_BLP_*).  Synchronises the stream. */
int mht_solve_blp(mht_ctx* ctx, int32_t nHyp, int32_t nT, int32_t nRows, int32_t depth, const int32_t* group_ptr,
                  const int32_t* rows, const double* cost, int32_t max_iter, int32_t node_limit, int32_t* selected,
                  double* objective, int32_t* status, int32_t* iterations, int32_t* nodes);

/* ---- seam (iv): Tracker._nScanPruning (tracker.py:1229-1231) -> _pruneTargetIndex (:1219-1227) -> Target.pruneDepth
 * (pyTarget.py:343-356) -> _pruneAllHypothesisExceptThis(backtrack=True) (:330-337), for trees the caller owns ---------------
 * The trees of all targets are one array of parent pointers.
 *   parent    dev [n_nodes] int32 : parent node or -1 (top of a tree)
 *   sel       dev [T] int32       : __trackNodes__[t], the selected leaf of target t
 *   window    dev [T] int32       : __targetWindowSize__[t] (N)
 *   new_root  dev [T] int32 out   : the ancestor `window` levels above sel[t] (the top of the tree if it is closer)
 *   keep      dev [n_nodes] uint8 out : 1 iff the node survives (it is a new root, above one, or below one)
 * Asynchronous on the ctx stream. */
int mht_prune(mht_ctx* ctx, int32_t n_nodes, const int32_t* parent, int32_t T, const int32_t* sel, const int32_t* window,
              int32_t* new_root, uint8_t* keep);

/* ---- the seams over a batch of track histories, (v) and (vi) below, share one host path (csrc/mht_smooth_seam.h): the model and the
 * batch are checked on the host before anything is launched, the lengths go to the front of the workspace, one launch (EM: one per
 * walk), a wait.  A workspace that is too small is MHT_E_CAPACITY from mht_smooth_tracks, mht_smooth_tracks_ct and
 * mht_smooth_tracks_ais, and MHT_E_INVALID from every other seam, mht_smooth_tracks_em* included; a launch that fails is waited for
 * before its error goes back, since the copy of the lengths reads the caller's array. */

/* ---- seam (v): Target.getSmoothTrack (pyTarget.py:580-609) for ALL tracks of an export -- Tracker.getSmoothTracks, and the
 * <SmoothedStates> of every <Track> (pyTarget.py:745-802) -- stateless ---------------------------------------------------------
 * A fixed-interval Rauch-Tung-Striebel smoother over a batch of track histories, float64 throughout.  The reference hands each
 * history to pykalman, whose EM step re-estimates the noise covariances and is not reproducible; here the model is the tracker's
 * own (model: nx, A, Q, C, R are read and widened to float64; transition must be 0 -- a state-dependent transition has no linear
 * smoother: MHT_E_INVALID).  Q and R are covariances: their upper triangles are read.
 * Track t (0 <= t < n_tracks) has len[t] nodes, 1 <= len[t] <= L_max; node 0 is its initial state, node k >= 1 carries a radar
 * measurement or none (a missed detection, or a node updated by an AIS message alone):
 *   forward   xf_0 = x_init, Pf_0 = P_init;  xp_k = A xf_{k-1}, Pp_k = A Pf_{k-1} A' + Q;  with a measurement S = C Pp_k C' + R,
 *             K = Pp_k C' S^-1, xf_k = xp_k + K (z_k - C xp_k), Pf_k = Pp_k - K C Pp_k;  without one xf_k = xp_k, Pf_k = Pp_k
 *   backward  xs_{L-1} = xf_{L-1}, Ps_{L-1} = Pf_{L-1};  G = Pf_k A' Pp_{k+1}^-1 (through a Cholesky factor of Pp_{k+1}),
 *             xs_k = xf_k + G (xs_{k+1} - xp_{k+1}),  Ps_k = Pf_k + G (Ps_{k+1} - Pp_{k+1}) G'
 * One track per lane; all device arrays are track-minor so that a wavefront's accesses coalesce:
 *   len      HOST [n_tracks] int32 (checked before anything is launched)
 *   x_init   dev [nx][n_tracks] f64          P_init  dev [nx*nx][n_tracks] f64 (row-major entries; the upper triangle is read)
 *   z        dev [L_max][2][n_tracks] f64    has_z   dev [L_max][n_tracks] uint8, non-zero = node k of the track has a measurement
 *            (row 0 of both is ignored; rows >= len[t] of track t are not read)
 *   xs       dev [L_max][nx][n_tracks] f64 out
 *   Ps       dev [L_max][nx (nx + 1) / 2][n_tracks] f64 out, or NULL (means only): the upper triangle row by row -- (0,0), (0,1), ..
 *            (0,nx-1), (1,1), ..; the result is symmetric by construction.  Rows >= len[t] of track t are left as they were.
 *   work     dev, work_bytes >= mht_smooth_work_bytes(nx, n_tracks, L_max) (the filtered states of every node; 0 for a bad nx or
 *            a negative size): MHT_E_CAPACITY if it is smaller.
 * A wavefront runs as long as the longest of its 64 tracks: put tracks of similar length next to each other.  No track's result
 * depends on its place in the batch or on the other tracks.  Synchronises.  On MHT_E_INVALID / MHT_E_CAPACITY nothing has been written. */
size_t mht_smooth_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max);
int mht_smooth_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                      const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* xs, double* Ps,
                      void* work, size_t work_bytes);

/* ---- seam (v), constant turn: the same smoother for histories of the constant-turn model (pymht_amd/models/ct.py) -- OPT-IN: nothing
 * routes here unless the caller asks (constantTurn=True in the Python API); mht_smooth_tracks keeps rejecting transition != 0 -------
 * The forest's filter predicts such a track with x+ = Phi(T, w) x, P+ = Phi P Phi' + Q, Phi taken at the hypothesis's FILTERED turn
 * rate w = x[4] and without a Jacobian with respect to w (not an EKF).  Along one track that is a linear model with a known A_k per
 * step, and this is the recursion above with A_k = Phi(T, xf_k[4]) in place of A, in the forward pass and -- rebuilt from the same
 * stored xf_k[4] -- in G_k = Pf_k A_k' Pp_{k+1}^-1:
 *   s = sin(w T), c = cos(w T), sw = s / w, cw = (1 - c) / w (|w| < 1e-9: sw = T, cw = 0);  A_k = I + the nine entries
 *   (0,2) sw (0,3) -cw (1,2) cw (1,3) sw (2,2) c (2,3) -s (3,2) s (3,3) c (4,5) T, in float64 and NOT rounded to float32 as the
 *   forest's own Phi is -- a rounded A_k would make the result a discontinuous function of w; the forward pass here therefore differs
 *   from the forest's filtered states by that rounding, of order 1e-7 relative.
 * model: nx == 6 and transition == 1 are required (anything else, transition == 0 included: MHT_E_INVALID); Q, C, R are read and
 * widened, T is `period` (> 0), A is ignored and may be NULL.  Every other argument, every layout and the error behaviour are those of
 * mht_smooth_tracks with nx = 6; work_bytes >= mht_smooth_ct_work_bytes(n_tracks, L_max) = mht_smooth_work_bytes(6, n_tracks, L_max)
 * (sin / cos are recomputed in the backward pass, not stored; 0 for a negative size). */
size_t mht_smooth_ct_work_bytes(int32_t n_tracks, int32_t L_max);
int mht_smooth_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                         const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* xs, double* Ps,
                         void* work, size_t work_bytes);

/* ---- seam (v), AIS: the same smoother for histories of an AIS-aided forest, with the AIS updates the forest applied -- OPT-IN: nothing
 * routes here unless the caller asks (ais=True in the Python API); mht_smooth_tracks smooths such a history as radar-only ------------
 * A node of an AIS-aided track that took a message did not step one radar period (Tracker.__fuseRadarAndAis, csrc/mht_ais_math.h):
 *   leg 1   xp = A1 x, Pp = A1 P A1' + Q1 to the message's time        AIS   S = Pp + r I4, K = Pp S^-1 (through a Cholesky factor of
 *   S), x = xp + K (m - xp), P = Pp - K Pp        leg 2   predict with A2, Q2 to the scan's time        radar   update, with a plot
 * and the backward pass takes two Rauch-Tung-Striebel steps over such a node: over leg 2 to the smoothed state at the message's time
 * (from the filtered state there, behind the AIS update; an intermediate, not output), then over leg 1 to the node in front.  A node
 * without a message is mht_smooth_tracks' step, operation for operation: a batch without any gives that seam's bits.
 * model: nx == 4 and transition == 0 are required (MHT_E_INVALID); A, Q, C, R as for mht_smooth_tracks.  len, x_init, P_init, z, has_z,
 * xs, Ps, the error behaviour and the layouts are mht_smooth_tracks' with nx = 4.  Next to them, per node and track:
 *   kind     dev [L_max][n_tracks] uint8: 0 plain step, no plot; 1 plain step, radar update; 2 AIS legs only; 3 AIS legs, then radar
 *            update.  The device takes the radar update from has_z and the legs from kind >= 2: the caller keeps has_z == kind & 1.
 *   ais_z    dev [L_max][4][n_tracks] f64: the message's state [x, y, vx, vy]      ais_r  dev [L_max][n_tracks] f64: its sigma^2 (> 0)
 *   leg      dev [L_max][n_tracks] int32: the node's entry of the leg table     (all three read where kind >= 2 only)
 *   legs     dev [n_legs][52] f64: one entry per distinct (dT1, dT2) of the batch -- A1 [16] row-major, Q1 [10] upper triangle row
 *            by row, A2 [16], Q2 [10]: Phi and Q of the two time steps as the forest used them (float32, widened).  NULL with n_legs == 0.
 *   work     dev, work_bytes >= mht_smooth_ais_work_bytes(n_tracks, L_max) (two filtered states per node: at the scan's and at the
 *            message's time; 0 for a negative size): MHT_E_CAPACITY if it is smaller.
 * kind, ais_r, leg and legs are device arrays the host cannot see: THE CALLER OWNS THEIR CONTRACT -- 0 <= leg < n_legs wherever
 * kind >= 2, and r > 0 (pymht_amd.smoothing checks both before it uploads).  Row 0 of every per-node array is ignored; rows >= len[t]
 * of track t are not read.  Exported by both builds. */
size_t mht_smooth_ais_work_bytes(int32_t n_tracks, int32_t L_max);
int mht_smooth_tracks_ais(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                          const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                          const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, int32_t n_legs,
                          double* xs, double* Ps, void* work, size_t work_bytes);

/* ---- seam (v), EM: Q, R and the initial state learned per track by expectation-maximisation, then the smoother -- OPT-IN: nothing
 * routes here unless the caller asks (em=5 in the Python API) ---------------------------------------------------------------------------
 * What the reference's pykalman call does per track (pyTarget.py:580-609: em(n_iter = 5), then smooth), restated: the target is the
 * algorithm (tests/smooth_em_ref.py), not pykalman's bits.  A and C stay the model's; theta = (Q, R, x0, P0) is per track and starts at
 * the model's Q and R (widened) and the track's x_init, P_init.  One iteration, all four updated from the same E-step:
 *   E-step   mht_smooth_tracks' forward and backward recursion under theta: xs_k, Ps_k, G_k, and X_k = Ps_{k+1} G_k' = Cov(x_{k+1}, x_k | z)
 *   M-step   Q <- 1 / (L - 1) sum_{k = 0 .. L-2} [e e' + A Ps_k A' + Ps_{k+1} - X_k A' - A X_k'],  e = xs_{k+1} - A xs_k
 *            R <- 1 / n_obs sum_{k: z_k present} [r r' + C Ps_k C'],  r = z_k - C xs_k;   x0 <- xs_0;   P0 <- Ps_0
 *   a track of one node learns nothing (its output is its input, Q and R stay); a track without a measurement keeps R.
 * After n_iter iterations (0 .. 64, else MHT_E_INVALID) one more E-step under the learned theta writes xs and Ps: n_iter == 0 gives
 * mht_smooth_tracks' bits.  model: nx 4 or 6 and transition == 0 (else MHT_E_INVALID).  len, x_init, P_init, z, has_z, xs, Ps (may be
 * NULL) and the layouts are mht_smooth_tracks'.  Next to them:
 *   Q_out    dev [nx (nx + 1) / 2][n_tracks] f64 out: the learned Q, upper triangle row by row      R_out  dev [3][n_tracks] f64 out: r00, r01, r11
 *   work     dev, work_bytes >= mht_smooth_em_work_bytes(nx, n_tracks, L_max) (>= mht_smooth_work_bytes of the same shape; 0 for a bad
 *            nx or a negative size): MHT_E_INVALID if it is smaller.
 * NOT POSITIVE DEFINITE: nothing keeps a re-estimated Q, R or P0 positive definite.  A track where one stops being so meets the square
 * root of a negative number in a Cholesky factor and its xs, Ps, Q_out, R_out are NaN from there on -- that track's only: it never
 * faults, and no other track's result depends on it.  One kernel launch per walk, n_iter + 1 in all, a wavefront running as long as its
 * longest track in each.  Synchronises.  On MHT_E_INVALID nothing has been launched or written.  Exported by both builds. */
size_t mht_smooth_em_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max);
int mht_smooth_tracks_em(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                         const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_iter,
                         double* xs, double* Ps, double* Q_out, double* R_out, void* work, size_t work_bytes);

/* ---- seam (v), EM with its trace: mht_smooth_tracks_em with the log-likelihood of every track under every theta_i handed out ------
 * Every argument of mht_smooth_tracks_em, its checks, its error codes, and its bits in xs, Ps, Q_out, R_out; behind them
 *   ll_trace  dev [n_iter + 1][n_tracks] f64 out: row i is each track's log-likelihood (mht_score_tracks' ll, below) under theta_i --
 *             theta_0 the call's start values (row 0 is mht_score_tracks' ll of the same arguments, bit for bit), theta_{n_iter} what
 *             the output walk runs under.  EM never decreases it; a track of one node has 0.0 in every row.
 * One forward-only launch in front of each walk, n_iter + 1 more than mht_smooth_tracks_em, on the same stream.  NULL ll_trace with a
 * non-empty batch: MHT_E_INVALID.  Exported by both builds. */
int mht_smooth_tracks_em_ll(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                            const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_iter,
                            double* xs, double* Ps, double* Q_out, double* R_out, void* work, size_t work_bytes, double* ll_trace);

/* ---- seam (vi): how well the model explains the plots of a batch of track histories -- log-likelihood and innovation consistency,
 * stateless, forward pass only ------------------------------------------------------------------------------------------------------
 * The forward (filter) recursion of mht_smooth_tracks, operation for operation -- the filtered states behind a score are that
 * smoother's own -- with nothing kept per node.  Node 0 is the initial state and is NOT an observation (pykalman's loglikelihood()
 * counts one at time 0: these are not its figures).  Per track, over every node k >= 1 with a radar measurement, with
 * v = z_k - C xp_k and S = C Pp_k C' + R:
 *   nis   = sum v' S^-1 v                                  the normalised innovation squared; over a consistent filter it is chi-square
 *                                                          with 2 nObs degrees of freedom
 *   ll    = - 1/2 sum (ln det S + v' S^-1 v + 2 ln 2 pi)   = sum ln N(z_k; C xp_k, S)
 *   nObs  = the number of such nodes
 * A track of one node, or one never detected, gives exactly ll = 0.0, nis = 0.0, nObs = 0.  A det S that is not positive gives NaN in
 * ll and nis of that track only.  model, len, x_init, P_init, z, has_z, their layouts and checks are mht_smooth_tracks'
 * (MHT_E_INVALID for nx other than 4 or 6, transition != 0, a length outside 1 .. L_max).  Next to them:
 *   ll_out   dev [n_tracks] f64 out       nis_out  dev [n_tracks] f64 out       nobs_out  dev [n_tracks] int32 out
 *   work     dev, work_bytes >= mht_score_work_bytes(nx, n_tracks, L_max) (the lengths, nothing per node; 0 for a bad nx or a negative
 *            size): MHT_E_INVALID if it is smaller.
 * One launch, one track per lane; no track's figures depend on its place in the batch.  Synchronises.  On MHT_E_INVALID nothing has
 * been launched or written.  Exported by both builds (nx at run time).
 * mht_score_tracks_ct: the same under the constant-turn model of mht_smooth_tracks_ct (nx == 6, transition == 1, period > 0; A ignored),
 * same sizer with nx = 6.
 * mht_score_tracks_ais: the same under the AIS-aware model of mht_smooth_tracks_ais (nx == 4), with that seam's kind, ais_z, ais_r,
 * leg, legs, n_legs and their contract.  A node that took a message (kind >= 2) is scored at the message's time as well, with
 * v = m - xp(t_m), S = Pp(t_m) + r I4 and ln det S = 2 sum ln U_ii of the Cholesky factor S = U' U the update takes:
 *   ll -= 1/2 (ln det S + v' S^-1 v + 4 ln 2 pi);   nis_ais_out dev [n_tracks] f64 out: sum v' S^-1 v over the messages;
 *   nais_out dev [n_tracks] int32 out: their number.   nis and nObs stay radar-only.  A batch without any message gives
 * mht_score_tracks' ll, nis and nObs bit for bit.  Same sizer with nx = 4. */
size_t mht_score_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max);
int mht_score_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                     const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* ll_out, double* nis_out,
                     int32_t* nobs_out, void* work, size_t work_bytes);
int mht_score_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                        const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* ll_out, double* nis_out,
                        int32_t* nobs_out, void* work, size_t work_bytes);
int mht_score_tracks_ais(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                         const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                         const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, int32_t n_legs,
                         double* ll_out, double* nis_out, int32_t* nobs_out, double* nis_ais_out, int32_t* nais_out, void* work,
                         size_t work_bytes);

/* mht_score_tracks_grid, mht_score_tracks_ct_grid: seam (vi) under n_cand candidate noise models in ONE launch -- the likelihood surface
 * Q and R are tuned over.  Candidate g replaces the model's Q and R and nothing else (A, C and the period stay the batch's; the model's
 * own Q and R are not read), and its row holds what mht_score_tracks / mht_score_tracks_ct give for a model carrying its matrices, bit
 * for bit where those are representable in the model's float32.  Candidates are float64: a tuning grid is not quantised.
 *   n_cand    1 .. 4096, else MHT_E_INVALID
 *   Q_cand    host [n_cand][nx*nx] f64 row-major; the upper triangle is read
 *   R_cand    host [n_cand][4] f64; entries 0, 1 and 3 are read
 *   ll_out    dev [n_cand][n_tracks] f64 out       nis_out  dev [n_cand][n_tracks] f64 out
 *   nobs_out  dev [n_tracks] int32 out (it does not depend on the candidate)
 *   work      dev, work_bytes >= mht_score_grid_work_bytes(nx, n_tracks, L_max, n_cand) (the lengths and the candidate table, each
 *             rounded up to 256 bytes; 0 for a bad nx, a negative size or an n_cand outside its range): MHT_E_INVALID if it is smaller.
 * Everything else, the model checks included, is mht_score_tracks' and mht_score_tracks_ct's.  One launch of ceil(n_tracks / 64) x n_cand
 * workgroups, one (track, candidate) per lane, a workgroup's candidate the same for all its lanes; a det S that is not positive gives NaN
 * in that (candidate, track) only.  Synchronises.  On MHT_E_INVALID nothing has been launched or written; n_tracks == 0 returns MHT_OK and
 * writes nothing.  The AIS-aware model has no grid (its leg table carries a Q per entry): the linear grid scores such histories as
 * mht_score_tracks does.  Exported by both builds (nx at run time). */
size_t mht_score_grid_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max, int32_t n_cand);
int mht_score_tracks_grid(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                          const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_cand,
                          const double* Q_cand, const double* R_cand, double* ll_out, double* nis_out, int32_t* nobs_out, void* work,
                          size_t work_bytes);
int mht_score_tracks_ct_grid(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                             const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_cand,
                             const double* Q_cand, const double* R_cand, double* ll_out, double* nis_out, int32_t* nobs_out, void* work,
                             size_t work_bytes);

/* mht_trace_tracks, mht_trace_tracks_ct, mht_trace_tracks_ais: seam (vi) with its terms handed out PER NODE -- the innovation sequence the
 * filter-consistency checks need (NIS inside its chi-square interval over time, whiteness of the innovations), and what says WHERE a model
 * stops fitting a track.  The walks, models, inputs and checks are mht_score_tracks', mht_score_tracks_ct's and mht_score_tracks_ais's;
 * the filtered states behind a trace are the score's own bits.  In place of the sums:
 *   radar_out  dev [L_max][7][n_tracks] f64 out.  At node k >= 1 of a track with a radar measurement, with v = z_k - C xp_k and
 *              S = C Pp_k C' + R:  elements 0, 1: v;  2, 3, 4: S00, S01, S11;  5: nis_k = v' S^-1 v;
 *              6: ll_k = - 1/2 (ln det S + nis_k + 2 ln 2 pi) = ln N(z_k; C xp_k, S)
 *   ais_out    (mht_trace_tracks_ais) dev [L_max][16][n_tracks] f64 out.  At a node that took a message (kind >= 2), at the message's
 *              time, with v = m - xp(t_m) and S = Pp(t_m) + r I4:  elements 0 .. 3: v;  4 .. 13: the upper triangle of S, row by row;
 *              14: nisAis_k = v' S^-1 v;  15: llAis_k = - 1/2 (ln det S + nisAis_k + 4 ln 2 pi)
 * EVERY other cell of both arrays is written as well, with a quiet NaN: node 0 (the initial state, not an observation), a node without
 * a measurement or without a message, and the rows len[t] <= k < L_max behind a track's end -- the arrays need not be initialised.  A
 * det S that is not positive (a pivot of the factorisation, for a message) leaves v and S as computed and gives NaN in nis and ll of
 * that node of that track only; has_z and kind, which the caller owns, tell such a node from one without a measurement.  Added up in
 * node order (llAis_k in front of ll_k at a node with both) a track's ll_k, nis_k and nisAis_k are mht_score_tracks*' ll, nis and
 * nis_ais bit for bit, and the cells that are not NaN-by-absence count nObs and nAis.
 *   work       dev, work_bytes >= mht_trace_work_bytes(nx, n_tracks, L_max) (the lengths, nothing per node; 0 for a bad nx or a negative
 *              size): MHT_E_INVALID if it is smaller.
 * One launch, one track per lane, the stores of a wavefront contiguous; no track's figures depend on its place in the batch.
 * Synchronises.  On MHT_E_INVALID nothing has been launched or written; n_tracks == 0 returns MHT_OK and writes nothing.  Exported by
 * both builds (nx at run time). */
size_t mht_trace_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max);
int mht_trace_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                     const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* radar_out, void* work,
                     size_t work_bytes);
int mht_trace_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                        const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* radar_out, void* work,
                        size_t work_bytes);
int mht_trace_tracks_ais(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                         const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                         const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, int32_t n_legs,
                         double* radar_out, double* ais_out, void* work, size_t work_bytes);

/* mht_filter_tracks, mht_filter_tracks_ct, mht_filter_tracks_ais: the FILTERED state and covariance of every node of a batch of track
 * histories -- what seam (v) computes on its way forward and keeps in its workspace, and what the score and trace seams compute and
 * discard.  The walks, models, inputs and checks are mht_trace_tracks', mht_trace_tracks_ct's and mht_trace_tracks_ais's: the float64
 * filter of the smoothers, run over the history from the chain's initial state (not the forest's own float32 / float64 chains).  In
 * place of the trace:
 *   xf   dev [L_max][nx][n_tracks] f64 out: the filtered mean of node k.  Node 0 is x_init; node k >= 1 is the state behind the step to
 *        the node and, with a measurement, its radar update -- at the scan's time (an AIS message is taken on the way there)
 *   Pf   dev [L_max][nx (nx + 1) / 2][n_tracks] f64 out: its covariance, the upper triangle row by row (the layout of seam (v)'s Ps)
 * The rows len[t] <= k < L_max behind a track's end are written as well, with a quiet NaN: the arrays need not be initialised.  The
 * filtered states are the smoother's own bits: for every track, rows len[t] - 1 of xf and Pf equal those of xs and Ps of
 * mht_smooth_tracks* on the same batch (the last node's filtered state is its smoothed state).
 *   work dev, work_bytes >= mht_filter_work_bytes(nx, n_tracks, L_max) (the lengths, nothing per node: mht_score_work_bytes' figure; 0
 *        for a bad nx or a negative size): MHT_E_INVALID if it is smaller.
 * One launch, one track per lane, the stores of a wavefront contiguous; no track's figures depend on its place in the batch.
 * Synchronises.  On MHT_E_INVALID nothing has been launched or written; n_tracks == 0 returns MHT_OK and writes nothing.  Exported by
 * both builds (nx at run time). */
size_t mht_filter_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max);
int mht_filter_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                      const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* xf, double* Pf, void* work,
                      size_t work_bytes);
int mht_filter_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                         const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* xf, double* Pf, void* work,
                         size_t work_bytes);
int mht_filter_tracks_ais(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                          const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                          const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, int32_t n_legs,
                          double* xf, double* Pf, void* work, size_t work_bytes);

/* mht_imm_tracks, mht_imm_tracks_ct: an INTERACTING-MULTIPLE-MODEL filter (Blom and Bar-Shalom 1988) over a batch of track histories.
 * The float64 filter of mht_filter_tracks / mht_filter_tracks_ct is run under n_modes noise levels at once, mixed through a Markov
 * chain over the modes; per node it hands out the posterior probability of every mode -- a manoeuvre detector per track and scan --
 * and one combined state and covariance in the layout of mht_filter_tracks (what mht_nees_nodes takes), per track the log-likelihood
 * of its plots under the mixture, comparable with mht_score_tracks' figure.  The batch (len .. has_z) and the model checks are
 * mht_filter_tracks' and mht_filter_tracks_ct's; the model's own Q and R are not read.
 *   n_modes  1 .. 4
 *   Q        host [n_modes][nx][nx] f64, R host [n_modes][2][2] f64: mode j's noise (the upper triangles are read)
 *   Pi       host [n_modes][n_modes] f64: Pi[i][j] = P(mode j at node k | mode i at node k - 1); entries in [0, 1] (zeros are legal),
 *            every row adding up to 1 within 1e-9
 *   mu0      host [n_modes] f64: the probabilities at node 0, in [0, 1], adding up to 1 within 1e-9
 *   mu       dev [L_max][n_modes][n_tracks] f64 out;  x dev [L_max][nx][n_tracks] f64 out;  P dev [L_max][nx (nx + 1) / 2][n_tracks] f64
 *            out, the upper triangle row by row;  ll dev [n_tracks] f64 out;  nobs dev [n_tracks] int32 out
 * Node 0: every mode holds (x_init, P_init), mu = mu0, (x, P) = (x_init, P_init).  Node k >= 1, sums over i ascending:
 *   cbar_j = sum_i Pi[i][j] mu_i;  where cbar_j > 0 mode j starts from the mixture w_ij = Pi[i][j] mu_i / cbar_j of the modes' states,
 *   x0_j = sum_i w_ij x_i, P0_j = sum_i w_ij (P_i + (x_i - x0_j)(x_i - x0_j)'), else from its own;  it advances under Q_j (constant turn:
 *   Phi(T, w) at x0_j[4]) and, with a plot, updates under R_j with lam_j = ln N(z; C xp_j, S_j), mht_score_tracks' term;  then
 *   m = max_j lam_j, u_j = cbar_j exp(lam_j - m), s = sum_j u_j, mu_j = u_j / s, ll += m + ln s, nobs += 1 -- without a plot mu_j = cbar_j;
 *   x = sum_j mu_j x_j, P = sum_j mu_j (P_j + (x_j - x)(x_j - x)').
 * With n_modes == 1 (Pi = [[1]]) x and P are mht_filter_tracks' bits and ll, nobs are mht_score_tracks'.  A track of one node, or one
 * never detected, gives exactly ll = 0.0 and nobs = 0.  A mode whose det S is not positive at some plot makes that track's ll NaN and its
 * rows from that node on unspecified; no other track is touched.  The rows len[t] <= k < L_max behind a track's end are written with a
 * quiet NaN: the arrays need not be initialised.
 *   work dev, work_bytes >= mht_imm_work_bytes(nx, n_tracks, L_max, n_modes) (the lengths, the modes, Pi, mu0; 0 for a bad nx or
 *        n_modes, a negative size or an empty batch): MHT_E_INVALID if it is smaller.
 * One launch, one (track, mode) per lane -- the four lanes of a quad are the modes of a track and read each other's registers; no
 * track's figures depend on its place in the batch.  Synchronises.  On MHT_E_INVALID (a null array, n_modes outside 1 .. 4, a length
 * outside 1 .. L_max, a short workspace, the wrong nx or transition, an entry of Pi or mu0 outside [0, 1], a sum that is not 1) nothing
 * has been launched or written; n_tracks == 0 returns MHT_OK and writes nothing.  The AIS-aware model is not run under an IMM (out of
 * scope: its per-node message arrays are not taken).  Exported by both builds (nx at run time). */
size_t mht_imm_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max, int32_t n_modes);
int mht_imm_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                   const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes, const double* Q, const double* R,
                   const double* Pi, const double* mu0, double* mu, double* x, double* P, double* ll, int32_t* nobs, void* work,
                   size_t work_bytes);
int mht_imm_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                      const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes, const double* Q, const double* R,
                      const double* Pi, const double* mu0, double* mu, double* x, double* P, double* ll, int32_t* nobs, void* work,
                      size_t work_bytes);

/* mht_imm_smooth_tracks, mht_imm_smooth_tracks_ct: the FIXED-INTERVAL IMM SMOOTHER over a batch of track histories -- the filter of
 * mht_imm_tracks / mht_imm_tracks_ct walked forward, then a mode-matched Rauch-Tung-Striebel pass walked backward (Nadarajah,
 * Tharmarasa, McDonald and Kirubarajan 2012 for modes that share the state space, restated in csrc/mht_imm_smooth.h).  Per node it hands
 * out the probability of every mode IN HINDSIGHT -- on time at the start and at the end of a manoeuvre, where the filter's is several
 * scans late -- and one smoothed state and covariance that needs no choice of a single noise level.  The arguments up to mu0, their
 * checks and the model checks are mht_imm_tracks' and mht_imm_tracks_ct's.  Then
 *   mus      dev [L_max][n_modes][n_tracks] f64 out: the smoothed mode probabilities
 *   xs       dev [L_max][nx][n_tracks] f64 out;  Ps dev [L_max][nx (nx + 1) / 2][n_tracks] f64 out, the upper triangle row by row: the
 *            smoothed combined state and covariance, in mht_filter_tracks' layout (what mht_nees_nodes takes)
 *   muf      dev [L_max][n_modes][n_tracks] f64 out, or NULL: the FILTERED mode probabilities, mht_imm_tracks' mu
 *   ll       dev [n_tracks] f64 out and nobs dev [n_tracks] int32 out, or both NULL: mht_imm_tracks' figures
 * Forward: mht_imm_tracks' recursion, every mode keeping per node its own state after its step, (xf_j, Pf_j), and its probability mu_j.
 * Backward, last node: xs_j = xf_j, Ps_j = Pf_j, mus = mu, (xs, Ps) the filter's combined state.  Node k = L - 2 .. 0, sums over i ascending:
 *   d_j = sum_i Pi[j][i] mus_i(k+1);  where d_j > 0 mode j goes back from the mixture b_i = Pi[j][i] mus_i(k+1) / d_j of the smoothed
 *   states of node k + 1, x0_j = sum_i b_i xs_i, P0_j = sum_i b_i (Ps_i + (xs_i - x0_j)(xs_i - x0_j)'), else from its own;
 *   A_j = A (constant turn: Phi(T, w) at xf_j(k)[4]), xp_j = A_j xf_j(k), M_j = A_j Pf_j(k) A_j';
 *   lam_ji = -1/2 |L^-1 (xs_i(k+1) - xp_j)|^2 - sum_e ln L_ee, L L' = M_j + Q_i;  m_j = max of lam_ji over the i with Pi[j][i] > 0,
 *   lnL_j = m_j + ln sum_i (Pi[j][i] > 0 ? Pi[j][i] exp(lam_ji - m_j) : 0);
 *   mht_smooth_tracks' step under Q_j: Pp = M_j + Q_j, G = Pf_j A_j' Pp^-1, xs_j(k) = xf_j + G (x0_j - xp_j), Ps_j(k) = Pf_j + G (P0_j - Pp) G';
 *   top = max of lnL_j over the j with mu_j(k) > 0, u_j = mu_j(k) > 0 ? mu_j(k) exp(lnL_j - top) : 0, mus_j(k) = u_j / sum_j u_j;
 *   xs(k), Ps(k) the moments of the (xs_j(k), Ps_j(k)) under mus(k).
 * The forward pass predicted mode j from its mixed state, the backward gain uses xf_j(k): that is the method's approximation.  No
 * logarithm of Pi or of a probability is taken: zeros are legal.  muf, ll and nobs are mht_imm_tracks' bits, and at a track's last node
 * so are mus, xs, Ps its mu, x, P.  With n_modes == 1 (Pi = [[1]]) xs and Ps are mht_smooth_tracks' (mht_smooth_tracks_ct's) bits and
 * mus is exactly 1; with Pi = I and mu0 = (0, 1) they are that smoother's bits under mode 1's Q.  The rows len[t] <= k < L_max behind a
 * track's end are written with a quiet NaN.
 *   work dev, work_bytes >= mht_imm_smooth_work_bytes(nx, n_tracks, L_max, n_modes): mht_imm_work_bytes' figure plus per node and mode
 *        the row [x | P packed | mu], L_max n_modes (nx + nx (nx + 1) / 2 + 1) n_tracks 8 bytes rounded up to 256 (0 where
 *        mht_imm_work_bytes gives 0): MHT_E_INVALID if it is smaller.
 * One launch, one (track, mode) per lane, forward and then backward; a lane reads back only the rows it stored itself; no track's
 * figures depend on its place in the batch.  Synchronises.  Error codes and the rule that nothing is launched or written on
 * MHT_E_INVALID are mht_imm_tracks' (ll without nobs, or nobs without ll, is a null array); n_tracks == 0 returns MHT_OK and writes
 * nothing.  The AIS-aware model is not run.  Exported by both builds (nx at run time). */
size_t mht_imm_smooth_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max, int32_t n_modes);
int mht_imm_smooth_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                          const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes,
                          const double* Q, const double* R, const double* Pi, const double* mu0, double* mus, double* xs, double* Ps,
                          double* muf, double* ll, int32_t* nobs, void* work, size_t work_bytes);
int mht_imm_smooth_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                             const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes,
                             const double* Q, const double* R, const double* Pi, const double* mu0, double* mus, double* xs, double* Ps,
                             double* muf, double* ll, int32_t* nobs, void* work, size_t work_bytes);

/* mht_nees_nodes: is the covariance a filter reports honest?  The estimation error e = x - truth and the normalised estimation error
 * squared e' P^-1 e of every node of a batch against ground truth -- the test that sees the unmeasured states, which the innovations
 * (mht_trace_tracks*) do not.  The inputs lie where mht_filter_tracks* (xf, Pf) or mht_smooth_tracks* (xs, Ps) wrote them:
 *   nx       4 or 6;  D: 2, 4 or nx -- the leading components [x, y, vx, vy, ...] the truth carries
 *   x        dev [L_max][nx][n_tracks] f64;  P dev [L_max][nx (nx + 1) / 2][n_tracks] f64, the packed upper triangle
 *   truth    dev [L_max][nx][n_tracks] f64: components >= D are not read
 *   present  dev [L_max][n_tracks] uint8: non-zero where the node has a truth to be held against
 *   out      dev [L_max][nx + 3][n_tracks] f64 out: elements 0 .. nx - 1: e (NaN at components >= D);  nx: nees2, over the position;
 *            nx + 1: nees4, over position and velocity;  nx + 2: neesN, over the full state
 * One factorisation P = U' U and one forward substitution U' y = e per cell give all three: the sum of y_j^2 over j < d is the NEES of
 * the leading d components under their marginal covariance, exactly.  A figure that needs components beyond D is NaN.  A cell whose flag
 * is 0, or whose x or P holds a NaN (the rows behind a track's end), is NaN throughout.  A pivot j that is not positive gives NaN in
 * every figure that includes component j, in that cell only; the figures in front of it stay valid.  EVERY cell is written.
 * One launch, one cell per lane with the track index fastest (loads and stores of a wavefront contiguous).  Synchronises.
 * MHT_E_INVALID: a bad nx or D, a negative size, a null array of a batch that is not empty; nothing has then been launched or written.
 * n_tracks == 0 or L_max == 0 returns MHT_OK.  Exported by both builds. */
int mht_nees_nodes(mht_ctx* ctx, int32_t nx, int32_t n_tracks, int32_t L_max, int32_t D, const double* x, const double* P,
                   const double* truth, const uint8_t* present, double* out);

/* mht_encounters: which tracks come close to each other, or to the own ship, within the next minutes, and how sure is that?  n entries
 * at one common time -- one row of mht_filter_tracks' layout -- are propagated K steps of dt seconds with a linear model
 * (x_k = Phi x_{k-1}, P_k = Phi P_{k-1} Phi' + Q, k = 0 the entries as they are), and for every pair (i, j) with i < first and
 * i < j < n, the two taken as INDEPENDENT, d_k the difference of the positions and Sigma_k the sum of their 2 x 2 covariances:
 *   tcpa, dcpa  the closest point of approach of the piecewise-linear path through d_0 .. d_K: its time (earliest) and distance.  The
 *               exact CPA within the horizon for a constant-velocity model; the piecewise-linear figure for a constant-acceleration one
 *   md2         min over k of d_k' Sigma_k^-1 d_k
 *   pc, tpc     max over k of pc_k, the probability mass of N(d_k, Sigma_k) within the disc of radius R, and the time k dt of the
 *               (earliest) maximum.  pc_k is DEFINED by a rule -- csrc/mht_encounter.h: the closed-form eigen-decomposition of Sigma_k,
 *               a clip at 8 sigma along the narrow axis (beyond it pc_k is 0 exactly) and a 64-node Gauss-Legendre rule of exp and
 *               erfc -- which is good to about 1e-6 absolute against the exact mass, not exact
 *   nx     4 or 6, the state [x, y, vx, vy, ...];  K: 1 .. 64 steps;  dt > 0 seconds;  R > 0
 *   n      entries;  first: 0 .. n.  first = n: all pairs;  first = 1 with the own ship as entry 0: the own ship against everyone
 *   Phi, Q HOST [nx][nx] f64, row-major, for one step of dt (of Q the upper triangle is read)
 *   x      dev [nx][n] f64;  P: dev [nx (nx + 1) / 2][n] f64, the packed upper triangle
 *   out    dev [5][first][n] f64 out: tcpa, dcpa, md2, pc, tpc.  EVERY cell is written; the cells with j <= i are NaN
 *   work   dev, at least mht_encounter_work_bytes(n, K) bytes (0 for n <= 0 or a K outside 1 .. 64): the propagated positions and
 *          their covariances, 5 (K + 1) n doubles
 * A NaN in an entry's x or P makes all five figures of its pairs NaN.  A Sigma_k that is not positive definite at some k makes pc, tpc
 * and md2 of that pair NaN; tcpa and dcpa stay valid.  Cross-correlation between tracks is not modelled.
 * Two launches (one entry per lane, then one cell per lane with j fastest).  Synchronises.
 * MHT_E_INVALID: nx not 4 or 6, K outside 1 .. 64, R <= 0 or dt <= 0 (or NaN), first outside 0 .. n, a null array or a work buffer too
 * small for a call that is not empty; nothing has then been launched or written.  n == 0 or first == 0 returns MHT_OK and launches
 * nothing.  Exported by both builds. */
size_t mht_encounter_work_bytes(int32_t n, int32_t K);
int mht_encounters(mht_ctx* ctx, int32_t nx, int32_t n, int32_t first, int32_t K, double dt, double R, const double* Phi, const double* Q,
                   const double* x, const double* P, double* out, void* work, size_t work_bytes);

/* mht_trial_manoeuvres: "and if I alter course by 40 degrees to starboard, or slow to half speed, in 30 s?" -- G candidate manoeuvres
 * of the own ship, each held against every one of n tracks over the horizon, in one call: the tracks are propagated once (as
 * mht_encounters propagates them), a cell (g, j) holds mht_encounters' five figures of candidate g against track j (d_k = own - track,
 * Sigma_k = S_own + S_j,k, pc by the same rule), and per candidate the worst track is folded out.
 * THE MANOEUVRE (csrc/mht_trial.h states the operations).  The own ship at the current scan is at p0 with velocity v0 and may carry a
 * constant 2 x 2 position covariance S_own, which is its covariance at every step.  A candidate is (dpsi, f, t0): the course change in
 * radians, positive counter-clockwise in the tracker's axes, |dpsi| <= pi; the speed factor f >= 0; the delay t0 >= 0 in seconds.  One
 * turn rate w > 0 (rad/s) serves all candidates.  With sg = sign(dpsi), te = t0 + |dpsi| / w and Rot(a) the plane rotation by a:
 *   t <= t0        p(t) = p0 + t v0
 *   t0 < t <= te   tau = t - t0, sw = sin(w tau) / w, cw = (1 - cos(w tau)) / w:  p(t) = p(t0) + f [sw, -sg cw; sg cw, sw] v0
 *                  (the arc of a constant turn at rate sg w and speed f |v0|; the speed changes at t0 at once, ARPA's convention)
 *   t > te         p(t) = p(te) + (t - te) f Rot(dpsi) v0
 * dpsi = 0 skips the arc, a t0 beyond the horizon is "stand on", a turn may end beyond the horizon.  Positions are evaluated in closed
 * form at t = k dt, k = 0 .. K, never accumulated.  A NaN in a candidate, in own or in Sown makes that candidate's row NaN.
 *   nx, n, K, dt, R, Phi, Q, x, P   as for mht_encounters; the n entries are the tracks (the own ship is not one of them)
 *   G        1 .. MHT_TRIAL_MAX_CANDIDATES candidates
 *   own      HOST [4] f64: p0 (x, y), v0 (x, y);  Sown: HOST [3] f64: xx, xy, yy;  w: the turn rate
 *   cand     HOST [G][3] f64: dpsi, f, t0
 *   out      dev [5][G][n] f64 out: tcpa, dcpa, md2, pc, tpc.  EVERY cell is written
 *   summary  dev [4][G] f64 out: pcMax, pcArg, dcpaMin, dcpaArg -- the largest pc of the row and the smallest dcpa, each with its track
 *            index as a double.  NaN cells do not take part, equal figures go to the lowest track; a row without a figure gives NaN, -1
 *   work     dev, at least mht_trial_work_bytes(n, G, K) bytes (0 for n <= 0, a G or a K out of range): the trajectories
 *            pos [K + 1][2][n + G] and S [K + 1][3][n + G] (tracks first), the per-tile partials, the staged entries and candidates
 * Four launches (tracks, candidates, cells with a fold per tile of 256 tracks, one wavefront per candidate over the tiles); no atomic,
 * the bits do not depend on the order workgroups run in.  Synchronises.
 * MHT_E_INVALID: nx not 4 or 6, K outside 1 .. 64, G outside its range, n < 0, R, dt or w not positive and finite; and for a call that
 * is not empty a null array, an infinite own or Sown, a candidate that is neither finite nor NaN or out of range, a work buffer too
 * small; nothing has then been launched or written.  n == 0 returns MHT_OK and launches nothing.  Exported by both builds. */
#define MHT_TRIAL_MAX_CANDIDATES 4096
size_t mht_trial_work_bytes(int32_t n, int32_t G, int32_t K);
int mht_trial_manoeuvres(mht_ctx* ctx, int32_t nx, int32_t n, int32_t G, int32_t K, double dt, double R, const double* Phi, const double* Q,
                         const double* x, const double* P, const double* own, const double* Sown, double w, const double* cand, double* out,
                         double* summary, void* work, size_t work_bytes);

/* mht_trial_hypotheses: the trial manoeuvres held against EVERY LIVE HYPOTHESIS of every target, not only the selected one.  The
 * entries are L leaves of the forest in target order (mht_forest_leaves*' order), the leaves of target t being seg[t] .. seg[t + 1] - 1;
 * a cell (g, l) is mht_trial_manoeuvres' cell of candidate g against leaf l -- the same code, the same bits -- and per (candidate,
 * target) the cells of the target's leaves are folded (csrc/mht_trial_hyp.h states the operations):
 *   pcWorst, pcWorstLeaf   the largest pc over the target's leaves and its leaf, a GLOBAL leaf index as a double
 *   dcpaMin, dcpaMinLeaf   the smallest dcpa and its leaf.  mht_trial_manoeuvres' fold: a NaN figure takes no part, equal figures go to
 *                          the lowest leaf, no figure gives NaN and -1; bit for bit independent of the grouping
 *   pcMean                 sum(w_l pc_l) / sum(w_l) over the leaves whose pc and cnllr are both not NaN, w_l = exp(-(cnllr_l - cmin_t)),
 *                          cmin_t the smallest non-NaN cnllr of the target (a lower cumulative NLLR is the better hypothesis); NaN where
 *                          there is no such leaf.  A target of one leaf has w = 1 and pcMean = pc bit for bit
 *   pcSel, dcpaSel, tcpaSel   the cell of leaf sel[t]: what the best-hypothesis view reports.  NaN where sel[t] = -1
 * THE APPROXIMATION.  The weights normalise INSIDE ONE TARGET: the hypotheses of a target are weighed against each other by their own
 * cumulative scores, and the exclusion constraints BETWEEN targets, which the ILP enforces (two targets cannot take the same plot), are
 * ignored.  This is the usual track-oriented approximation of the hypothesis probabilities; it is not the probability of a global
 * hypothesis.
 *   nx, K, dt, R, Phi, Q, own, Sown, w, cand, G   as for mht_trial_manoeuvres
 *   L, T     leaves and targets, 1 <= T <= L for a call that is not empty
 *   x        dev [nx][L] f64;  P: dev [nx (nx + 1) / 2][L] f64;  cnllr: dev [L] f64, the cumulative NLLR of every leaf (NaN: the leaf
 *            has no weight and takes no part in pcMean; +inf: weight 0)
 *   seg      HOST [T + 1] int32: seg[0] = 0, non-decreasing (an empty target is allowed), seg[T] = L
 *   sel      HOST [T] int32: the GLOBAL index of the target's selected leaf, inside seg[t] .. seg[t + 1] - 1, or -1
 *   table    dev [5][G][L] f64 out, or NULL: mht_trial_manoeuvres' table for n = L.  The figures below do not need it to exist
 *   fig      dev [8][G][T] f64 out, in the order above.  EVERY cell is written (an empty target: NaN and -1)
 *   weight   dev [L] f64 out: w_l / sum(w) over the target's leaves that have a cnllr, the sum taken in leaf order; NaN for a leaf
 *            without one
 *   work     dev, at least mht_trial_hyp_work_bytes(L, T, G, K) bytes (0 for sizes out of range)
 * Five launches (weights, one target per lane; leaves; candidates; cells with a serial fold per piece of a target inside a tile of 256
 * leaves; one lane per (candidate, target) over the pieces in tile order); no atomic, the bits do not depend on the order workgroups
 * run in.  The small host arrays have been copied when the call returns.  Synchronises.
 * MHT_E_INVALID: what mht_trial_manoeuvres refuses, and T outside 1 .. L, a seg that does not start at 0, decreases or does not end at
 * L, a sel outside its segment; nothing has then been launched or written.  L == 0 returns MHT_OK and launches nothing.  Exported by
 * both builds. */
size_t mht_trial_hyp_work_bytes(int32_t n_leaves, int32_t n_targets, int32_t G, int32_t K);
int mht_trial_hypotheses(mht_ctx* ctx, int32_t nx, int32_t L, int32_t T, int32_t G, int32_t K, double dt, double R, const double* Phi,
                         const double* Q, const double* x, const double* P, const double* cnllr, const int32_t* seg, const int32_t* sel,
                         const double* own, const double* Sown, double w, const double* cand, double* table, double* fig, double* weight,
                         void* work, size_t work_bytes);

/* mht_mc_encounters: encounters by MONTE CARLO.  Every target is a Gaussian mixture of components -- the leaves of the forest with
 * their weights --; `particles` particles per target are drawn from it, walked over `steps` steps of dt seconds WITH process noise, and
 * held against G paths of the own ship (csrc/mht_mc.h states the method, the random numbers and the order of every sum).  It answers
 * what the Gaussian rule of mht_encounters cannot: the probability of coming within R AT ANY TIME of the horizon (a first-passage
 * figure over correlated steps), a target whose hypotheses disagree (a mixture), and the constant-turn model, whose transition
 * Phi(dt, w) is taken at every particle's own turn rate.
 *   nx, transition   4 or 6 states; 0: linear, x+ = Phi x + noise; 1: constant turn (models/ct.py's state, nx 6 only), Phi is not read
 *   nComp, nTarget   components and targets, 1 <= nTarget <= nComp
 *   G, steps, particles   1 .. MHT_MC_MAX_PATHS, 1 .. MHT_MC_MAX_STEPS, a multiple of MHT_MC_WARP in MHT_MC_WARP .. MHT_MC_MAX_PARTICLES
 *   seed             of the Philox4x32-10 stream: one seed, one result, bit for bit, on any device and under any grid
 *   dt, radius       the step and the safety radius R, positive and finite
 *   Phi, Q           HOST [nx][nx] row-major f64, finite; of Q the upper triangle is read.  Q is positive SEMIdefinite (models/ct.Q
 *                    has rank 3): it is factored on the host with a zero-pivot rule
 *   x, P             dev [nx][nComp] f64 and dev packed upper [nx (nx + 1) / 2][nComp] f64; a P may be singular or zero
 *   first            dev [nTarget + 1] int32: a target's components are first[t] .. first[t + 1] - 1; first[0] = 0, STRICTLY ascending,
 *                    first[nTarget] = nComp.  Read back and checked before anything is launched
 *   cdf              dev [nComp] f64: the cumulative weight inside the target, its last entry 1.0
 *   ownPath          dev [G][steps + 1][2] f64: the own ship's position at every step of every path
 *   within           dev [G][steps + 1][nTarget] uint32 out: the particles with |X_k - own_k| < R at step k
 *   ever             dev [G][nTarget] uint32 out: the particles whose piecewise-linear path comes inside R; ever >= within at every step
 *   valid            dev [nTarget] uint32 out: `particles` for a scored target, else 0 -- the divisor of the counts
 *   status           dev [nTarget] int32 out: MHT_MC_OK; MHT_MC_NAN: a NaN in a component's x, P or cdf; MHT_MC_NOT_PSD: a component's
 *                    P is not positive semidefinite.  Every count of such a target is 0
 *   work             dev, at least mht_mc_work_bytes(nx, nComp, nTarget, G, steps, particles) bytes (0 for arguments out of range)
 * Three launches (a component per lane: the factors; a workgroup per slab of a target's particles, a particle per lane; the fold of the
 * slabs), no atomic.  Synchronises.
 * MHT_E_INVALID: a null pointer (Phi may be null with transition 1), arguments out of range, a Phi or Q that is not finite, a Q that is
 * not positive semidefinite, a short work buffer, a `first` that does not ascend strictly from 0 to nComp; nothing has then been
 * launched or written.  Pairs of targets: mht_mc_pair_encounters below.  Out of scope: an own-ship covariance, correlation between
 * targets, the time of the first violation (firstAt, which the pair engine has).  Exported by both builds. */
#define MHT_MC_MAX_PATHS 64            /* own paths per call */
#define MHT_MC_MAX_STEPS 64            /* steps of the horizon */
#define MHT_MC_MAX_PARTICLES 1048576   /* particles per target, 2^20 */
#define MHT_MC_WARP 64                 /* particles come in multiples of a wavefront */
#define MHT_MC_OK 0                    /* status: scored */
#define MHT_MC_NAN 1                   /* a NaN in a component's x, P or cdf */
#define MHT_MC_NOT_PSD 2               /* a component's P is not positive semidefinite */
size_t mht_mc_work_bytes(int32_t nx, int32_t nComp, int32_t nTarget, int32_t G, int32_t steps, int32_t particles);
int mht_mc_encounters(mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t G, int32_t steps, int32_t particles,
                      uint64_t seed, double dt, double radius, const double* Phi, const double* Q, const double* x, const double* P,
                      const int32_t* first, const double* cdf, const double* ownPath, uint32_t* within, uint32_t* ever, uint32_t* valid,
                      int32_t* status, void* work, size_t work_bytes);

/* mht_mc_pair_encounters: Monte-Carlo encounters between PAIRS OF TARGETS -- target against target, what a VTS operator or a fleet
 * monitor asks for -- with the engine of mht_mc_encounters: particle p of target a is held against particle p of target b, both drawn
 * from their target's mixture and walked exactly as mht_mc_encounters walks them (the same Philox stream keyed by (seed, target), the
 * same sums, the constant-turn model included; csrc/mht_mc_pair.h states the definition).  Per pair j = (a, b), with d_k the difference
 * of the two positions at step k:
 *   nx, transition, nComp, nTarget, steps, particles, seed, dt, radius, Phi, Q, x, P, first, cdf   as for mht_mc_encounters
 *   nPair            1 .. MHT_MC_MAX_PAIRS
 *   pairs            dev [nPair][2] int32: the two target indices of every pair, 0 <= a, b < nTarget and a != b.  Duplicates and both
 *                    orders of a pair are allowed (and give equal counts).  Read back and checked before anything is launched
 *   within           dev [steps + 1][nPair] uint32 out: the particles with |d_k| < R at step k
 *   firstAt          dev [steps + 1][nPair] uint32 out: the particles whose relative path comes inside R FIRST at step k (at the step, or
 *                    on the segment that ends in it): the distribution of the time to the first violation; its sum over k is ever
 *   ever             dev [nPair] uint32 out: the particles whose piecewise-linear relative path comes inside R; ever >= within at every step
 *   valid            dev [nPair] uint32 out: `particles` for a scored pair, else 0 -- the divisor of the counts
 *   status           dev [nPair] int32 out: MHT_MC_OK; MHT_MC_NAN: either target has a NaN in a component's x, P or cdf; MHT_MC_NOT_PSD:
 *                    either target has a component whose P is not positive semidefinite (NAN wins).  Every count of such a pair is 0
 *   work             dev, at least mht_mc_pair_work_bytes(nx, nComp, nTarget, nPair, steps, particles) bytes (0 for arguments out of range)
 * No particle position is stored: a target in many pairs is walked once per pair.  Three launches (a component per lane: the factors; a
 * workgroup per slab of a pair's particle indices, a pair of particles per lane; the fold of the slabs), no atomic.  Synchronises.
 * MHT_E_INVALID: as for mht_mc_encounters, and an nPair out of range or a pair that names a target outside 0 .. nTarget - 1 or one
 * target twice; nothing has then been launched or written.  Out of scope: correlation between targets (two targets' particles are
 * independent), pairs across mht_trial_hypotheses' Gaussian cells.  Exported by both builds. */
#define MHT_MC_MAX_PAIRS 1048576       /* pairs per call, 2^20 */
size_t mht_mc_pair_work_bytes(int32_t nx, int32_t nComp, int32_t nTarget, int32_t nPair, int32_t steps, int32_t particles);
int mht_mc_pair_encounters(mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t nPair, int32_t steps,
                           int32_t particles, uint64_t seed, double dt, double radius, const double* Phi, const double* Q, const double* x,
                           const double* P, const int32_t* first, const double* cdf, const int32_t* pairs, uint32_t* within,
                           uint32_t* firstAt, uint32_t* ever, uint32_t* valid, int32_t* status, void* work, size_t work_bytes);

/* mht_mc_zone_encounters: Monte-Carlo GUARD ZONES -- will a target enter a place (a restricted area, a shoal contour, an anchorage, a
 * traffic-separation zone), with what probability within the horizon, and when -- with the engine of mht_mc_encounters: the particles
 * are drawn from their target's mixture and walked exactly as mht_mc_encounters walks them (the same Philox stream keyed by
 * (seed, target), the same sums, the constant-turn model included), and held against nZone simple polygons by a point-in-polygon test
 * at every step and a segment-against-edges test between two steps, so that a zone thinner than one step's travel is not stepped over
 * (csrc/mht_mc_zone.h states the definition, every operation in one order).
 *   nx, transition, nComp, nTarget, steps, particles, seed, dt, Phi, Q, x, P, first, cdf   as for mht_mc_encounters; there is no radius
 *   nZone, nVert     1 .. MHT_MC_ZONE_MAX_ZONES zones of 3 vertices each at least, MHT_MC_ZONE_MAX_VERTS vertices in all at most
 *   zoneFirst        dev [nZone + 1] int32: zone z owns the vertices zoneFirst[z] .. zoneFirst[z + 1] - 1; zoneFirst[0] = 0, ascending in
 *                    strides of 3 at least, zoneFirst[nZone] = nVert.  Read back and checked before anything is launched
 *   zoneXY           dev [nVert][2] f64, finite, metres in the frame of the states: the vertices, either orientation, concave polygons
 *                    included; the edge from a zone's last vertex to its first is implied.  Read back and checked as zoneFirst is
 *   inside           dev [nZone][steps + 1][nTarget] uint32 out: the particles inside the zone at step k
 *   firstAt          dev [nZone][steps + 1][nTarget] uint32 out: the particles that are inside the zone, or whose path segment k - 1 -> k
 *                    meets an edge of it, FIRST at step k: the distribution of the time of entry; its sum over k is ever
 *   ever             dev [nZone][nTarget] uint32 out: the particles that enter the zone at all; ever >= inside at every step
 *   valid, status    dev [nTarget] out, as for mht_mc_encounters
 *   work             dev, at least mht_mc_zone_work_bytes(nx, nComp, nTarget, nZone, steps, particles) bytes (0 for arguments out of range)
 * Three launches (the factors and the fold of mht_mc_encounters; a workgroup per slab of a target's particles, a particle per lane, the
 * zones staged in LDS, a far zone skipped by a whole wavefront), no atomic.  Synchronises.
 * MHT_E_INVALID: as for mht_mc_encounters, and an nZone or nVert out of range, a zoneFirst that does not ascend from 0 to nVert in
 * strides of 3 at least, a vertex that is not finite; nothing has then been launched or written.  Zones that move with
 * the own ship (a polygonal ship domain) are mht_mc_domain_encounters' case.  Out of scope: open gates and polylines (a thin
 * quadrilateral serves), holes, geodetic coordinates, the dwell time inside a zone.  Exported by both builds. */
#define MHT_MC_ZONE_MAX_ZONES 32       /* zones per call */
#define MHT_MC_ZONE_MAX_VERTS 1024     /* vertices of all zones of a call together */
size_t mht_mc_zone_work_bytes(int32_t nx, int32_t nComp, int32_t nTarget, int32_t nZone, int32_t steps, int32_t particles);
int mht_mc_zone_encounters(mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t nZone, int32_t nVert,
                           int32_t steps, int32_t particles, uint64_t seed, double dt, const double* Phi, const double* Q, const double* x,
                           const double* P, const int32_t* first, const double* cdf, const int32_t* zoneFirst, const double* zoneXY,
                           uint32_t* inside, uint32_t* firstAt, uint32_t* ever, uint32_t* valid, int32_t* status, void* work,
                           size_t work_bytes);

/* mht_mc_domain_encounters: Monte-Carlo SHIP DOMAINS -- will a target enter the safety region around the own ship, a polygon that is
 * longer ahead than astern and usually wider to starboard than to port, with what probability within the horizon, and when, for every
 * candidate path of the own ship -- with the engine of mht_mc_encounters: the particles are drawn and walked exactly as
 * mht_mc_encounters walks them (the same Philox stream keyed by (seed, target), the same sums, the constant-turn model included), taken
 * into the own ship's BODY FRAME under the pose of every (path, step) and held there against nDomain simple polygons with the geometry
 * of mht_mc_zone_encounters (csrc/mht_mc_domain.h states the definition, every operation in one order).
 *   nx, transition, nComp, nTarget, steps, particles, seed, dt, Phi, Q, x, P, first, cdf   as for mht_mc_encounters; there is no radius
 *   G, nDomain       G >= 1 own paths and 1 .. MHT_MC_DOMAIN_MAX_DOMAINS domains; a (domain, path) is a CELL, cell = d * G + g, and
 *                    nDomain * G <= MHT_MC_DOMAIN_MAX_CELLS
 *   nVert            3 vertices per domain at least, MHT_MC_DOMAIN_MAX_VERTS in all at most
 *   ownPose          dev [G][steps + 1][4] f64, finite: (ox, oy, ux, uy), the own ship's position and its UNIT heading vector at every
 *                    step, |ux^2 + uy^2 - 1| <= 1e-9 (a vector, not an angle: the device evaluates no sin or cos for the transform).
 *                    Read back and checked before anything is launched
 *   domFirst         dev [nDomain + 1] int32: domain d owns the vertices domFirst[d] .. domFirst[d + 1] - 1; domFirst[0] = 0, ascending
 *                    in strides of 3 at least, domFirst[nDomain] = nVert.  Read back and checked as ownPose is
 *   domXY            dev [nVert][2] f64, finite, metres in the BODY FRAME: the first coordinate to the right of the heading, the second
 *                    ahead (x east, y north: starboard and ahead; a domain is drawn bow-up).  Either orientation, concave allowed, no
 *                    holes.  Read back and checked
 *   The body-frame point of a position (X0, X1) under a pose: dx = X0 - ox, dy = X1 - oy, qx = dx * uy - dy * ux, qy = dx * ux + dy * uy.
 *   THE BODY-FRAME PATH BETWEEN TWO STEPS IS TAKEN AS STRAIGHT, from the point under pose k - 1 to the point under pose k: exact where
 *   the own ship does not turn between the two steps, a chord of a curved path on a step inside an arc (shorter steps are the remedy).
 *   inside           dev [nDomain][G][steps + 1][nTarget] uint32 out: the particles inside the domain at step k
 *   firstAt          dev [nDomain][G][steps + 1][nTarget] uint32 out: the particles that are inside the domain, or whose body-frame
 *                    segment k - 1 -> k meets an edge of it, FIRST at step k; its sum over k is ever
 *   ever             dev [nDomain][G][nTarget] uint32 out: the particles that enter at all; ever >= inside at every step
 *   valid, status    dev [nTarget] out, as for mht_mc_encounters
 *   work             dev, at least mht_mc_domain_work_bytes(nx, nComp, nTarget, G, nDomain, steps, particles) bytes (0 for arguments out
 *                    of range)
 * Three launches (the factors and the fold of mht_mc_encounters; a workgroup per slab of a target's particles, a particle per lane, a
 * cell per lane of the first wavefront, the domains staged in LDS, a far cell skipped by a whole wavefront), no atomic.  Synchronises.
 * MHT_E_INVALID: as for mht_mc_encounters, and a G, nDomain, nDomain * G or nVert out of range, a domFirst that does not ascend from 0
 * to nVert in strides of 3 at least, a vertex or a pose that is not finite, a heading that is not a unit vector; nothing has then been
 * launched or written.  Out of scope: domains around targets or between pairs of targets, a domain that scales with speed, the own
 * ship's covariance, a curved body-frame path inside a turning step, holes, more than 64 cells, a stationary own ship (it has no
 * heading: a guard ring about it is mht_mc_zone_encounters' case).  Exported by both builds. */
#define MHT_MC_DOMAIN_MAX_DOMAINS 4    /* domains per call */
#define MHT_MC_DOMAIN_MAX_VERTS 256    /* vertices of all domains of a call together */
#define MHT_MC_DOMAIN_MAX_CELLS 64     /* nDomain * G */
size_t mht_mc_domain_work_bytes(int32_t nx, int32_t nComp, int32_t nTarget, int32_t G, int32_t nDomain, int32_t steps, int32_t particles);
int mht_mc_domain_encounters(mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t G, int32_t nDomain,
                             int32_t nVert, int32_t steps, int32_t particles, uint64_t seed, double dt, const double* Phi, const double* Q,
                             const double* x, const double* P, const int32_t* first, const double* cdf, const double* ownPose,
                             const int32_t* domFirst, const double* domXY, uint32_t* inside, uint32_t* firstAt, uint32_t* ever,
                             uint32_t* valid, int32_t* status, void* work, size_t work_bytes);

/* mht_gospa_steps: a tracking result scored against ground truth -- GOSPA (generalised optimal sub-pattern assignment, Rahmathullah,
 * Garcia-Fernandez, Svensson 2017, alpha = 2) of a batch of independent steps.  A step has n estimates and m true positions (2-D);
 * with d_ij = sqrt(dx dx + dy dy) in float64 and only pairs with d_ij < c (strictly) assignable,
 *     total = min over partial one-to-one assignments of  sum d_ij^p + c^p / 2 (n + m - 2 |assigned|)            (GOSPA = total^(1/p))
 * and at the optimum loc = sum d_ij^p over the assigned pairs, nMissed = m - |assigned|, nFalse = n - |assigned|.
 *   n_steps    steps of the batch; 0 returns MHT_OK and writes nothing
 *   est_off    host [n_steps + 1]: step s has estimates est_off[s] .. est_off[s + 1] - 1 of est_xy; est_off[0] == 0, non-decreasing
 *   est_xy     dev [est_off[n_steps]][2] f64 (NULL if there is none)
 *   tru_off    host [n_steps + 1], tru_xy dev [tru_off[n_steps]][2] f64: the same for the true positions
 *   c, p       the cut-off, finite and positive (and c^p a finite positive float64); p = 1 or 2.  p = 2 takes no root, p = 1 one;
 *              there is no pow
 *   step_out   dev [n_steps][2] f64 out: total, loc
 *   count_out  dev [n_steps][3] int32 out: nAssigned, nMissed, nFalse
 *   match_out  dev [est_off[n_steps]] int32 out: per estimate the index of its true position LOCAL to the step, or -1
 *   work       dev, work_bytes >= mht_gospa_work_bytes(n_steps, n_est_total, n_tru_total) (the offsets; 0 for a negative size and for
 *              an empty batch)
 * Every cell of the three outputs that belongs to a step is written: they need not be initialised.  The sums are float64, in an order
 * that is the same wherever in the batch a step sits.  Where several assignments are optimal one of them is reported.  A coordinate
 * that is not finite never satisfies d < c: its object is never assigned (pymht_amd.evaluation refuses such input).  Should a step's
 * search run into its iteration bound -- every loop is counted, none spins -- its total and loc are NaN and its matches -1.
 * One launch, one step per workgroup of one wavefront, the search tables in LDS (csrc/mht_gospa.h).  Synchronises.
 * MHT_E_INVALID: a null pointer where a size is not zero, a negative count, offsets that decrease or do not start at 0, a bad c or p,
 * a short workspace.  MHT_E_CAPACITY: a step with more than 2048 objects on either side.  On either nothing has been launched or
 * written.  Exported by both builds. */
size_t mht_gospa_work_bytes(int32_t n_steps, int32_t n_est_total, int32_t n_tru_total);
int mht_gospa_steps(mht_ctx* ctx, int32_t n_steps, const int32_t* est_off, const double* est_xy, const int32_t* tru_off,
                    const double* tru_xy, double c, int32_t p, double* step_out, int32_t* count_out, int32_t* match_out, void* work,
                    size_t work_bytes);

/* mht_ospa2_windows: whole tracks scored against truth trajectories -- OSPA(2) (Beard, Vo, Vo, "A solution for large-scale multi-object
 * tracking", IEEE TSP 2020) of a batch of windows of one run.  Per-step GOSPA says whether the targets were found at each step; it
 * cannot say whether they were KEPT: a track cut into two fragments, or two tracks that swap targets, score 0 at every step.  OSPA(2)
 * is OSPA between the SET OF TRACKS and the SET OF TRUTH TRAJECTORIES, with the time-averaged cut-off distance of a pair as its base
 * distance, so a fragment pays the cut-off for every step of the trajectory it does not cover.
 * A run has n_steps steps, n_trk tracks and n_tru truths, each with a position and a presence flag at every step (gaps allowed).  A
 * window is the inclusive range of steps [lo, hi].  For one window:
 *   members    a track / truth present at one or more of its steps; n_w and m_w of them, N = max(n_w, m_w)
 *   D_ij       of members i, j: over the U >= 1 steps of the window at which at least one of the two is present, a step is NEAR if both
 *              are present and d = sqrt(dx dx + dy dy) < c (float64, strictly), else FAR.  No near step: D_ij = c exactly and (i, j) is no
 *              edge.  Else D_ij = (c nFar + sum of d over the near steps) / U, an edge iff D_ij < c as computed.  The time average
 *              has order 1: there is no pow.
 *   total      min over one-to-one assignments on edges of  sum D_ij^p + c^p (N - nAssigned)        (OSPA(2) = (total / N)^(1/p), 0 if N = 0)
 *   loc        sum D_ij^p over the assigned pairs; the cardinality part is c^p (N - nAssigned)
 * (OSPA on D, since D <= c: leaving a member of the smaller side out costs what assigning it at c would.)
 *   trk_xy     dev [n_steps][n_trk][2] f64, 16-byte aligned; trk_on dev [n_steps][n_trk] uint8, non-zero = present.  Step-major: the lanes
 *              of a wavefront read consecutive objects.  A position whose flag is 0 never reaches a result (it may be NaN).
 *   tru_xy     dev [n_steps][n_tru][2], tru_on dev [n_steps][n_tru]: the same for the truths
 *   win_lo, win_hi   host [n_win]: 0 <= lo <= hi < n_steps
 *   c, p       as in mht_gospa_steps
 *   win_out    dev [n_win][2] f64 out: total, loc
 *   count_out  dev [n_win][3] int32 out: nAssigned, n_w, m_w
 *   match_out  dev [n_win][n_trk] int32 out: the truth index of a track, -1 for an unassigned member, -2 for a track that is no member
 *   work       dev, 16-byte aligned, work_bytes >= mht_ospa2_work_bytes(n_trk, n_tru, n_steps, n_win): the windows, the member lists and
 *              one n_trk x n_tru float64 matrix per window (0 for a negative size, a side above 2048 and an empty batch)
 * Every cell of the three outputs is written.  A window's outputs are the same wherever in the batch it stands.  Should a window's search
 * run into its iteration bound its total and loc are NaN and no track of it is assigned.  Three launches on the context's stream
 * (membership; the base distances, O(n_win n_trk n_tru W); one wavefront per window for the search of csrc/mht_gospa.h with its tables
 * in LDS), then the seam waits.  n_win == 0 or n_steps == 0: MHT_OK, nothing launched or written.
 * MHT_E_INVALID: a null array with a non-zero count, a negative count, p not 1 or 2, a bad c, a window with lo < 0, hi >= n_steps or
 * lo > hi, positions or workspace not aligned, a short workspace.  MHT_E_CAPACITY: more than 2048 tracks or truths.  On either nothing has
 * been launched or written.  Exported by both builds.
 * mht_ospa2_set_timing(1) makes later calls of this process (of at most 32768 windows) record events around the three launches;
 * mht_ospa2_stage_times gives the last such call's ms [3]: membership, base distances, assignment (tools/ospa2_cost.py). */
size_t mht_ospa2_work_bytes(int32_t n_trk, int32_t n_tru, int32_t n_steps, int32_t n_win);
int mht_ospa2_windows(mht_ctx* ctx, int32_t n_steps, int32_t n_trk, const double* trk_xy, const uint8_t* trk_on, int32_t n_tru,
                      const double* tru_xy, const uint8_t* tru_on, int32_t n_win, const int32_t* win_lo, const int32_t* win_hi, double c,
                      int32_t p, double* win_out, int32_t* count_out, int32_t* match_out, void* work, size_t work_bytes);
void mht_ospa2_set_timing(int32_t on);
void mht_ospa2_stage_times(float* ms);

/* mht_kbest_hypotheses: the K best GLOBAL hypotheses of every cluster -- the figure of a multi-hypothesis tracker that says how
 * ambiguous a cluster is, what the second-best joint explanation is, and how probable a leaf is once the other targets have had
 * their say.  The instance is mht_solve_blp's sparse form: nT targets, target t owning the columns group_ptr[t] .. group_ptr[t + 1] - 1
 * (a column is a leaf), every column a cost and up to `depth` row ids (rows dev [depth][nHyp], -1 = none).  Clusters: cluster c has the
 * targets cluster_targets[cluster_ptr[c] .. cluster_ptr[c + 1] - 1], ascending; row ids are LOCAL to the cluster, in
 * [0, MHT_KBEST_MAX_ROWS).  A global hypothesis of a cluster picks one column per target so that no two picked columns share a row
 * id; its cost is the float64 sum of the picked costs from 0.0, left to right in the cluster's target order.  Listed per cluster are
 * the K cheapest under the total order (cost, then the tuple of column indices in target order): the list is unique, ties are decided.
 * A column whose cost is not finite is never picked.
 *   count [nC]       hypotheses listed;  status [nC] MHT_KBEST_*;  nodes [nC] sibling tests the search made (<= node_limit)
 *   hyp_cost [K][nC] ascending; hyp_prob [K][nC] = exp(-(cost[r] - cost[0])) / sum over the listed r (summed in ascending r: the
 *                    probabilities are those of the K listed hypotheses, truncated); NaN beyond count
 *   hyp_sel [K][nT]  the global column of every target in hypothesis r of its cluster; -1 beyond count and for a target in no cluster
 *   marginal [nHyp]  sum of hyp_prob[r] over the listed hypotheses that hold the column (ascending r); 0 for a column in none and for
 *                    a target in no cluster; NaN for the columns of a cluster that was not searched
 *   work             dev, work_bytes >= mht_kbest_work_bytes(nHyp, nT, nC, depth, K): the listed tuples, 2 K nT bytes rounded up to
 *                    256 (0 for a negative size, K outside 1 .. MHT_KBEST_MAX_K or a negative depth)
 * A cluster beyond a limit below -- or whose indices point outside the arrays -- is not searched: MHT_KBEST_TOO_LARGE, count 0.  A
 * row id other than -1 outside the range: MHT_KBEST_BAD_ROWS, count 0; it indexes nothing.  A target without a finite column, or no
 * conflict-free choice: MHT_KBEST_OK with count 0.  The search is a depth-first branch and bound, one wavefront per cluster
 * (csrc/mht_kbest.h states the bound and its rounding allowance); after node_limit sibling tests it stops with the best found so far.
 * The targets of different clusters must be disjoint.  One launch behind two fills, ASYNCHRONOUS on the ctx stream (mht_synchronize).
 * MHT_E_INVALID, nothing launched or written: a null pointer (rows may be null with depth 0), nHyp, nT or nC < 1, depth < 0, K outside
 * 1 .. MHT_KBEST_MAX_K, node_limit < 1, a short workspace.  Exported by both builds (the search is model-free). */
#define MHT_KBEST_MAX_K 64          /* hypotheses listed per cluster */
#define MHT_KBEST_MAX_TARGETS 32    /* targets per cluster */
#define MHT_KBEST_MAX_COLUMNS 1024  /* columns per cluster */
#define MHT_KBEST_MAX_DEPTH 16      /* row ids per column */
#define MHT_KBEST_MAX_ROWS 2048     /* row ids are local to the cluster, in [0, MHT_KBEST_MAX_ROWS) */
#define MHT_KBEST_OK 0              /* the list is exact; count < K: only count feasible hypotheses exist, 0: infeasible */
#define MHT_KBEST_NODE_LIMIT 1      /* the best found so far, not certified */
#define MHT_KBEST_TOO_LARGE 2       /* not searched */
#define MHT_KBEST_BAD_ROWS 3        /* a row id was out of range */
size_t mht_kbest_work_bytes(int32_t nHyp, int32_t nT, int32_t nC, int32_t depth, int32_t K);
int mht_kbest_hypotheses(mht_ctx* ctx, int32_t nHyp, int32_t nT, int32_t nC, int32_t depth, int32_t K, int32_t node_limit,
                         const int32_t* group_ptr, const int32_t* rows, const double* cost, const int32_t* cluster_ptr,
                         const int32_t* cluster_targets, int32_t* count, int32_t* status, int32_t* nodes, double* hyp_cost,
                         double* hyp_prob, int32_t* hyp_sel, double* marginal, void* work, size_t work_bytes);

/* ---- AIS-aided children: Tracker.__fuseRadarAndAis (tracker.py:417-552), stateless ------------------------------------------
 * Per leaf and per AIS message (a 4-state report [x, y, vx, vy] of a ship with identity mmsi, made inside the radar period in
 * front of the scan; models/ais.py) that gates with it (eta2_ais, tracker.py:111): the leaf is predicted to the message's time,
 * updated with it, predicted on to the scan's time and gated against the radar measurements; one child per gated radar
 * measurement, score (nllr_ais + nllr_radar) / 2, or ONE child without a radar measurement, score nllr_ais (tracker.py:497-526).
 * The messages come grouped as the reference walks them (tracker.py:447-453: message times in the iteration order of their SET,
 * high accuracy before low, list order inside a group; pymht_amd/ais.py::group_messages builds the arrays):
 *   groups  host [nG]: Phi, Q (models/pv.py:12-24, float32) over dT1 = t_message - t_leaves and dT2 = t_scan - t_message,
 *           sigma^2 of the accuracy class (models/ais.py:9-13), first message and count
 *   msgs    host [nA]: state float64[4], mmsi
 * Leaves as in mht_gate_scan_x (x dev [4][L] float64, flags, P dev [L][16] float32, pd), own dev [L] int32 or null: the identity
 * a leaf's track is bound to, 0 = none -- messages of other ships are skipped (pyTarget.py:269-272).  model: C, R, eta2,
 * lambda_ex are read.  lambda_ais = nTargets P_ais / (pi radarRange^2) (tracker.py:438; needs a finite radarRange).
 * Out, CSR by leaf in the reference's order: child_ptr dev [L+1]; out_x dev [4][cap] float64; out_P dev [cap][16] float64 (the
 * reference's fused covariances are float64: ais.C is); out_radar dev [cap] (0-based radar measurement or -1); out_nllr;
 * out_msg dev [cap] index into msgs.  Synchronous; MHT_E_CAPACITY if cap is too small (*n_children = what is needed).
 * 4-state build only. */
typedef struct mht_ais_group {
    float A1[16], Q1[16], A2[16], Q2[16];
    float r_diag;
    int32_t first, count, pad;
} mht_ais_group;
typedef struct mht_ais_msg {
    double state[4];
    int32_t mmsi;
    int32_t pad;
} mht_ais_msg;
int mht_fuse_ais(mht_ctx* ctx, const mht_model* model, int32_t L, const double* x, const uint8_t* flags, const float* P, const double* pd,
                 const int32_t* own, const mht_ais_group* groups, int32_t nG, const mht_ais_msg* msgs, int32_t nA, double eta2_ais,
                 double lambda_ais, const float* z, int32_t M, int32_t* child_ptr, double* out_x, double* out_P, int32_t* out_radar,
                 double* out_nllr, int32_t* out_msg, int32_t cap, int32_t* n_children);

/* The same for leaves whose covariance the reference carries in float64 (ABI 5): P dev [L][16] float64 -- the leaves with MHT_F_COV_F64 in
 * `flags` are fused from it as it is (kalman.predict_single on a float64 node.P_0, tracker.py:449-450: nodes behind an AIS update and their
 * targets' later leaves), the others from its values rounded to float32 (exact when they ARE float32 values). */
int mht_fuse_ais_f64(mht_ctx* ctx, const mht_model* model, int32_t L, const double* x, const uint8_t* flags, const double* P, const double* pd,
                     const int32_t* own, const mht_ais_group* groups, int32_t nG, const mht_ais_msg* msgs, int32_t nA, double eta2_ais,
                     double lambda_ais, const float* z, int32_t M, int32_t* child_ptr, double* out_x, double* out_P, int32_t* out_radar,
                     double* out_nllr, int32_t* out_msg, int32_t cap, int32_t* n_children);

/* ---- the device-resident hypothesis forest: Tracker.addMeasurementList end to end -----------------------------
 * Replaces steps 1-6 of tracker.py:162-307 (grow :207-209, cluster :220, optimise :228-236, terminate :252-253,
 * N-scan prune :258 = seam (iv) Tracker._nScanPruning, tracker.py:1219-1231 / pyTarget.py:343-356) without a host
 * round trip between the stages.  The tree store of pyTarget.Target objects becomes a ring of mht_nodes layers
 * (one per scan of the window) owned by the ctx. */
typedef struct mht_forest_config {
    int32_t max_targets;  /* capacity of the target list */
    int32_t max_nodes;    /* hypotheses per scan layer (children of one scan + roots born in it) */
    int32_t max_meas;     /* measurements per scan (<= 4096; (n_scan + 4) x max_meas rounded up to 64 <= 65536) */
    int32_t n_scan;       /* Tracker.N: N-scan window (tracker.py:112-114) */
    int32_t blp_max_iter; /* dual-ascent steps before branch and bound (200 when < 0; 0 = branch and bound only) */
    int32_t blp_node_limit; /* branch-and-bound node budget per cluster (default 1<<20 when <= 0) */
    double score_limit;   /* Tracker.scoreUpperLimit  (tracker.py:115) */
    double cnllr_limit;   /* Tracker.clnnrUpperLimit  (tracker.py:116) */
    double radar_x, radar_y, radar_range; /* Tracker.position / radarRange (tracker.py:44-45), range may be +inf */
    double merge_threshold; /* Tracker.mergeThreshold (tracker.py:65) used by initiateTarget */
} mht_forest_config;

/* ---- AIS-aided forest (Tracker.addMeasurementList(scanList, aisList), tracker.py:162, :394-396, :417-552) ---------------------
 * mht_forest_create_ex(..., MHT_FOREST_AIS): a forest whose nodes also carry the identity of the AIS message they were updated
 * with and the identity their track is bound to (pyTarget.py:34, :297-302) and whose ILP rows include the AIS messages
 * (tracker.py:1057-1064, :1083-1090).  4-state build, any n_scan a forest takes (<= 12).  Path records of two halves, radar rows and
 * AIS rows: n_scan <= 3: 8 entries (32 bytes), the ILPs stay in LDS; n_scan <= 7: 16 entries (64 bytes); n_scan >= 8: 32 entries
 * (128 bytes); from n_scan 4 on the ILPs run on the HBM policy.  mht_forest_set_ais hands over the messages of the NEXT scan, grouped as
 * for mht_fuse_ais; the next mht_forest_step / _step_host / _scan consumes them: radar M + nA <= max_meas (rounded up to a multiple
 * of 64).  A scan without messages needs no call.  Messages start tracks through the initiator (mht_initiator_set_ais).
 * Not available to members of a group.  The cluster-sharded step takes the messages (ABI 5): every shard makes the fused children itself.
 * mht_forest_read_mmsi: identities of the nodes [first, first + count) of the layer of `scan` (host arrays out, either may be null):
 * mmsi[i] = the message node first + i was updated with (0: none; with measurement number 0 that is a child WITHOUT a radar
 * measurement, the reference's measurementNumber None), hist[i] = Target._getHistoricalMmsi(). */
#define MHT_FOREST_AIS 1u
/* mht_forest_create_ex(..., MHT_FOREST_CT), six-state build (libmht_amd6.so) only: the constant-turn model BASELINE config 5 names
 * (pymht_amd/models/ct.py; state [x, y, vx, vy, w, a]).  The transition is not model->A but Phi(T, w) rebuilt for every hypothesis from its
 * own turn rate x[4], T = model->A[4][5] (give A = Phi(T, 0)); every leaf runs the reference's per-hypothesis form kalman.predict_single +
 * kalman.precalc on a batch of one (kalman.py:67-70, :82-101) -- what mht_gate_scan_x does with mht_model_x.transition = 1 -- and nothing
 * is shared by value: the forest keeps the children's covariances per node.  The device initiator starts tracks in it (as in any forest of
 * the six-state build) once its births are lifted (mht_initiator_set_lift); they begin on the straight-line branch of Phi(T, 0).  No groups. */
#define MHT_FOREST_CT 2u
int mht_forest_create_ex(mht_ctx* ctx, const mht_model* model, const struct mht_forest_config* cfg, uint32_t flags);
int mht_forest_set_ais(mht_ctx* ctx, const mht_ais_group* groups, int32_t nG, const mht_ais_msg* msgs, int32_t nA, double eta2_ais, double lambda_ais);
int mht_forest_read_mmsi(mht_ctx* ctx, int32_t scan, int32_t first, int32_t count, int32_t* mmsi, int32_t* hist);
/* the same for n given nodes of the layer (host array `nodes`; a node outside the layer gives 0): a gather on the device, for callers that
 * need a few scattered nodes -- e.g. the roots that join a track's committed history -- and not a whole layer (ABI 5) */
int mht_forest_read_mmsi_nodes(mht_ctx* ctx, int32_t scan, int32_t n, const int32_t* nodes, int32_t* mmsi, int32_t* hist);

/* per-target record of the scan report (old target-list order) */
typedef struct mht_target_report {
    int32_t id;         /* Target.ID */
    int32_t status;     /* 0 alive, 1 out of range, 2 score too high, 3 cNLLR too high (tracker.py:891-916) */
    int32_t sel_node;   /* index of the selected leaf (__trackNodes__[t]) in the layer of this scan */
    int32_t sel_meas;   /* its measurementNumber */
    int32_t new_index;  /* index in the target list after termination, -1 if terminated */
    int32_t root_scan;  /* scanNumber of the root after N-scan pruning */
    int32_t root_node;  /* node index of that root in its layer */
    int32_t n_leaves;   /* leaves kept for the next scan */
    double sel_x[MHT_NX];    /* state of the selected leaf */
    double sel_cnllr;   /* its cumulativeNLLR */
    double score;       /* getScore() = cNLLR - root.cNLLR before pruning (pyTarget.py:124) */
    double root_cnllr;  /* cumulativeNLLR of the root after pruning */
    double root_x[MHT_NX];   /* state of the root after pruning */
    int32_t root_meas;  /* measurementNumber of the root after pruning */
    int32_t cluster;    /* smallest target index of this target's cluster (tracker.py:961-974) */
} mht_target_report;

/* one target the device initiator gave birth to after the scan (mht_forest_initiate) */
typedef struct mht_birth_report {
    int32_t id;          /* Target.ID, or -1 if Tracker.initiateTarget discarded the candidate (too close to a current track) */
    int32_t meas;        /* measurementNumber: 1-based index among the scan's UNUSED measurements, 0 for a merged target */
    double x0[MHT_NX];   /* float32 values */
    float P0[MHT_NX * MHT_NX];
} mht_birth_report;

typedef struct mht_scan_report {
    int32_t scan;          /* scanNumber just processed */
    int32_t n_targets;     /* targets before termination (= number of records) */
    int32_t n_alive;
    int32_t n_leaves_in;   /* L: leaves gated in this scan */
    int32_t n_children;    /* L + G */
    int32_t n_leaves_out;  /* leaves kept for the next scan */
    int32_t n_clusters, n_ilp; /* clusters, clusters with >= 2 targets (Tracker.nOptimSolved) */
    int32_t n_branched;    /* ILPs that needed branch and bound */
    int32_t n_limit;       /* ILPs that hit the node limit (selection feasible, not proven optimal) */
    int32_t blp_iters_max;
    int32_t error;         /* 0 or MHT_E_CAPACITY if a pool overflowed during the scan */
    int32_t used_words;    /* number of valid words in `used` */
    int32_t n_births;      /* candidates of the device initiator after this scan (0 without mht_forest_initiate) */
    int32_t pad[2];
    /* device time of the scan's stages in 10 ns ticks of the GPU's wall clock, stamped by the kernels themselves (no HIP events, no
     * host cost): t_process = grow launch (tracker.py toc['Process']), t_cluster (toc['Cluster']), t_optim = similar-state pruning +
     * ILPs + termination / N-scan prune decisions (toc['Optim']), t_scan = start of the grow launch .. end of the last ILP workgroup */
    int32_t t_process, t_cluster, t_optim, t_scan;
    const uint64_t* used;              /* host: bit j set iff measurement j was gated by some leaf */
    const mht_target_report* targets;  /* host: n_targets records */
    const mht_birth_report* births;    /* host: n_births records */
} mht_scan_report;

int mht_forest_create(mht_ctx* ctx, const mht_model* model, const mht_forest_config* cfg);
/* Tracker.initiateTarget (tracker.py:147-160) for n candidates in order: a candidate closer than merge_threshold
 * to any current leaf (or to an earlier accepted candidate) is discarded when check_neighbours != 0.
 * x0 host [n][4] double, P0 host [n][16] float, flags host [n] uint8 (MHT_F_*), pd host [n] double,
 * meas host [n] int32 (measurementNumber of the new root), accepted host [n] uint8 out (may be NULL),
 * ids host [n] int32 out (assigned Target.ID or -1; may be NULL).  Synchronises when an output is requested. */
int mht_forest_add_targets(mht_ctx* ctx, int32_t n, const double* x0, const float* P0, const uint8_t* flags,
                           const double* pd, const int32_t* meas, int32_t check_neighbours, uint8_t* accepted,
                           int32_t* ids);
/* Same with every array in device memory (dev pointers, accepted/ids may be NULL); fully asynchronous -- used to
 * replay pre-staged births without a host round trip. */
int mht_forest_add_targets_dev(mht_ctx* ctx, int32_t n, const double* x0, const float* P0, const uint8_t* flags,
                               const double* pd, const int32_t* meas, int32_t check_neighbours, uint8_t* accepted,
                               int32_t* ids);
/* One scan, asynchronous: z dev (M,2) float32.  Two launches (grow with the clustering union-find, ILP + prune decisions; three with the
 * clustering kernel on similar-state pruning scans); the target-side commit
 * of the scan (compacted target table, next leaf ranges, the report) is deferred: it rides in the next step's first launch,
 * or runs as a launch of its own as soon as the report, new targets or an export are asked for.  Either order leaves the same
 * forest (tests/test_forest_edge_gpu.py).  */
int mht_forest_step(mht_ctx* ctx, const float* z, int32_t M);
/* Same with z in host memory (copied through a ring of pinned staging buffers of the ctx: asynchronous). */
int mht_forest_step_host(mht_ctx* ctx, const float* z_host, int32_t M);
/* Start the transfer of the last step's report into pinned host memory (runs the scan's commit first if it is still pending) and
 * return at once.  A host that issues the next step before it calls mht_forest_report overlaps its own work with the device's;
 * two transfers can be in flight.  Behind mht_forest_scan (whose report waits for a ride in the NEXT scan's grow launch) it sends
 * that report on its way now, in a launch of its own: what a host does that has no further scan to queue. */
int mht_forest_report_begin(mht_ctx* ctx);
/* Wait for the last step (or for the transfer mht_forest_report_begin started) and expose its report (pointers stay valid until
 * the next but one mht_forest_report_begin on this ctx). */
int mht_forest_report(mht_ctx* ctx, mht_scan_report* out);
/* The report whose transfer the last (which = 0) or the last but one (which = 1) mht_forest_report_begin started.
 * which = 2 (streaming with mht_forest_scan and an initiator only): the report of the scan TWO before the last one, while the last
 * scan's own report has not left the device yet -- a host that queues scan k before it folds the report of scan k - 2 never waits for
 * the device unless it is two scans ahead (MHT_E_STATE when that report is not in a host block any more). */
int mht_forest_report_get(mht_ctx* ctx, int32_t which, mht_scan_report* out);
/* Snapshot of the current leaves in target-list / DFS order (pyTarget.getLeafNodes order): any pointer may be
 * NULL.  x host [n][4], P host [n][16], cnllr host [n], meas/target/id/node host [n] int32, flags host [n] uint8.
 * capacity = length of the host arrays; *n_out = number of leaves.  Synchronises. */
int mht_forest_leaves(mht_ctx* ctx, int32_t capacity, double* x, float* P, double* cnllr, int32_t* meas,
                      int32_t* target, int32_t* id, int32_t* node, uint8_t* flags, int32_t* n_out);
/* The same with every covariance as float64, P host [n][16] double: the exact value of a float32 covariance, the reference's own float64
 * one where flags carries MHT_F_COV_F64 (a forest with AIS: Target.P_0 keeps the dtype the reference gives it, pyTarget.py:16-40).
 * mht_forest_leaves rounds those to float32. */
int mht_forest_leaves_f64(mht_ctx* ctx, int32_t capacity, double* x, double* P, double* cnllr, int32_t* meas,
                          int32_t* target, int32_t* id, int32_t* node, uint8_t* flags, int32_t* n_out);
/* The window rows of the current leaves, in mht_forest_leaves' order and with its capacity semantics: rows host [capacity][depth]
 * int32.  One thread per leaf walks `parent` from the leaf up to its target's window root (root_scan / root_node of the target table);
 * the root itself is left out unless it is the leaf.  Every node on the way with a measurement (meas > 0) gives one key
 * (level << 24) | meas, level = current scan - the node's scan; the other cells are -1.  These are the rows the reference's ILP gives
 * the leaf's column, so two leaves share a key exactly where they exclude each other.  The walk is bounded by depth and by the ring;
 * nothing else is launched, no forest state changes.  depth 1 .. 64.  A forest with MHT_FOREST_AIS: MHT_E_STATE (its columns also
 * carry message rows).  Synchronises. */
int mht_forest_leaf_rows(mht_ctx* ctx, int32_t capacity, int32_t depth, int32_t* rows, int32_t* n_out);
/* Similar-state pruning -- Tracker._pruneSimilarState (tracker.py:1233-1239) -> Target.pruneSimilarState (pyTarget.py:358-412),
 * what addMeasurementList(..., pruneSimilar=True) asks for (tracker.py:230-231) -- for the scans stepped from now on: in every target
 * that is alone in its cluster, the hit children of a node that lie within `threshold` metres (Tracker.pruneThreshold,
 * tracker.py:117) of its missed-detection child are replaced, together with that child, by one measurement-less hypothesis carrying
 * their mean state / covariance / cumulativeNLLR (NumPy's float32 / float64 arithmetic and summation order).  One extra launch
 * per scan between clustering and the ILPs (also for a member of a group stepped by mht_group_step).  threshold <= 0 switches it off.
 * With it on, n_leaves / n_leaves_out of the report count the slots of the surviving leaf ranges (emptied ones included);
 * n_leaves_in and mht_forest_leaves count hypotheses. */
int mht_forest_set_prune_similar(mht_ctx* ctx, double threshold);
/* Real-time guard for the global-hypothesis ILPs (_solveBLP_OR_TOOLS, tracker.py:1124-1217, has none: a giant cluster without
 * a dual certificate keeps CBC -- and this library's branch and bound -- busy for as long as it takes): a cluster whose
 * branch and bound has run for `milliseconds` of wall-clock time stops like one that reached blp_node_limit -- the best feasible
 * selection found so far is used, the scan's report counts it in n_limit and the report call returns MHT_E_LIMIT.  0 = no limit
 * (default).  For forests stepped by mht_group_step: set it before mht_group_create. */
int mht_forest_set_blp_time_limit(mht_ctx* ctx, double milliseconds);
/* Per-stage device time in milliseconds, SUMMED over the steps issued since the last call (at most 64 may be
 * pending): [0] grow kernel = the reference's toc['Process'], [1] cluster, [2] optimise (ILP + single-target selection,
 * incl. the per-target termination test / prune decision / surviving leaf ranges), [3] commit (target-table compaction,
 * next leaf ranges, report), [4] whole step.  *n_steps = number of steps summed.
 * Timing is off by default (five hipEventRecord per step); enable != 0 switches it on for subsequent steps.
 * Synchronises the stream. */
int mht_forest_set_timing(mht_ctx* ctx, int32_t enable);
int mht_forest_stage_times(mht_ctx* ctx, float* ms5, int32_t* n_steps);
/* Tooling: copy a named internal per-cluster array of the last step to the host ("cl_status", "cl_iters",
 * "cl_nodes", "cl_time" [2 int32 per cluster: setup / total in 10 ns ticks], "cl_ptr", "cl_members", "multi_list",
 * "single_list", "cl_counts", "cl_owner", "team_list", "tchild").  Synchronises. */
int mht_forest_debug_read(mht_ctx* ctx, const char* name, void* host, int64_t bytes);
/* Ancestor chain of one node: walks parents from (scan, node) towards the root of time, at most max_len steps
 * (bounded by the ring of n_scan + 4 layers: with k scans queued behind `scan`, n_scan + 4 - k layers are left).  Outputs host arrays
 * nodes/meas [max_len] int32, x [max_len][4], cnllr [max_len], P [max_len][16]; any may be NULL. */
int mht_forest_chain(mht_ctx* ctx, int32_t scan, int32_t node, int32_t max_len, int32_t* nodes, int32_t* meas,
                     double* x, double* cnllr, float* P, int32_t* n_out);
/* The same with float64 covariances (see mht_forest_leaves_f64) and the nodes' flag bytes, flags host [max_len] uint8 or NULL. */
int mht_forest_chain_f64(mht_ctx* ctx, int32_t scan, int32_t node, int32_t max_len, int32_t* nodes, int32_t* meas,
                         double* x, double* cnllr, double* P, uint8_t* flags, int32_t* n_out);

/* The streaming form (ABI 6; Tracker._apply_report: the window ancestors of the tracks a scan terminated, tracker.py:353-381 keeps them): the
 * chains of `count` nodes of layer `scan` are gathered by ONE launch queued behind what is already on the forest's stream, into a pinned
 * block of the library; nothing waits.  *ticket names the block; it stays valid until 8 later tickets have been issued.  f64 != 0:
 * float64 covariances as mht_forest_chain_f64.  mht_forest_chains_fetch waits for that launch only (not for scans queued behind it)
 * and copies chain `index` out: arrays as mht_forest_chain / _f64 (P: float32 or float64 [max_len][16] as asked at begin). */
int mht_forest_chains_begin(mht_ctx* ctx, int32_t scan, const int32_t* start_nodes, int32_t count, int32_t max_len, int32_t f64, int64_t* ticket);
int mht_forest_chains_fetch(mht_ctx* ctx, int64_t ticket, int32_t index, int32_t* nodes, int32_t* meas, double* x, double* cnllr, void* P,
                            uint8_t* flags, int32_t* n_out);

/* ---- step 7 of a scan: M-of-N track initiation on the device (tracker.py:264-278 -> initiators/m_of_n.py:215-478) -------------
 * What Tracker.__init__ hands to m_of_n.Initiator (tracker.py:66-72) plus the model constants the initiator imports (pv.P0, pv.Q's
 * sigmaQ, m_of_n.py:12-16 gamma = chi2(2).ppf(0.99)). */
typedef struct mht_initiator_config {
    int32_t m_required, n_checks;   /* Tracker.M_required / N_checks */
    int32_t max_meas;               /* measurements per scan */
    int32_t max_prelim;             /* preliminary tracks kept */
    int32_t max_born;               /* confirmed tracks per scan, before merging (behind a forest: at most 256, the report's capacity; more in a scan: MHT_E_CAPACITY) */
    double v_max;                   /* Tracker.maxSpeedMS */
    double gamma;                   /* gate of the preliminary tracks */
    double merge_threshold;         /* Tracker.mergeThreshold */
    double default_pd;
    float C[8], R[4], P0[16];       /* C_RADAR, R_RADAR(), pv.P0 */
    float sigma_q;                  /* scale of pv.Q */
} mht_initiator_config;
typedef struct mht_initiator mht_initiator;
int mht_initiator_create(mht_ctx* ctx, mht_initiator** out, const mht_initiator_config* cfg);
int mht_initiator_destroy(mht_initiator* in);
/* Initiator.processMeasurements (m_of_n.py:233-244) for one scan, asynchronous on the ctx stream: z dev (M,2) float32, the scan;
 * used dev [ceil(M/64)] uint64 or NULL: bit j set = measurement j was gated by a track and is not offered to the initiator
 * (tracker.py:266, MeasurementList.filterUnused); now = scan time stamp. */
int mht_initiator_step(mht_initiator* in, const float* z, int32_t M, const uint64_t* used, double now);
/* AIS messages for the initiator (Initiator.processMeasurements(radar, ais), m_of_n.py:233, :262-280): the messages of the scan it runs on
 * next, host array in LIST order (dT = time of the scan - time of the message); the ones no track took start preliminary tracks unless a
 * track with that identity exists or an existing one is too similar.  `used` (host, one byte per message) marks the taken ones for the
 * stand-alone mht_initiator_step; mht_forest_scan works them out itself (tracker.py:267-270: the identities still in an association set
 * behind the scan's pruning) and then runs the initiator behind the scan instead of next to the clustering. */
typedef struct mht_ais_init_msg { double state[4]; double dT; int32_t mmsi; int32_t pad; } mht_ais_init_msg;
int mht_initiator_set_ais(mht_initiator* in, const mht_ais_init_msg* msgs, int32_t nA, const uint8_t* used);
/* The targets the last step gave birth to (host arrays, any may be NULL): x0 [n][4] (float32 values), P0 [n][16],
 * meas [n] measurementNumber (1-based index among the UNUSED measurements, 0 for a merged target) -- and the sizes of the
 * initiator's lists.  Synchronises. */
int mht_initiator_born(mht_initiator* in, int32_t capacity, double* x0, float* P0, int32_t* meas, int32_t* n_born,
                       int32_t* n_prelim, int32_t* n_seeds);
/* Six-state build only: the births of this 4-state initiator enter a forest behind mht_forest_initiate / mht_forest_scan LIFTED into its
 * state space, x0 [x, y, vx, vy] (float32 values) and P0 (4 x 4) becoming
 *     x = [x0, x_tail[0], x_tail[1]],   P = [[P0, 0], [0, P_tail]]   (P_tail 2 x 2 row-major, the cross blocks exactly 0)
 * -- in the forest's layers, its root covariances and the report's mht_birth_report rows.  nx must be 6.  The initiator itself (its
 * preliminary tracks, gates, assignments, merging, mht_initiator_born's x0 [n][4] / P0 [n][16]) is unchanged.  Without this call the
 * six-state build refuses an initiator in mht_forest_initiate / mht_forest_scan; the 4-state build refuses the call (MHT_E_INVALID). */
int mht_initiator_set_lift(mht_initiator* in, int32_t nx, const float* x_tail, const float* P_tail);

/* Step 7 behind a forest step, on the stream, no host round trip: runs the scan's commit, offers the scan's unused measurements
 * (tracker.py:266) to the initiator and hands its confirmed candidates to Tracker.initiateTarget's device twin
 * (mht_forest_add_targets_dev, neighbour test included).  z / M: the scan just stepped (z = NULL: the copy mht_forest_step_host
 * staged); now: its time stamp.  The candidates and
 * their fate appear in the report of that scan (mht_scan_report::births).  The initiator must have been created on the same ctx. */
int mht_forest_initiate(mht_ctx* ctx, mht_initiator* in, const float* z, int32_t M, double now);

/* ---- one tracker on several devices: the independent per-cluster ILPs (tracker.py:228-236) are spread --------------------------------
 * Every device holds the same forest and is fed the same scans and births; the multi-target clusters are placed by size -- longest
 * processing time first on their column counts, each to the least loaded device; every device computes the same table from the same
 * data (cluster kernel: cl_owner) --, a single-target cluster goes to device (target index % shard_n).  sel_rel: dev [max_targets] int32 owned by the caller; after _begin it holds, for the targets whose
 * cluster this device solved, the selected child's ordinal inside the target's block, -1 elsewhere.  The caller combines the
 * devices' arrays with an element-wise MAX (all-reduce over RCCL) and calls _end, which finishes the scan for all targets.
 * Asynchronous on the ctx stream. */
int mht_forest_step_sharded_begin(mht_ctx* ctx, const float* z, int32_t M, int32_t shard_n, int32_t shard_i, int32_t* sel_rel);
int mht_forest_step_sharded_end(mht_ctx* ctx, const int32_t* sel_rel);
/* (ABI 6) A gating graph that is ONE big component on several devices (tracker.py:1155-1217 is one CBC call; any exact split will do): with an
 * exchange block of mht_forest_sharded_words() int32 -- [max_targets] selections as above, then [shard_n][8][260] files -- the clusters of
 * >= 24 targets (at most 8 per scan) are searched by ALL devices: the subtrees of the branch and bound are dealt out over every device's
 * workgroups, every device files its best selection and its value in its own slots (-1 = empty), the SAME element-wise MAX all-reduce over
 * the whole block gathers the files, and mht_forest_step_sharded_end (given the block) lets the smallest value win -- on every device alike. */
int mht_forest_sharded_words(mht_ctx* ctx, int32_t shard_n, int32_t* n_words);
int mht_forest_step_sharded_begin2(mht_ctx* ctx, const float* z, int32_t M, int32_t shard_n, int32_t shard_i, int32_t* xch, int32_t n_words);

/* One radar scan of Tracker.addMeasurementList (tracker.py:162-307) in one call, nothing waits for the device: steps 1-6
 * (mht_forest_step_host), step 7 (mht_forest_initiate, skipped when `in` is NULL), mht_forest_report_begin.
 * With an initiator the scans are STREAMED: the scan's commit, the admission of what its initiator gave birth to and the report's push ride
 * in the next scan's grow launch (which starts while this scan's ILP launch is still running); the initiator is a one-workgroup launch on a
 * side stream of the forest's; the report is complete in its pinned host block when the words the pushing workgroups post there say so
 * (mht_forest_report_get waits for them, not for an event).  mht_synchronize also waits for the side stream. */
int mht_forest_scan(mht_ctx* ctx, mht_initiator* in, const float* z_host, int32_t M, double now);

/* ---- a group of independent sectors on one device (BASELINE config 4: four sensor sectors = four independent Tracker
 * instances, pymht/tracker.py:39-137; nothing in tracker.py:162-307 couples two Tracker objects) -------------------------------
 * The members' forests step TOGETHER with one launch per stage (grow, cluster, ILP) for the whole group: a single sector is a
 * chain of dependent round trips that leaves most of the GPU idle, S sectors cost about one such chain.  Results are exactly
 * those of stepping every member with mht_forest_step (tests/test_sectors_gpu.py).
 *   ctxs   n contexts (1 <= n <= 32) that own a forest each; same device, same stream, same forest configuration
 *   z      host array of n device pointers, z[i] = member i's scan, dev (M[i],2) float32
 *   M      host array of n measurement counts
 * After a group step every per-forest call (mht_forest_report, _add_targets*, _leaves, ...) works on the members as usual. */
typedef struct mht_group mht_group;
int mht_group_create(mht_group** out, int32_t n, mht_ctx* const* ctxs);
int mht_group_step(mht_group* g, const float* const* z, const int32_t* M);
int mht_group_destroy(mht_group* g);

#ifdef __cplusplus
}
#endif
#endif /* MHT_AMD_H */
