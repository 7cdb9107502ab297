/*
 * movba.h — C-ABI of the MI355X-native local bundle adjustment (libmovba.so).
 *
 * Drop-in boundary for MoV-SLAM's optimizer hot path.  The reference has no FFI: the
 * boundary is the static-method surface of class MOV_SLAM::Optimizer
 * (/root/reference/include/Optimizer.h:45-60).  An adapter with those exact signatures
 * (mov-slam_amd/host/Optimizer.cc) flattens the KeyFrame/MapPoint graph into the plain
 * arrays below and calls these entry points; everything from "arrays in" to
 * "poses / points / chi2 / outlier list out" — what the reference delegates to
 * g2o at src/Optimizer.cc:754-755 plus the gate at :757-804 — runs in hand-written
 * HIP kernels for gfx950.  No Eigen / Sophus / g2o / OpenCV / torch types cross this
 * boundary: plain pointers and sizes only.
 *
 * Threading: a handle is bound to one device + one stream and must be used by one
 * thread at a time; different handles are independent (LocalMapping thread and
 * Tracking thread each own one, reference src/System.cc:128-129).
 * Ownership: the caller owns every buffer; the library keeps no caller pointer
 * after a call returns (the stop flag is read only during the call).
 * Errors: int status, never throws / exits; on non-zero status nothing was written
 * to the result buffers except `status` (reference convention of silent early
 * returns, src/Optimizer.cc:525-529, 749-751).
 */
#ifndef MOVBA_H
#define MOVBA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOVBA_VERSION 5

/* status codes */
#define MOVBA_OK              0
#define MOVBA_STOPPED         1   /* *stop was set before the solve (Optimizer.cc:749-751)   */
#define MOVBA_NO_FIXED        2   /* no fixed keyframe vertex (Optimizer.cc:525-529)          */
#define MOVBA_EMPTY           3   /* nothing to optimise (no edges / no free vertex)          */
#define MOVBA_SINGULAR        4   /* the information matrix (plus damping) is not positive definite: nothing written */
#define MOVBA_ERR_ARG        -1
#define MOVBA_ERR_HIP        -2   /* HIP runtime failure (no device, OOM, launch error)       */
#define MOVBA_ERR_STATE      -3   /* call order violated (run before upload, ...)             */
#define MOVBA_ERR_DEVICE_WAIT -4  /* a workgroup gave up a bounded wait inside a launch (20 ms) in the FIRST attempt of a run
                                     AND in its repeat on the paths that do not wait inside launches: never seen.  The usual
                                     outcome of a given-up wait is MOVBA_OK with n_sync_timeouts > 0 (movba_lba_run solves the
                                     window again, see movba_lba_result); results are never handed out from a failed attempt */
#define MOVBA_ERR_TOO_LARGE  -5   /* the window's reduced system exceeds what the direct solver can hold             */
/* Free keyframes per window: <= 80 the on-chip PCG (where the reduced matrix fits its registers), <= 432 the one-launch
 * direct solver, beyond that one launch per block column; the solution vector of the latter's back substitution lives in
 * LDS (48 doubles per 8 keyframes beside 28 KB of work space: 159 KB at 2 700 keyframes). */
#define MOVBA_MAX_FREE_KEYFRAMES 2700

/* flags */
#define MOVBA_FLAG_STALE_ERROR_QUIRK 1u  /* chi2 of a rejected last trial, as g2o leaves it */

typedef struct movba_handle movba_handle;

/* One flattened local-BA window.  Replaces the g2o graph the reference builds at
 * src/Optimizer.cc:532-747 (vertices :554-584, :623-632; mono edges :646-672). */
typedef struct {
    int32_t n_poses;            /* K + F keyframe vertices, ascending KeyFrame::mnId          */
    int32_t n_points;           /* P map-point vertices                                       */
    int32_t n_edges;            /* E monocular edges, caller order = vpEdgesMono order        */
    const double  *poses;       /* n_poses x 7: qx qy qz qw tx ty tz = Tcw (Optimizer.cc:559) */
    const uint8_t *pose_fixed;  /* n_poses: 1 = setFixed(true) (Optimizer.cc:561, 578)        */
    const double  *points;      /* n_points x 3 world position (Optimizer.cc:627)             */
    const int32_t *edge_pose;   /* E: index into poses   (vertex 1 of the edge, :655)         */
    const int32_t *edge_point;  /* E: index into points  (vertex 0 of the edge, :654)         */
    const double  *obs;         /* E x 2: mvKeysUn[idx].pt (Optimizer.cc:648-650)             */
    const double  *inv_sigma2;  /* E: information = inv_sigma2 * I2 (Optimizer.cc:656-657)    */
    double fx, fy, cx, cy;      /* GeometricCamera::getParameter(0..3), float -> double       */
    double huber_delta;         /* (double)sqrtf(5.0f) (Optimizer.cc:616); <= 0: no kernel    */
    double chi2_gate;           /* 5.0 (Optimizer.cc:52, 769)                                 */
    int32_t max_iters;          /* optimizer.optimize(10) (Optimizer.cc:755)                  */
    int32_t max_trials;         /* g2o maxTrialsAfterFailure (default-constructed LM, :539); 0 -> 10 */
    uint32_t flags;             /* MOVBA_FLAG_*                                               */
    const volatile uint8_t *stop; /* pbStopFlag (Optimizer.cc:544-545, 749), may be NULL      */
    /* stereo observations (g2o::EdgeStereoSE3ProjectXYZ, Optimizer.cc:673-705): obs_right[e] >= 0 is
     * mvuRight[idx] of a stereo observation (third residual u_r - (u - bf/z)); < 0 or NULL: monocular */
    const double  *obs_right;   /* E or NULL                                                  */
    double bf;                  /* KeyFrame::mbf (Optimizer.cc:695)                           */
    /* intrinsics by keyframe: the reference gives every edge the camera of ITS keyframe (e->pCamera = pKFi->mpCamera,
     * Optimizer.cc:664; e->fx .. e->bf = pKFi->fx .. pKFi->mbf, :690-695).  NULL (every shipped MoV-SLAM configuration has
     * one camera): fx, fy, cx, cy / bf above hold for every keyframe.  Either may be given without the other.        */
    const double  *cam_kf;      /* n_poses x 4 (fx fy cx cy) or NULL                          */
    const double  *bf_kf;       /* n_poses or NULL                                            */
} movba_lba_desc;

#define MOVBA_MAX_TRACE 128

typedef struct {
    double  *poses;             /* n_poses x 7 out (fixed vertices returned unchanged)        */
    double  *points;            /* n_points x 3 out                                           */
    double  *chi2;              /* E out, caller edge order: e->chi2() (Optimizer.cc:769)     */
    uint8_t *outlier;           /* E out: chi2 > gate || !isDepthPositive() (Optimizer.cc:769)*/
    int32_t status;
    int32_t iters_done;         /* outer LM iterations run                                    */
    int32_t n_solves;           /* linear solves = accepted + rejected trials                 */
    int32_t n_outliers;
    int32_t pcg_iters;          /* total PCG iterations over all solves                       */
    int32_t last_rejected;      /* 1 if the final trial was rejected                          */
    double lambda;              /* final damping                                              */
    double cost0, cost;         /* initial / final robust cost (activeRobustChi2)             */
    int32_t n_trace;            /* per-trial trace (min(n_solves, MOVBA_MAX_TRACE) entries)   */
    double  tr_lambda[MOVBA_MAX_TRACE];
    double  tr_f0[MOVBA_MAX_TRACE];
    double  tr_f1[MOVBA_MAX_TRACE];
    double  tr_rho[MOVBA_MAX_TRACE];
    int32_t tr_accept[MOVBA_MAX_TRACE];
    int32_t tr_pcg_iters[MOVBA_MAX_TRACE];   /* PCG iterations of the trial; -1: solved by the dense direct solver; -2: by the
                                                banded factorisation                                                          */
    /* Reduced solve (LinearSolverCSparse in the reference, Optimizer.cc:535): banded Cholesky in one workgroup for the
     * windows it solves fastest (up to ~24 free keyframes at a band of 9), on-chip PCG for windows of up to 80 free
     * keyframes whose reduced matrix fits the PCG workgroup's registers, dense Cholesky otherwise (more keyframes, or
     * denser covisibility) and from the first trial on which one of the other two handed the solve over. */
    int32_t n_direct;           /* trials solved by the dense direct solver                                    */
    int32_t direct_from;        /* n_solves at the switch to the dense direct solver (0: whole solve; > 0: the PCG gave up or
                                   the banded factorisation met a non-positive pivot on that trial), -1: never */
    int32_t n_chol_fail;        /* trials whose factorisation failed (dense solver: non-positive pivot; banded: NaN / inf in
                                   the normal equations): booked as the oracle books them, nothing moved, rejected unless the
                                   current cost is infinite (mov-slam_amd/csrc/lm_rule.h; not g2o's own booking) */
    int32_t n_pcg_giveups;      /* 0 or 1: hand-overs of the solve to the dense direct solver - the PCG gave up (breakdown or
                                   iteration cap), or the banded factorisation met a finite non-positive pivot (the name is
                                   from when only the PCG could hand over)                                      */
    int32_t n_sync_timeouts;    /* waits inside a launch that a workgroup gave up (one-launch direct solver without all its
                                   workgroups resident): > 0 with status MOVBA_OK = the run was repeated with the multi-launch
                                   direct solver and THIS is its result (the reference never skips a solve,
                                   src/Optimizer.cc:535, 754)                                                                   */
    int32_t n_band;             /* trials solved by the single-workgroup banded factorisation (exact, one launch)  */
} movba_lba_result;

/* Solver options (all have defaults; pass NULL to movba_create for defaults). */
typedef struct {
    double pcg_rel_tol;         /* stop when sqrt(r.z / r0.z0) <= tol       (default 1e-10)   */
    int32_t pcg_max_iters;      /* per solve; reaching it hands the trial to the direct solver (default 200) */
    int32_t run_ahead;          /* trial sets the host keeps queued ahead    (default 2)       */
    int32_t profile;            /* bit k set: bracket launches of kernel class k (see movba_profile)
                                 * with HIP events on the handle's stream; 0x3f = all          */
    int32_t pcg_coarse;         /* 0 = default (two-level: block-Jacobi + aggregate coarse level),
                                 * -1 = block-Jacobi only                                       */
    int32_t host_wait;          /* how the calling thread waits for the device between queueing trials:
                                 * 0 = spin on the progress word (default, lowest latency), 1 = sched_yield() between
                                 * looks (for a LocalMapping thread that shares its core with Tracking; the upload's helper
                                 * thread then sleeps between uploads instead of staying awake for 4 ms after each)    */
    int32_t pcg_spill;          /* 1 = keep the PCG for windows whose reduced matrix does not fit the PCG workgroup's registers
                                 * (list tails read from an L2 copy every iteration); 0 = default: such windows take the
                                 * one-launch direct solver from the first trial                                        */
    int32_t solver;             /* 0 = default, 1 = the dense direct solver for every window, 2 = the banded factorisation in one workgroup
                                   where the window's band fits LDS (else as 0), 3 = never the banded factorisation (PCG where it fits,
                                   dense direct solver elsewhere)                                                                    */
    int32_t reorder;            /* 0 = default: free keyframes are renumbered by covisibility (reverse Cuthill-McKee on the pair
                                 * graph) when that shrinks the reduced matrix's envelope by a fifth or more; -1 = keep the
                                 * caller's order (KeyFrame::mnId order, as the reference numbers its vertices)             */
    int32_t pad_o;              /* (keeps the struct a multiple of 8 bytes; until ABI 4 the opt-in two-stream LM loop, removed in
                                 * round 5: measured 1 - 3 % slower on MI355X than the one-stream loop)                  */
} movba_options;

/* Per-kernel-class timing collected with HIP events on the handle's stream. */
#define MOVBA_NKERNELS 6
typedef struct {
    const char *name[MOVBA_NKERNELS];
    double      ms[MOVBA_NKERNELS];      /* summed device time                               */
    int64_t     launches[MOVBA_NKERNELS];
    double      upload_ms, structure_ms, download_ms;   /* host-side phases, wall clock     */
} movba_profile;

int  movba_version(void);
const char *movba_status_string(int status);

/* device: HIP device ordinal.  stream: a hipStream_t created by the caller on that device
 * (e.g. torch.cuda.current_stream().cuda_stream) or NULL for a private stream. */
int  movba_create(movba_handle **out, int device, void *stream, const movba_options *opt);
void movba_destroy(movba_handle *h);

/* Optimizer::LocalBundleAdjustment's solve (Optimizer.cc:754-755 + :757-775) in one call:
 * upload + run + download.  Also serves Optimizer::BundleAdjustment (Optimizer.cc:286-287). */
int  movba_lba_solve(movba_handle *h, const movba_lba_desc *desc, movba_lba_result *res);

/* The same in three phases, for callers that keep the window resident in HBM
 * (the window can be re-run after movba_lba_reset).  desc->stop is the one caller pointer the
 * phased API keeps: from movba_lba_upload until the next upload / solve on the handle, read by
 * every movba_lba_run in between; it must stay valid that long (or be NULL).  A raised flag
 * makes that run return MOVBA_STOPPED; the next run looks at the flag again. */
int  movba_lba_upload(movba_handle *h, const movba_lba_desc *desc);   /* host structure + H2D */
int  movba_lba_reset(movba_handle *h);                                /* restore uploaded state on device */
int  movba_lba_run(movba_handle *h);                                  /* LM loop on device; returns after stream sync */
int  movba_lba_download(movba_handle *h, movba_lba_result *res);      /* D2H + caller edge order */

/* Marginal covariances of the window's last movba_lba_run / movba_lba_solve (status MOVBA_OK only; also after
 * movba_lba_run_batch), at the estimate movba_lba_download returns - what g2o's SparseOptimizer::computeMarginals, Ceres'
 * Covariance and GTSAM's Marginals give.
 *   pose_cov   n_poses x 36, caller order: the row-major 6 x 6 block of keyframe i over the left tangent [omega; upsilon] of Tcw,
 *              the update VertexSE3Expmap::oplusImpl applies (T <- exp(delta) T)
 *   point_cov  n_points x 9: the row-major 3 x 3 block of map point l, world coordinates
 * Either may be NULL, not both.  Definition: H is the full normal matrix of the window at the returned estimate as g2o's
 * buildSystem and the LM kernels build it - every edge, inliers and gated outliers alike, stereo edges with their third row,
 * the camera of each edge's keyframe, information rho'(chi2) inv_sigma2 I (Huber; no kernel when huber_delta <= 0) - with
 * `damping` added to every diagonal entry.  The pose block of free keyframe i is the (i, i) block of H^-1, i.e. of S^-1 with
 * S = Hpp - Hpl Hll^-1 Hlp; the point block of l is D + D (sum over its free observers i, j of B_il^T Sigma_ij B_jl) D with
 * D = (Hll_l + damping I)^-1, B_il the 6 x 3 Hpl block of edge (i, l) and Sigma_ij the (i, j) block of S^-1.  Fixed keyframes
 * get zero blocks (they fix the gauge); free keyframes and map points without an edge are not in the system: NaN blocks.
 * Every block is exactly symmetric, and two calls give the same bits.
 * Monocular windows with fewer than two fixed keyframes leave the scale free: H is singular, and at damping = 0 the call
 * returns MOVBA_SINGULAR or values dominated by rounding - damp such windows (e.g. 1e-3).
 * Returns MOVBA_ERR_ARG (NULL handle, both outputs NULL, damping negative or not finite), MOVBA_ERR_STATE (no upload, no run
 * since the upload / reset, or a run whose status was not MOVBA_OK), MOVBA_SINGULAR (a non-positive or non-finite pivot in the
 * factorisation of S, or a map point whose Hll + damping I is not positive definite).  On any non-zero status nothing is
 * written.  The window, its results and later runs are left exactly as they were.  (Not g2o's computeMarginals to the bit: that
 * one reuses the damped Hessian from before the last update.) */
int  movba_lba_marginals(movba_handle *h, double damping, double *pose_cov, double *point_cov);

/* movba_lba_run on the resident windows of n handles at once (multi-session serving: several independent windows on one
 * GPU): every kernel of an LM trial is one launch over the concatenated windows, with per-window LM state, so each window
 * takes exactly the steps of its solo run and returns bit-identical results; download each handle as usual.  The handles
 * must have been created on the same device and the same stream, and hold either stereo or monocular windows.  Windows
 * that end before the solve (MOVBA_EMPTY / MOVBA_NO_FIXED / stop flag up) report that through their own download.
 * The windows run in two groups half a trial out of phase; the second group's launches go to the device's COPY stream,
 * which every handle's upload also uses (one stream per device for all handles: each further stream of the process
 * competes for the few hardware queues).  Results never depend on it (tested with another handle uploading and solving
 * meanwhile), but an upload on ANOTHER handle of the device queues behind the running batch, and its copies between the
 * second group's kernels cost the batch its out-of-phase schedule for that trial: for the quoted batch throughput, upload
 * the windows first, then run.  Windows without an on-chip PCG are run one by one behind the batched launches. */
int  movba_lba_run_batch(movba_handle *const *handles, int32_t n);

/* Copy the optimised poses (n_poses x 7 f64) into a caller-owned DEVICE buffer on the
 * handle's stream — what the RCCL all-gather of independent windows sends. */
int  movba_lba_export_poses_device(movba_handle *h, void *dst_device, int64_t capacity_bytes);
/* The same without a copy of its own: register a DEVICE buffer once and every later movba_lba_run leaves
 * the optimised poses in it (written by the solve's last kernel; valid when movba_lba_run returns).
 * NULL unregisters.  The buffer must stay allocated while it is registered. */
int  movba_lba_set_pose_export(movba_handle *h, void *dst_device, int64_t capacity_bytes);

/* Pinned, device-visible host memory for result arrays (optional).  When `poses`, `points` or `chi2` of the
 * movba_lba_result handed to movba_lba_solve point into a block obtained here, the solve's last kernel writes those
 * results straight into them across the bus; otherwise they arrive in the handle's staging buffer and are copied out by
 * the calling thread.  (g2o's own results are in place too: vertex->estimate() is read after optimize(),
 * /root/reference/src/Optimizer.cc:822-838.)  Ordinary host memory for the CPU: read, write and keep it as long as
 * needed; release it with movba_host_free.  Returns NULL when no device is available or the allocation fails. */
void *movba_host_alloc(size_t bytes);
void  movba_host_free(void *p);

int  movba_get_profile(movba_handle *h, movba_profile *out);
int  movba_reset_profile(movba_handle *h);
int  movba_set_profile_mask(movba_handle *h, int32_t mask);

/* Host-only structure pass (no GPU needed): what movba_lba_upload derives from a window
 * before any H2D copy.  Exposed for the CPU test suite. */
typedef struct {
    int32_t n_free;             /* free AND active pose vertices (hessian blocks)            */
    int32_t n_pairs;            /* upper-triangle pose pairs sharing >= 1 point               */
    int64_t n_entries;          /* sum over points of d(d+1)/2 over free observers            */
    int32_t n_items;            /* schur work items (pair chunks)                             */
    int32_t max_degree;         /* max edges per point                                        */
    int32_t already_grouped;    /* 1 if caller edges were already grouped by point            */
    int32_t pcg_on_chip;        /* 1: reduced matrix stays in VGPRs during the PCG (k_pcg_rows) */
    int32_t pcg_overflow;       /* 1: some gather-list tails are read from an L2 copy          */
    int32_t pcg_max_wave_entries; /* largest number of gather entries dealt to one wave       */
    int32_t n_row_entries;      /* gather-list entries incl. padding                          */
    int32_t n_sched_slots;      /* slots of the schur launch schedule (8 XCD segments)        */
    int32_t sched_items;        /* work items found in the schedule (must equal n_items)      */
    int32_t sched_max_permille; /* heaviest XCD segment / mean segment weight, x1000          */
    int32_t slots_ok;           /* pose-major edge slots are a bijection onto 0..E_free-1     */
    int32_t reordered;          /* 1: the free keyframes were renumbered by covisibility (free_index is the new numbering) */
    int32_t pad_s;
} movba_structure_info;
int  movba_structure_probe(const movba_lba_desc *desc, movba_structure_info *info,
                           int32_t *edge_perm /* E or NULL */, int32_t *free_index /* n_poses or NULL */);

/* Host only (no device needed): the static schedule of the one-launch direct solver that stands in for the reference's
 * LinearSolverCSparse factorisation (Optimizer.cc:535) for a reduced system of n_block_cols 48-wide block columns — for
 * tests, which replay it against its own flags.  info[0..3] = supported, workgroups, tile slots per workgroup, tasks;
 * task_ptr (workgroups + 1) and tasks (8 int32 each: op, slot, I, K, k, 0, 0, 0) are filled up to their capacities. */
int  movba_dense_plan_probe(int32_t n_block_cols, int32_t max_groups, int32_t max_slots, int32_t info[4],
                            int32_t *task_ptr, int32_t task_ptr_cap, int32_t *tasks, int32_t tasks_cap);

/* Pose-only optimisation behind Optimizer::PoseOptimization (Optimizer.cc:397-459), over the
 * reference's EdgeSE3ProjectXYZOnlyPose (include/OptimizableTypes.h:30-58). */
typedef struct {
    int32_t n;                  /* 2D-3D matches (Frame::N non-null, Optimizer.cc:404-413)    */
    const double *Xw;           /* n x 3 MapPoint::GetWorldPos                                */
    const double *obs;          /* n x 2 mvKeys[i].pt                                         */
    const double *inv_sigma2;   /* n or NULL (= 1)                                            */
    double fx, fy, cx, cy;
    double pose0[7];            /* initial Tcw                                                */
    double huber_delta;         /* reprojection threshold in px                               */
    double chi2_gate;           /* threshold^2                                                */
    int32_t rounds;             /* 4                                                          */
    int32_t its_per_round;      /* 10                                                         */
    /* Hypothesis stage in front of the LM, so that the result does not depend on pose0 (the reference calls
     * cv::solvePnPRansac with useExtrinsicGuess = false, Optimizer.cc:437): ransac_iters minimal P3P samples
     * (iterationCount of PoseOptimization, 50 by default), drawn from ransac_seed; every candidate pose is scored on
     * all matches by MAGSAC++'s sigma-consensus loss (flag 38 = cv::USAC_MAGSAC, Optimizer.cc:437; sigma_max from
     * chi2_gate: pose_kernels.hip) and the one of lowest loss among those with at least 4 matches inside chi2_gate starts
     * the LM.  0: LM from pose0. */
    int32_t ransac_iters;       /* <= MOVBA_MAX_RANSAC_ITERS                                  */
    uint32_t ransac_seed;
    /* `confidence` of cv::solvePnPRansac (Optimizer.cc:437; 0.95 in TartanAir.yaml): the standard stopping rule
     * N = log(1 - confidence) / log(1 - w^3), w = inlier ratio of the best hypothesis so far.  The device scores all
     * ransac_iters samples at once; the rule decides which of them a sequential RANSAC over the same samples would have
     * drawn: only those are eligible (ransac_samples_used in the result).  <= 0 or >= 1: all samples are eligible.
     * lo_iters > 0: one local-optimisation step on the winner (USAC's LO): an LM refit weighted by the sigma-consensus
     * weights w(r) (lo_iters iterations), kept when its sigma-consensus loss is lower.
     * rounds x its_per_round: the motion-only LM with re-classification behind the hypothesis stage is ORB-SLAM's
     * PoseOptimization scheme (4 x 10); MoV-SLAM's own PoseOptimization (Optimizer.cc:397-459) takes solvePnPRansac's pose
     * as it is - rounds = 0 gives exactly that. */
    double  confidence;
    int32_t lo_iters;
    int32_t pad_p;
} movba_pose_desc;

#define MOVBA_MAX_RANSAC_ITERS 256

typedef struct {
    double   pose[7];
    uint8_t *outlier;           /* n out (Frame::mvbOutlier, Optimizer.cc:452-456)            */
    double  *chi2;              /* n out or NULL                                              */
    int32_t  n_inliers;         /* return value of PoseOptimization (Optimizer.cc:458)        */
    int32_t  status;
    int32_t  ransac_inliers;    /* inliers of the best hypothesis (0: stage off, or no candidate with >= 4)  */
    int32_t  lm_iters;          /* LM iterations run over the 4 rounds (g2o stops a round early when the cost stops changing) */
    double   ransac_pose[7];    /* the pose the LM started from                               */
    int32_t  ransac_samples_used;   /* minimal samples the stopping rule admitted (<= ransac_iters)                  */
    int32_t  lo_accepted;       /* 1: the local-optimisation refit replaced the winning hypothesis                   */
    int32_t  lo_inliers;        /* inliers of the pose the LM started from, at chi2_gate (after the LO step)          */
    int32_t  pad_q;
} movba_pose_result;

int  movba_pose_opt(movba_handle *h, const movba_pose_desc *desc, movba_pose_result *res);
#define MOVBA_MAX_POSE_BATCH 1024
/* movba_pose_opt on n frames at once (several Tracking sessions on one GPU): one set of launches, one synchronisation.
 * Every frame's result equals, bit for bit, what movba_pose_opt returns for the same descriptor.  Every descriptor is
 * checked first: one invalid descriptor (as movba_pose_opt rejects it), n < 0, n > MOVBA_MAX_POSE_BATCH or a NULL pointer
 * gives MOVBA_ERR_ARG and nothing is solved.  n == 0: MOVBA_OK.  A frame with fewer than 4 matches gets status MOVBA_EMPTY
 * and pose0, the others are still solved, and the call returns MOVBA_OK; results[i].status holds each frame's outcome.
 * Uses the handle's staging buffer and pose scratch like movba_pose_opt (waits for an uploaded window's arrays first).
 * Frames of more than ~3 000 matches (beyond what a workgroup keeps in LDS) go to a second launch. */
int  movba_pose_opt_batch(movba_handle *h, const movba_pose_desc *descs, movba_pose_result *results, int32_t n);
/* The minimal samples movba_pose_opt draws for (n matches, n_hyp, seed): n_hyp x 3 distinct match indices.  Host only. */
int  movba_pose_ransac_samples(int32_t n, int32_t n_hyp, uint32_t seed, int32_t *out);

/* The numeric body of LocalMapping::CreateNewMapPoints (LocalMapping.cc:313-476) for many keyframe pairs at once: every
 * match of every pair is triangulated (or un-projected from a stereo observation) and taken through the reference's gates
 * in the reference's order.  Choosing the neighbours (the baseline test at :268-287 with ComputeSceneMedianDepth included:
 * a neighbour the reference skips is simply not passed), matching (MOVMatcher::SearchForTriangulation, :292) and the MapPoint
 * bookkeeping (:483-494) stay with the caller (the matching is movba_track_match, whose output has this call's layout).  Pairs are independent: one call serves one keyframe against its 30
 * neighbours, or the keyframes of many sessions. */
typedef struct {
    /* views */
    int32_t n_views;
    int32_t n_pairs;
    const double  *poses;       /* n_views x 7: qx qy qz qw tx ty tz = Tcw, as movba_lba_desc::poses (KeyFrame::GetPose, :237, :294);
                                   the quaternion is normalised before use                                                */
    const double  *cam;         /* n_views x 4: fx fy cx cy (KeyFrame::fx .. cy, :244-247, :302-305)                      */
    const double  *bf;          /* n_views or NULL (monocular): KeyFrame::mbf (:430, :456)                                */
    const double  *b;           /* n_views or NULL (monocular): KeyFrame::mb (:346, :348)                                 */
    /* pairs: view 1 = the current keyframe (mpCurrentKeyFrame), view 2 = the neighbour (pKF2, :265) */
    const int32_t *pair_view;   /* n_pairs x 2: indices into the views                                                    */
    const int32_t *pair_ptr;    /* n_pairs + 1: ascending prefix into the matches, pair_ptr[0] = 0 (vMatchedIndices, :289-310) */
    /* matches: n_matches = pair_ptr[n_pairs], those of pair p are [pair_ptr[p], pair_ptr[p + 1]) */
    const double  *obs1;        /* n_matches x 2: kp1.pt in view 1, pixels (:318-320)                                     */
    const double  *obs2;        /* n_matches x 2: kp2.pt in view 2 (:326-328)                                             */
    const double  *ur1;         /* n_matches or NULL: mvuRight[idx1] (:321); < 0 or NULL: monocular observation (:322)    */
    const double  *ur2;         /* n_matches or NULL: mvuRight[idx2] (:330-331)                                           */
    const double  *depth1;      /* n_matches (required with ur1): mvDepth[idx1] (:346, KeyFrame::UnprojectStereo)         */
    const double  *depth2;      /* n_matches (required with ur2): mvDepth[idx2] (:348)                                    */
    /* gates */
    double reproj_gate;         /* bound of the SQUARED reprojection error: the reference's delta = 5 (LocalMapping.cc:28, :422) */
    double far_threshold;       /* mThFarPoints (:477); <= 0: off (mbFarPoints false)                                     */
} movba_tri_desc;

/* code[m]: what happened to match m, in the order the reference tests it (each reject is one of its `continue`s) */
#define MOVBA_TRI_DLT            1   /* accepted: null vector of the 4 x 4 DLT system (:363-377)                         */
#define MOVBA_TRI_STEREO1        2   /* accepted: un-projected from view 1's stereo depth (:378-383)                     */
#define MOVBA_TRI_STEREO2        3   /* accepted: un-projected from view 2's stereo depth (:384-389)                     */
#define MOVBA_TRI_REJ_W0        16   /* homogeneous w == 0 (:369-372)                                                    */
#define MOVBA_TRI_REJ_PARALLAX  17   /* a stereo observation, but neither stereo parallax below the other (:390-393)     */
#define MOVBA_TRI_REJ_DEPTH     18   /* non-positive stereo depth: UnprojectStereo false (:395-396)                      */
#define MOVBA_TRI_REJ_BEHIND1   19   /* z1 <= 0 (:399-403)                                                               */
#define MOVBA_TRI_REJ_BEHIND2   20   /* z2 <= 0 (:405-409)                                                               */
#define MOVBA_TRI_REJ_REPROJ1   21   /* squared reprojection error in view 1 > reproj_gate (mono :416-426, stereo :427-437) */
#define MOVBA_TRI_REJ_REPROJ2   22   /* ... in view 2 (mono :443-452, stereo :453-463)                                   */
#define MOVBA_TRI_REJ_ZERO_DIST 23   /* the point lies in a camera centre (:472-475)                                     */
#define MOVBA_TRI_REJ_FAR       24   /* a distance >= far_threshold (:477-480)                                           */

typedef struct {
    double  *points;            /* n_matches x 3 out, world (x3D, :483): written for every match that reached a 3-D position
                                   (accepted, or rejected from MOVBA_TRI_REJ_BEHIND1 on), NaN for the three rejects before it */
    uint8_t *code;              /* n_matches out: MOVBA_TRI_*                                                             */
    int32_t  n_accepted;        /* matches with an accepted code (the reference's cnt, :490)                              */
    int32_t  status;
} movba_tri_result;

/* Restated exactly, quirks included:
 *   - rays R1^T xn1, R2^T xn2 over the normalised coordinates ((u - cx) / fx, (v - cy) / fy, 1) and cosParallaxRays (:334-339);
 *   - the stereo parallaxes as the `if / else if` at :345-348 leaves them: cos(2 atan2(b / 2, depth)) for view 1 when its
 *     observation is stereo, for view 2 ONLY when view 1's is not; the other keeps cosParallaxRays + 1;
 *   - no stereo observation: DLT rows x P[2] - P[0], y P[2] - P[1] of both views with P = [Rcw | tcw], null vector, division
 *     by w (cv::triangulatePoints, :365-376); a stereo observation: the view with the smaller parallax cosine is un-projected
 *     (:378-389), (u - cx) depth / fx, (v - cy) depth / fy, depth taken to the world;
 *   - the stereo reprojection in view 2 subtracts VIEW 1's bf over z2 (:456), as the reference does;
 *   - comparisons as written (z <= 0, error > gate, distance == 0, distance >= threshold): a NaN passes them as it does there.
 * The reference computes in float32 around a double SVD; this call is fp64 from the boundary to the result (as the LBA,
 * DESIGN.md section 6), so its decisions can differ from the reference's only for matches within float rounding of a gate.
 * The null vector comes from a one-sided Jacobi iteration on the 4 x 4 system itself (not on its normal matrix), with a fixed
 * maximum of sweeps: the result of a match depends on that match and its two views alone - not on the other matches, the
 * order or number of pairs, or how a set of matches is split over calls - and two calls give the same bits.
 * Returns MOVBA_ERR_ARG (NULL handle / descriptor / result, a negative count, a NULL array that the counts make necessary,
 * pair_ptr not ascending or not starting at 0, a view index out of range, ur1 / ur2 without bf and b or without its depth
 * array, reproj_gate not finite, far_threshold NaN), MOVBA_ERR_HIP as elsewhere; every argument is checked before anything
 * is queued, and on a non-zero status nothing is written except `status`.  No matches: MOVBA_OK, n_accepted = 0, nothing else
 * written.  One packed copy to the device, one kernel launch, one synchronisation; `points` and `code` that lie in
 * movba_host_alloc memory are written by the kernel itself.  May share a handle with an uploaded or solved window (it waits
 * for the window's arrays before reusing the staging buffer): the window, its results and later runs stay as they were. */
int  movba_triangulate(movba_handle *h, const movba_tri_desc *desc, movba_tri_result *res);

/* Monocular map initialisation: the numeric body of TwoViewReconstruction::Reconstruct (TwoViewReconstruction.cc:68-118, called
 * from Tracking.cc:620 through Pinhole::ReconstructWithTwoViews, Pinhole.cpp:90-100) for n independent frame pairs per call -
 * cv::findEssentialMat(USAC_MAGSAC), cv::recoverPose and CheckRT.  One session's attempt is n = 1; a process that serves many
 * sessions hands all of them to one set of launches. */
typedef struct {
    int32_t n_matches;          /* matches of the pair: the caller compacts vMatches12 >= 0 (TwoViewReconstruction.cc:54-63)     */
    int32_t ransac_iters;       /* minimal samples scored, 1 .. MOVBA_MAX_TWO_VIEW_ITERS                                       */
    const double *obs1;         /* n_matches x 2, pixels: mvKeys1[mvMatches12[i].first].pt (:81)                                */
    const double *obs2;         /* n_matches x 2: mvKeys2[mvMatches12[i].second].pt (:82)                                       */
    double fx, fy, cx, cy;      /* mK (:85-87)                                                                                  */
    double threshold;           /* 1.0: findEssentialMat's threshold in pixels (:89)                                            */
    double confidence;          /* 0.999 (:89); <= 0 or >= 1: every sample is eligible                                          */
    double sigma;               /* 1.0: CheckRT's th2 = 4 sigma^2 (:110)                                                        */
    double min_parallax_deg;    /* 1.0 (:41, :112)                                                                              */
    double max_depth;           /* 50: cv::recoverPose's distance bound in the overload the reference calls (:94)               */
    int32_t min_triangulated;   /* 50 (:65, :92)                                                                                */
    uint32_t ransac_seed;
} movba_two_view_desc;

#define MOVBA_MAX_TWO_VIEW_ITERS 1024   /* (confidence 0.999 at half the matches wrong asks for 218 samples: MOVBA_MAX_RANSAC_ITERS is too few) */
#define MOVBA_MAX_TWO_VIEW_BATCH 1024
/* matches per pair at most: k_tv_check selects the parallax cosine by counting ranks, n^2 / 256 comparisons per thread of the
 * pair's one workgroup (4 million at this bound, a few milliseconds); a frame holds a few thousand keypoints */
#define MOVBA_MAX_TWO_VIEW_MATCHES 32768

/* outcome: MOVBA_TV_OK, or the `return false` of Reconstruct that was taken */
#define MOVBA_TV_OK            0
#define MOVBA_TV_NO_MODEL      1   /* no candidate, or no match within the threshold: n == 0 (:91); also pairs under 5 matches */
#define MOVBA_TV_FEW_GOOD      2   /* pass < minGood = max((int)(0.75 n), min_triangulated) (:92-99)                           */
#define MOVBA_TV_LOW_PARALLAX  3   /* !(parallax > minParallax) (:112-117)                                                     */

/* code[m]: what CheckRT did with match m (each reject is one of its `continue`s, in its order) */
#define MOVBA_TV_CHK_NONE           0   /* CheckRT was not reached (MOVBA_TV_NO_MODEL)                                         */
#define MOVBA_TV_CHK_GOOD           1   /* accepted (counted in nGood, point written) and vbGood: cosParallax < 0.99998 (:230) */
#define MOVBA_TV_CHK_LOW_PARALLAX   2   /* accepted, but not vbGood                                                            */
#define MOVBA_TV_CHK_REJ_NOT_INLIER 16  /* not in the mask after recoverPose (:163)                                            */
#define MOVBA_TV_CHK_REJ_W0         17  /* homogeneous w == 0 (:179)                                                           */
#define MOVBA_TV_CHK_REJ_BEHIND1    18  /* z1 <= 0 and cosParallax < 0.99998 (:195)                                            */
#define MOVBA_TV_CHK_REJ_BEHIND2    19  /* z2 <= 0 and cosParallax < 0.99998 (:201)                                            */
#define MOVBA_TV_CHK_REJ_REPROJ1    20  /* squared reprojection error in image 1 > th2 (:212)                                  */
#define MOVBA_TV_CHK_REJ_REPROJ2    21  /* ... in image 2 (:223)                                                               */

typedef struct {
    double   pose[7];           /* T21: qx qy qz qw tx ty tz, |t| = 1 (:114); identity without a model                         */
    double   E[9];              /* the winning essential matrix, row-major, Frobenius norm sqrt 2 (:89)                        */
    double   parallax_deg;      /* CheckRT's parallax (:234-242)                                                               */
    int32_t  outcome;           /* MOVBA_TV_*                                                                                  */
    int32_t  status;            /* MOVBA_OK; MOVBA_EMPTY: fewer than 5 matches (outcome MOVBA_TV_NO_MODEL, no array written)   */
    int32_t  n_inliers;         /* n = countNonZero(mask) after findEssentialMat (:90)                                         */
    int32_t  n_pass;            /* recoverPose's return (:94)                                                                  */
    int32_t  n_good;            /* CheckRT's return nGood (:244; the reference computes it and does not use it, :110)          */
    int32_t  samples_used;      /* minimal samples the stopping rule admitted                                                  */
    uint8_t *inlier;            /* n_matches out: the mask after recoverPose (:104-108)                                        */
    double  *points;            /* n_matches x 3 out, camera-1 frame (vP3D, :227): NaN where CheckRT wrote none                */
    uint8_t *good;              /* n_matches out: vbGood = vbTriangulated (:230-231)                                           */
    uint8_t *code;              /* n_matches out: MOVBA_TV_CHK_*                                                               */
    /* the hypothesis stage, each NULL or caller memory (what tests compare solver against solver) */
    int32_t *hyp_nsol;          /* ransac_iters: candidates of every sample                                                    */
    double  *hyp_E;             /* ransac_iters x 10 x 9: the candidates (zeros behind a sample's last)                        */
    double  *hyp_loss;          /* ransac_iters x 10: their sigma-consensus++ loss over all matches (infinity behind the last) */
} movba_two_view_result;

/* OpenCV's own text is neither in the reference nor available to this project (as for cv::solvePnPRansac):
 * stages 1 - 3 restate the PUBLISHED algorithms by the rules below and do not claim OpenCV's bits; stage 4 is the reference's
 * own text and is restated exactly, quirks included.  fp64 from the boundary to the result.
 *  1. Hypotheses.  Pixels are normalised with ONE focal length f = 0.5 (fx + fy) and (cx, cy): the reference hands
 *     findEssentialMat and recoverPose that, not K (:85-89, :94); only CheckRT sees fx and fy apart.  Sample h = five distinct
 *     matches (movba_two_view_samples).  Five-point relative pose (Nister 2004): null space of the 5 x 9 epipolar system, the ten
 *     cubic constraints, elimination to a degree-10 polynomial in z, REAL roots only (derivative chain + bisection + Newton with
 *     a fixed work bound on [-1, 1]; |z| > 1 through the reversed polynomial in 1 / z), back-substitution: up to 10 candidates.
 *  2. Score.  Every candidate on all matches: squared Sampson distance in pixels, sigma-consensus++ loss (MAGSAC++, as
 *     movba_pose_opt) with gate threshold^2.  Winner: lowest loss among the samples the stopping rule admits, N = log(1 -
 *     confidence) / log(1 - w^5) with w the inlier ratio of the best candidate so far; ties go to the lower (sample, root) index.
 *     inlier0[m] = Sampson^2 <= threshold^2, n_inliers = their number.  movba_two_view does not refit the winner;
 *     movba_two_view_lo (below) does: stage 2b.
 *  2b. (movba_two_view_lo with lo_iters > 0 only.)  Local optimisation of the winner E0: iteratively reweighted Gauss-Newton with the
 *     sigma-consensus++ weights of ALL matches (MAGSAC++'s refit; restated by these rules, not OpenCV's bits).  Start: (R, t) of
 *     E0's decomposition, of its two rotations the one with the larger trace (the first on equal traces), t with the
 *     sign that makes <[t]x R, E0> >= 0 (the iterates do not depend on it beyond rounding).  Parameters: E = [t]x R,
 *     |t| = 1; a step (d omega, d tau) is R <- exp([d omega]x) R, t <- normalise(t + d tau_1 b1 + d tau_2 b2) with b1 = normalise(t x e_k),
 *     k the index of the smallest |t_k| (the lowest on a tie), b2 = t x b1.  Residual: the SIGNED Sampson distance in pixels, its
 *     1 x 5 Jacobian exact.  Pass k = 0 .. lo_iters over all matches at iterate k: L_k = sum of the losses (gate threshold^2; iterate 0
 *     is E0 itself); for k < lo_iters, H = sum w J J^T, g = sum w J r, step -H^-1 g by Cholesky without damping; a pivot that is not
 *     positive and finite ends the refit.  Kept: the iterate with the lowest L_k, the lowest k on a tie - so loss <= loss0 - handed
 *     out as [t]x R with the sign that makes <E, E0> >= 0, or as E0 itself, bit for bit, for k = 0.  inlier0, n_inliers and stages
 *     3 and 4 then run on the kept E; samples_used and the hypothesis tables stay those of stages 1 and 2.
 *  3. Pose recovery.  SVD of E (one-sided Jacobi), the four (R, t) with det R = +1; for each, every inlier0 match is triangulated
 *     linearly over [I | 0], [R | t] in f-normalised coordinates and counted when 0 < z1 < max_depth and 0 < z2 < max_depth; the
 *     largest count wins, ties in the order (R1, t), (R2, t), (R1, -t), (R2, -t).  n_pass = that count, inlier = inlier0 AND the test.
 *  4. CheckRT (:120-245): P1 = K [I | 0], P2 = K [R | t] in pixels with the true fx, fy; DLT rows x P[2] - P[0], y P[2] - P[1];
 *     w == 0 skips; cosParallax; the two depth tests that only reject when cosParallax < 0.99998; the two squared reprojection
 *     errors against th2 = 4 sigma^2 with `>`; nGood, vbGood = cosParallax < 0.99998; the sorted cosines' element min(50, size - 1)
 *     in degrees, 0 when nGood == 0; comparisons as written, so a NaN passes them as it does there.  (The reference computes
 *     this stage in float32.)  CheckRT is also run when the outcome is MOVBA_TV_FEW_GOOD - the reference has returned by then -
 *     so that a caller can see why an attempt failed; per-match arrays are written for every pair of 5 matches or more.
 * Conventions as movba_pose_opt_batch and movba_triangulate: every descriptor is checked before anything is queued; a NULL
 * pointer, n < 0, n > MOVBA_MAX_TWO_VIEW_BATCH or one invalid descriptor (n_matches negative or above MOVBA_MAX_TWO_VIEW_MATCHES; a NULL array that n_matches makes
 * necessary; ransac_iters outside 1 .. MOVBA_MAX_TWO_VIEW_ITERS; fx, fy not positive and finite; any other parameter not finite;
 * threshold or max_depth not positive; sigma or min_triangulated negative) gives MOVBA_ERR_ARG and nothing is written except
 * `status`.  n == 0: MOVBA_OK.  A pair under 5 matches gets status MOVBA_EMPTY; the others are still solved and the call
 * returns MOVBA_OK.  One packed copy to the device, three launches (k_tv_hyp, k_tv_recover, k_tv_check) over all pairs, one
 * synchronisation; per-match arrays in movba_host_alloc memory are written by the kernels themselves.  A pair's result does
 * not depend on the other pairs of the call or on their order, and two calls give the same bits.  May share a handle with an
 * uploaded or solved window: the window, its results and later runs stay as they were. */
int  movba_two_view(movba_handle *h, const movba_two_view_desc *descs, movba_two_view_result *results, int32_t n);
/* The minimal samples movba_two_view draws for (n_matches >= 5, n_hyp, seed): n_hyp x 5 distinct match indices, from the
 * generator of movba_pose_ransac_samples on another stream.  Host only. */
int  movba_two_view_samples(int32_t n_matches, int32_t n_hyp, uint32_t seed, int32_t *out);

/* movba_two_view with the local optimisation of the winner (stage 2b above): what cv::USAC_MAGSAC does with its best model and
 * movba_pose_opt does with lo_iters.  10 steps is the setting examined in DESIGN.md. */
#define MOVBA_MAX_TWO_VIEW_LO_ITERS 32
typedef struct {
    double  loss0;        /* sigma-consensus++ loss (sum over the pair's matches, as hyp_loss) of the minimal-sample winner     */
    double  loss;         /* ... of the iterate that was kept: loss <= loss0                                                   */
    double  E0[9];        /* the minimal-sample winner: bit for bit what movba_two_view returns as E                           */
    int32_t kept;         /* 0: the winner itself was kept; k: the iterate after k steps                                       */
    int32_t steps;        /* steps taken, <= lo_iters (fewer: the 5 x 5 system was not positive definite or not finite)        */
    int32_t n_inliers0;   /* matches within threshold of E0: movba_two_view's n_inliers                                        */
    int32_t pad;
} movba_two_view_lo_info;   /* 104 bytes */
/* Conventions, checks, statuses, batch limit, pinned result memory and handle sharing as movba_two_view, which is this call with
 * lo_iters = 0 and info = NULL.  lo_iters outside 0 .. MOVBA_MAX_TWO_VIEW_LO_ITERS: MOVBA_ERR_ARG, nothing written except
 * `status`.  lo_iters == 0: the results of movba_two_view bit for bit, info[i] = { loss0, loss0, E, 0, 0, n_inliers }.  info: n
 * entries or NULL; a pair without a model (MOVBA_TV_NO_MODEL, MOVBA_EMPTY) gets a zeroed entry.  One launch more than
 * movba_two_view (k_tv_lo, one workgroup per pair, between k_tv_hyp and k_tv_recover) when lo_iters > 0, and one small copy
 * back before the synchronisation.  No floating-point atomics: a pair's result, `info` included, does not depend on the other
 * pairs or their order, and two calls give the same bits. */
int  movba_two_view_lo(movba_handle *h, const movba_two_view_desc *descs, movba_two_view_result *results, int32_t n,
                       int32_t lo_iters, movba_two_view_lo_info *info /* n, or NULL */);

/* The second half of the monocular start: the numeric body of Tracking::CreateInitialMapMonocular (Tracking.cc:641-748) behind
 * movba_two_view / movba_two_view_lo, for n independent frame pairs per call - Optimizer::GlobalBundleAdjustemnt(map, 20) over
 * the two keyframes (:688, Optimizer.cc:68-395), ComputeSceneMedianDepth(2) of the first (:690, KeyFrame.cc:757-791), the
 * acceptance test (:694) and the rescaling of the baseline and of every point to median depth 1 (:702-717).  Building the
 * KeyFrame / MapPoint objects stays with the caller. */
typedef struct {
    int32_t n_matches;            /* matches of the pair, as handed to movba_two_view: 0 .. MOVBA_MAX_TWO_VIEW_MATCHES               */
    int32_t max_iters;            /* 20 (Tracking.cc:688); 0 .. MOVBA_MAX_INIT_MAP_ITERS; 0: no optimisation, stages 3 and 4 only     */
    int32_t max_trials;           /* g2o maxTrialsAfterFailure; 0 -> 10                                                            */
    int32_t min_tracked;          /* 50 (Tracking.cc:694)                                                                          */
    const double  *obs1;          /* n_matches x 2, pixels: the observation in keyframe 1                                          */
    const double  *obs2;          /* n_matches x 2: ... in keyframe 2                                                              */
    const double  *points;        /* n_matches x 3: mvIniP3D, in the frame of camera 1 = the world frame (Tracking.cc:631)         */
    const uint8_t *use;           /* n_matches or NULL (all): non-zero = the match was triangulated (Tracking.cc:622-629):
                                     movba_two_view_result::good as it is.  obs1, obs2, points, inv_sigma2_* of a match that is not
                                     used may hold anything, NaN included: they do not reach the result                             */
    const double  *inv_sigma2_1;  /* n_matches or NULL (= 1): mvInvLevelSigma2 of the keypoint's octave (Optimizer.cc:181-182)     */
    const double  *inv_sigma2_2;  /* n_matches or NULL (= 1)                                                                       */
    double pose2[7];              /* T21: qx qy qz qw tx ty tz, as movba_two_view returns it; the quaternion is normalised first   */
    double fx, fy, cx, cy;
    double huber_delta;           /* (double)sqrtf(5.0f) (Optimizer.cc:52, 138); <= 0: no kernel (bRobust false)                    */
} movba_init_map_desc;

#define MOVBA_MAX_INIT_MAP_ITERS 100

/* outcome: what the test at Tracking.cc:694 said */
#define MOVBA_IM_OK            0
#define MOVBA_IM_NEG_DEPTH     1   /* medianDepth < 0                                                                              */
#define MOVBA_IM_FEW_TRACKED   2   /* TrackedMapPoints(1) < min_tracked (= n_used: nothing was culled); also a pair without a used match */

typedef struct {
    double   pose[7];           /* T21 after the bundle adjustment; MOVBA_IM_OK: translation times 1 / median_depth (:702-704)      */
    double  *points;            /* n_matches x 3 out: the optimised points, MOVBA_IM_OK: times 1 / median_depth (:707-717); NaN for
                                   matches that are not used                                                                      */
    double  *chi2;              /* n_matches x 2 out or NULL: e->chi2() of the edge in keyframe 1 and in keyframe 2 at the returned
                                   estimate (before the rescaling, which does not change them); NaN for matches that are not used  */
    double   median_depth;      /* ComputeSceneMedianDepth(2) of keyframe 1 after the bundle adjustment (NaN: MOVBA_EMPTY)          */
    double   lambda;            /* final damping                                                                                  */
    double   cost0, cost;       /* robust cost (activeRobustChi2) at the start and at the returned estimate                       */
    int32_t  outcome;           /* MOVBA_IM_*                                                                                      */
    int32_t  status;            /* MOVBA_OK; MOVBA_EMPTY: no used match (pose = pose2 normalised, no array written)                */
    int32_t  n_used;            /* used matches = map points created (Tracking.cc:665-684)                                         */
    int32_t  iters_done;        /* outer LM iterations run                                                                         */
    int32_t  n_solves;          /* linear solves = accepted + rejected trials                                                      */
    int32_t  last_rejected;     /* 1 if the final trial was rejected                                                               */
    int32_t  n_chol_fail;       /* trials whose 6 x 6 factorisation met a pivot that is not positive and finite: rejected          */
    int32_t  pad;
} movba_init_map_result;

/* the per-trial trace of one pair: movba_lba_result's n_trace / tr_* (min(n_solves, MOVBA_MAX_TRACE) entries) */
typedef struct {
    int32_t n_trace, pad;
    double  tr_lambda[MOVBA_MAX_TRACE];
    double  tr_f0[MOVBA_MAX_TRACE];
    double  tr_f1[MOVBA_MAX_TRACE];
    double  tr_rho[MOVBA_MAX_TRACE];
    int32_t tr_accept[MOVBA_MAX_TRACE];
} movba_init_map_trace;

/* fp64 from the boundary to the result.  One workgroup per pair (k_init_map), the whole Levenberg-Marquardt loop inside one launch.
 *  1. The graph (BundleAdjustment's for this map, Optimizer.cc:121-282).  Keyframe 1 fixed at the identity (Tracking gives the
 *     initial frame the identity pose), keyframe 2 free at pose2.  One point vertex per USED match, in ascending match order,
 *     with two monocular edges: keyframe 1 first, then keyframe 2; information inv_sigma2 I, Huber kernel with huber_delta on
 *     every edge, all points marginalised.  There is no outlier gate: BundleAdjustment erases nothing at nLoopKF == 0.
 *  2. The optimisation: g2o's Levenberg-Marquardt as movba_lba_solve runs it, max_iters outer iterations.
 *     lambda0 = 1e-5 max |H_jj| over the pose block and every point block; lambda is added to the pose and the point diagonals
 *     before the Schur complement; the reduced system - one 6 x 6 block, Hpp + lambda I - sum over the points of Hpl (Hll +
 *     lambda I)^-1 Hpl^T with Hpl of the keyframe-2 edge - is solved by Cholesky; the points follow by back substitution; pose
 *     update T <- exp(delta) T, point update X <- X + delta; rho = (F0 - F1) / (sum x (lambda x + b) + 1e-3); accept (rho > 0
 *     and F1 finite): lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), nu = 2; reject: lambda *= nu, nu *= 2, the estimates
 *     are restored; up to max_trials trials per iteration while rho < 0; the run ends (Terminate) after an iteration that used
 *     max_trials trials, met rho == 0 or a lambda that is not finite.  A failed factorisation is a rejected trial with F1 =
 *     DBL_MAX, counted in n_chol_fail.  cost and chi2 are evaluated at the returned estimate (the oracle with
 *     stale_error_quirk off).  Sums over the points run in a fixed tree over the workgroup: no floating-point atomics.
 *  3. Median depth: z = third coordinate of the optimised points (camera 1 is the world frame); the median is element
 *     (n_used - 1) / 2 of their ascending order (KeyFrame.cc:788-790 with q = 2), found exactly by counting ranks (ties by match
 *     order; a NaN sorts by its bit pattern, above every number when positive).  The reference's depths are float.
 *  4. Outcome, as written at Tracking.cc:694: MOVBA_IM_NEG_DEPTH when median_depth < 0, else MOVBA_IM_FEW_TRACKED when n_used <
 *     min_tracked, else MOVBA_IM_OK.  MOVBA_IM_OK: the translation of `pose` and every point are multiplied by 1 / median_depth
 *     (:702-714); a median of exactly 0 passes the test as it does there and gives values that are not finite.  The other
 *     outcomes return the unscaled estimate of the bundle adjustment, so that a caller can see what was rejected.
 *  5. The result of a pair depends on its used matches and their order alone - not on the matches that are not used, the
 *     other pairs of the call or their order: the same pair handed over compacted (use == NULL) or spread out under a mask
 *     gives the same bits in the used slots, and two calls give the same bits.
 * max_iters == 0: stages 3 and 4 on the points as given, n_solves = 0, cost0 = cost = the robust cost of the input.
 * trace: n entries or NULL; a pair with status MOVBA_EMPTY gets n_trace = 0.
 * Conventions as movba_two_view: every descriptor is checked before anything is queued; a NULL handle, n < 0, n >
 * MOVBA_MAX_TWO_VIEW_BATCH, NULL descs or results with n > 0, or one invalid descriptor (n_matches negative or above
 * MOVBA_MAX_TWO_VIEW_MATCHES; obs1, obs2, points or the result's points NULL with n_matches > 0; max_iters outside 0 ..
 * MOVBA_MAX_INIT_MAP_ITERS; max_trials or min_tracked negative; fx, fy not positive and finite; cx, cy, huber_delta or an entry
 * of pose2 not finite; a pose2 whose quaternion is zero) gives MOVBA_ERR_ARG and nothing is written except `status`.  n == 0:
 * MOVBA_OK.  A pair without a used match gets status MOVBA_EMPTY; the others are still solved and the call returns MOVBA_OK.
 * One packed copy to the device, one launch, one synchronisation; `points` and `chi2` that lie in movba_host_alloc memory
 * are written by the kernel itself.  May share a handle with an uploaded or solved window: the window, its results and later
 * runs stay as they were. */
int  movba_init_map(movba_handle *h, const movba_init_map_desc *descs, movba_init_map_result *results, int32_t n,
                    movba_init_map_trace *trace /* n, or NULL */);

/* The per-point visibility arithmetic between the poses this library returns and the next set of matches it is given (matching
 * in this fork is by track id, not by descriptor), for many frames and keyframes per call: Frame::isInFrustum over the local
 * map points of a tracked frame (Frame.cc:456-519, from Tracking::SearchLocalPoints, Tracking.cc:1134-1152), the gates at the
 * head of MOVMatcher::Fuse (MOVMatcher.h:207-245, from LocalMapping::SearchInNeighbors, LocalMapping.cc:558, :586) and
 * KeyFrame::ComputeSceneMedianDepth (KeyFrame.cc:757-791), which feeds the baseline test in front of triangulation
 * (LocalMapping.cc:268-287).  A view is one frame or keyframe with one list of map points in one mode; a keyframe that needs
 * two lists appears as two views.  The mnLastFrameSeen and isBad filters, IncreaseVisible, the track-id lookup (movba_track_match), Replace and
 * AddObservation, the far-points test on track_depth and the division baseline / median_depth stay with the caller. */
#define MOVBA_VIEW_FRUSTUM 0   /* Frame.cc:464-518, the monocular branch (this fork's frames have Nleft == -1)          */
#define MOVBA_VIEW_FUSE    1   /* MOVMatcher.h:207-245                                                                  */
#define MOVBA_VIEW_DEPTH   2   /* KeyFrame.cc:775-790: z only, then the median                                          */
#define MOVBA_MAX_VIEW_BATCH 4096

typedef struct {
    /* the point table, shared by all views */
    int32_t n_points;
    int32_t n_views;
    const double  *points;          /* n_points x 3, world (MapPoint::GetWorldPos)                                         */
    const double  *normals;         /* n_points x 3 (MapPoint::GetNormal); may be NULL when every view is a DEPTH view      */
    const double  *max_distance;    /* n_points: the raw mfMaxDistance - the 1.2 of GetMaxDistanceInvariance is applied here;
                                       NULL as normals                                                                     */
    const double  *min_distance;    /* n_points: the raw mfMinDistance (0.8 applied here); NULL as normals                 */
    /* views: every array has one entry per view */
    const int32_t *mode;            /* MOVBA_VIEW_*                                                                        */
    const double  *poses;           /* x 7: qx qy qz qw tx ty tz = Tcw, as movba_lba_desc::poses; the quaternion is normalised
                                       before use; the camera centre is Ow = -Rcw^T tcw, computed from the pose            */
    const double  *cam;             /* x 4: fx fy cx cy (pinhole)                                                          */
    const double  *bf;              /* x 1, or NULL: 0 (Frame::mbf, :512)                                                  */
    const double  *bounds;          /* x 4: mnMinX mnMaxX mnMinY mnMaxY; NULL when every view is a DEPTH view              */
    const double  *log_scale_factor;/* x 1: mfLogScaleFactor (MapPoint::PredictScale); NULL without a FRUSTUM view         */
    const int32_t *n_levels;        /* x 1: mnScaleLevels; NULL without a FRUSTUM view                                     */
    const double  *cos_limit;       /* x 1: viewingCosLimit, 0.5 at Tracking.cc:1143; NULL without a FRUSTUM view.  FUSE
                                       views use the reference's literal 0.5 * dist3D and ignore it                        */
    const int32_t *q;               /* x 1: the divisor of ComputeSceneMedianDepth, 2 at both call sites; NULL without a
                                       DEPTH view                                                                          */
    /* items: n_items = view_ptr[n_views], those of view v are [view_ptr[v], view_ptr[v + 1]) */
    const int32_t *view_ptr;        /* n_views + 1: ascending prefix, view_ptr[0] = 0                                      */
    const int32_t *item_point;      /* n_items: indices into the point table                                               */
} movba_view_desc;      /* 128 bytes */

/* code[i]: what happened to item i, in the order the reference tests it (each reject is one of its returns / `continue`s) */
#define MOVBA_VP_VISIBLE         1   /* FRUSTUM: isInFrustum returned true (:518)                                         */
#define MOVBA_VP_FUSE_CANDIDATE  2   /* FUSE: every gate in front of the keypoint loop passed (MOVMatcher.h:245)           */
#define MOVBA_VP_DEPTH_ITEM      3   /* DEPTH: the item's z is in the view's list                                          */
#define MOVBA_VP_REJ_BEHIND     16   /* z < 0 (Frame.cc:474, MOVMatcher.h:211)                                             */
#define MOVBA_VP_REJ_U          17   /* FRUSTUM: u < minX || u > maxX (:479)                                               */
#define MOVBA_VP_REJ_V          18   /* FRUSTUM: v < minY || v > maxY (:481)                                               */
#define MOVBA_VP_REJ_IMAGE      19   /* FUSE: !(u >= minX && u < maxX && v >= minY && v < maxY) (KeyFrame.cc:735)          */
#define MOVBA_VP_REJ_DIST       20   /* dist < 0.8 min_distance || dist > 1.2 max_distance (Frame.cc:493, MOVMatcher.h:231) */
#define MOVBA_VP_REJ_ANGLE      21   /* FRUSTUM: PO.Pn / dist < cos_limit (:501); FUSE: PO.Pn < 0.5 dist (:240)            */

typedef struct {
    uint8_t *code;              /* n_items out: MOVBA_VP_* (required when n_items > 0)                                     */
    /* per item, each NULL or n_items entries; NaN (level: -1) where the reference had not computed the value when it returned */
    double  *z;                 /* third camera coordinate: every item of every mode                                       */
    double  *uv;                /* x 2, the pinhole projection: FRUSTUM and FUSE items from the depth test passed on        */
    double  *dist;              /* |P - Ow|: FRUSTUM and FUSE items from the bounds passed on                              */
    double  *view_cos;          /* PO.Pn / dist: FRUSTUM items from the distance gate passed on                            */
    int32_t *level;             /* nPredictedLevel: accepted FRUSTUM items                                                 */
    double  *ur;                /* u - bf / z (mTrackProjXR): accepted FRUSTUM items                                       */
    double  *track_depth;       /* |Pc| (mTrackDepth): accepted FRUSTUM items                                              */
    /* per view (required when n_views > 0) */
    int32_t *n_accepted;        /* n_views out: items with an accepted code - FRUSTUM: the reference's nToMatch (Tracking.cc:1146),
                                   FUSE: the candidates, DEPTH: the length of the list                                     */
    double  *median_depth;      /* n_views out: DEPTH views; NaN for the others                                            */
    int32_t  status;
    int32_t  pad;
} movba_view_result;    /* 88 bytes */

/* Restated as written, item by item:
 *   FRUSTUM  Pc = Rcw P + tcw; z = Pc_z < 0 rejects; u = fx x / z + cx, v = fy y / z + cy; u < minX || u > maxX rejects, then the
 *            same for v; dist = |P - Ow|; dist < 0.8 min_distance || dist > 1.2 max_distance rejects; view_cos = PO.Pn / dist <
 *            cos_limit rejects; level = ceil(log(max_distance / dist) / log_scale_factor) clamped to [0, n_levels - 1]; ur = u -
 *            bf / z; track_depth = |Pc|.  The clamp is applied to the real number before it becomes an integer: NaN gives 0 and
 *            +inf gives n_levels - 1, where the reference's conversion is undefined.
 *   FUSE     the same up to the projection; then IsInImage, half-open: u >= minX && u < maxX && v >= minY && v < maxY; the same
 *            distance gate; PO.Pn < 0.5 dist rejects, without the division; no level is predicted.
 *   DEPTH    z = (row 2 of Rcw) . P + t_z only.  median_depth is element (n - 1) / q, integer division, of the ascending order of the
 *            view's z (KeyFrame.cc:788-790): exactly, by a radix select over the total order of bit patterns that movba_init_map's
 *            median uses (-0 below +0, a positive NaN above +inf).  An empty list gives -1.0, the reference's N == 0 return (:759);
 *            the reference reads out of bounds when N > 0 but no slot holds a point, and that case is an empty list here too.
 * Comparisons as written: a NaN in a point, a normal or a distance passes them as it does there (z = 0 passes the depth test and
 * projects to an infinity or a NaN).  The reference computes in float; this call is fp64 from the boundary to the result (as the
 * LBA), so its decisions can differ from the reference's only for items within float rounding of a gate.
 * The result of an item depends on that item and its view alone, and the result of a view on its own list alone - not on the
 * other views, their order, or how the lists are split over calls - and two calls give the same bits: n_accepted is an integer
 * count, the median is selected, not averaged, and there are no floating-point atomics.
 * Returns MOVBA_ERR_ARG for a NULL handle, descriptor or result; a negative count; n_views > MOVBA_MAX_VIEW_BATCH; n_items above
 * 2^28; view_ptr not ascending or not starting at 0; a point index out of range; an unknown mode; a NULL array that the counts or
 * the modes make necessary (see the fields); fx or fy not positive and finite; any other per-view number that is given and not
 * finite; n_levels < 1; q < 1 on a DEPTH view; log_scale_factor not positive on a FRUSTUM view; a zero quaternion.  MOVBA_ERR_HIP
 * as elsewhere.  Every argument is checked before anything is queued, and on a non-zero status nothing is written except
 * `status`.  No views: MOVBA_OK and nothing else written.  The contents of points, normals and distances may be anything.
 * One packed copy to the device, two launches - k_vp_items, one thread per item over all items of the call, and k_vp_views, one
 * workgroup per view: the count, and for DEPTH views the select, linear in the list: there is no limit like
 * MOVBA_MAX_TWO_VIEW_MATCHES here - and one synchronisation; result arrays that lie in movba_host_alloc memory are written by the
 * kernels themselves.  May share a handle with an uploaded or solved window, waiting for the window's arrays before it reuses
 * the staging buffer: the window, its results and later runs stay as they were. */
int  movba_view_points(movba_handle *h, const movba_view_desc *desc, movba_view_result *res);

/* The numeric body of MapPoint::UpdateNormalAndDepth (MapPoint.cc:362-435) for many map points per call: the mean viewing
 * direction and the scale-invariance distances that movba_view_points takes as `normals`, `max_distance` and `min_distance`.
 * The reference calls it after every step this library accelerates - LocalMapping::CreateNewMapPoints (LocalMapping.cc:488),
 * SearchInNeighbors (:597), ProcessNewKeyFrame (:192), both bundle adjustments (Optimizer.cc:387, :837), both initialisations
 * (Tracking.cc:542, :668, :715), Tracking::CreateNewKeyFrame (Tracking.cc:1082) and Map.cc:277.  The isBad test, the copy of the
 * observations under the feature mutex (:367-375), the choice of mpRefKF and the lookup of the keypoint's octave (:409-423)
 * stay with the caller: it passes the observers as index lists and the octave as a number. */
typedef struct {
    int32_t n_views;
    int32_t n_points;
    int32_t n_levels;               /* mnScaleLevels (:427), >= 1                                                          */
    int32_t pad;
    const double  *poses;           /* n_views x 7: qx qy qz qw tx ty tz = Tcw, as movba_view_desc::poses; the quaternion is
                                       normalised before use; Ow = -Rcw^T tcw (KeyFrame::GetCameraCenter, :392, :406)       */
    const double  *points;          /* n_points x 3, world: mWorldPos (:374)                                               */
    const int32_t *obs_ptr;         /* n_points + 1: ascending prefix, obs_ptr[0] = 0; n_obs = obs_ptr[n_points]            */
    const int32_t *obs_view;        /* n_obs: the observers of point p are [obs_ptr[p], obs_ptr[p + 1]), summed in this order
                                       (mObservations, :372, :383-396)                                                     */
    const int32_t *ref_view;        /* n_points: mpRefKF (:373) as a view index; it need not be in the point's list
                                       (observations[pRefKF] at :409 does not require it either); the entry of a point with
                                       an empty list is not read                                                           */
    const int32_t *ref_level;       /* n_points: octave of the point's keypoint in the reference keyframe (:414),    
                                       0 .. n_levels - 1                                                                   */
    const double  *scale_factors;   /* n_levels: mvScaleFactors (:426, :432); one table per call - every frame of this fork has
                                       the same 8 levels x 1.2 (Frame.cc:103-111)                                          */
} movba_normals_desc;   /* 72 bytes */

typedef struct {
    double  *normals;               /* n_points x 3 out: mNormalVector (:433)                                              */
    double  *max_distance;          /* n_points out: the raw mfMaxDistance (:431), what movba_view_desc::max_distance takes */
    double  *min_distance;          /* n_points out: the raw mfMinDistance (:432)                                          */
    int32_t  status;
    int32_t  pad;
} movba_normals_result; /* 32 bytes; each array is required when n_points > 0 */

/* Restated as written, point by point, fp64 from the boundary to the result (the reference computes in float):
 *   Ow_v   = -Rcw^T tcw of view v, from the pose, by the function movba_view_points derives it with: both calls agree on a
 *            keyframe's centre to the bit.  Computed once per view.
 *   acc = 0, n = 0; for each observer v of the point, strictly in list order (:383-396):
 *            d = P - Ow_v; acc += d / sqrt(dx dx + dy dy + dz dz), a component-wise IEEE division, not a multiplication by a
 *            reciprocal (:393-394); n++
 *   normal = acc / (double)n (:433)
 *   dist   = |P - Ow_ref|, ref = ref_view[p] (:406-407)
 *   max_distance = dist * scale_factors[ref_level[p]] (:431)
 *   min_distance = max_distance / scale_factors[n_levels - 1] (:432)
 * A point with an empty list gets NaN in all five numbers: the reference returns at :377 and leaves the fields as they were.  A
 * point lying in an observer's centre gives whatever the division gives (0 / 0), as it does there.  The reference sums in the
 * iteration order of std::map<KeyFrame*, ...>, which is pointer order; here it is the caller's list order, and that is the only
 * freedom: another order changes a normal by rounding only.  This fork's keyframes have NLeft == -1 and no right-camera
 * observations, so the branches at :397-403 and :416-423 that read them are not restated.
 * A point's result depends only on its own list in its order, the views it names, its ref_view and ref_level entries and the
 * table - not on the other points, their order, or how the points are split over calls - and two calls give the same bits: the
 * sum is sequential, there is no tree over a list and there are no floating-point atomics.
 * Returns MOVBA_ERR_ARG for a NULL handle, descriptor or result; a negative count; n_obs above 2^28; a NULL array that the
 * counts make necessary (obs_ptr, ref_level, scale_factors and the result arrays when n_points > 0; poses when n_views > 0;
 * points, obs_view and ref_view when n_obs > 0); obs_ptr not ascending or not starting at 0; an observer index out of range; a
 * ref_view that is read (a point with observers) out of range; a ref_level outside 0 .. n_levels - 1, or n_levels < 1; a scale
 * factor that is not positive and finite; a pose entry that is not finite, or a zero quaternion.  MOVBA_ERR_HIP as elsewhere.
 * Every argument is checked before anything is queued, and on a non-zero status nothing is written except `status`.  No points:
 * MOVBA_OK and nothing else written.  The contents of `points` may be anything.
 * One packed copy to the device, two launches - k_pn_centres, one thread per view, and k_pn_points, one thread per point walking
 * its list: no limit on views or list length beyond the 2^28 observations, the centres live in device memory - and one
 * synchronisation; result arrays that lie in movba_host_alloc memory are written by the kernels themselves.  May share a handle
 * with an uploaded or solved window, waiting for the window's arrays before it reuses the staging buffer: the window, its
 * results and later runs stay as they were. */
int  movba_point_normals(movba_handle *h, const movba_normals_desc *desc, movba_normals_result *res);

/* The same quantities for every map point of the handle's window after a run (Optimizer.cc:832-838), read out of the window
 * where it lies on the device: the poses, the points and the observation lists do not cross the bus again.
 *   the estimate   the one movba_lba_download returns
 *   the observers  of point l: its uploaded edges in caller order (the upload's grouping by point is stable), as pose indices;
 *                  edges whose outlier[e] is non-zero are skipped - the reference erases those observations at :809-818,
 *                  before :837.  Re-choosing mpRefKF after an erasure (MapPoint::EraseObservation) stays with the caller.
 *   ref_pose       n_points: mpRefKF as an index into the window's poses.  Every entry must be one, also that of a point whose
 *                  edges are all skipped (the lists are on the device: the call cannot tell before it queues which are read)
 *   ref_level      n_points, scale_factors n_levels: as movba_normals_desc
 *   outlier        n_edges in caller edge order - what movba_lba_download returned - or NULL: no edge is skipped.  Copied by
 *                  this call; never read through a pointer the window kept
 *   normals, max_distance, min_distance   out, all required: as movba_normals_result; NaN for a point whose edges are all
 *                  skipped
 * Gives the bits of movba_point_normals fed the downloaded poses and points and the same lists (one kernel and one per-point
 * function serve both).  Returns MOVBA_ERR_ARG (a NULL handle or array other than outlier, n_levels < 1, a ref_pose or ref_level
 * out of range, a scale factor that is not positive and finite), MOVBA_ERR_STATE exactly where movba_lba_marginals gives it (no
 * upload, no run since the upload / reset, or a run whose status was not MOVBA_OK) and MOVBA_ERR_HIP; on a non-zero status
 * nothing is written.  Works after movba_lba_run_batch as well.  The window, its results, its marginals and later runs are left
 * exactly as they were. */
int  movba_lba_point_normals(movba_handle *h, const int32_t *ref_pose, const int32_t *ref_level, const double *scale_factors,
                             int32_t n_levels, const uint8_t *outlier, double *normals, double *max_distance, double *min_distance);

/* The covisibility count for many keyframes or frames per call: "for each map point of this keyframe, for each keyframe that
 * observes it, counter[keyframe]++", then the threshold, the maximum and the ordering - the numeric body of
 * KeyFrame::UpdateConnections (KeyFrame.cc:367-459, run after ProcessNewKeyFrame, SearchInNeighbors and both initialisations),
 * of the voting loop of Tracking::UpdateLocalKeyFrames with its choice of mpReferenceKF (Tracking.cc:1200-1280) and of the count
 * that gives a local window its fixed keyframes (Optimizer.cc:506-522).  Its output decides what the other calls are fed: the
 * neighbours handed to movba_triangulate (GetBestCovisibilityKeyFrames), the views handed to movba_view_points, the window handed
 * to movba_lba_upload.  A query is one keyframe or frame, given as the list of its map points; the observation lists are the
 * prefix array movba_point_normals takes.  Everything is integer: the result is exact. */
#define MOVBA_MAX_COVIS_VIEWS   8192
#define MOVBA_MAX_COVIS_QUERIES 4096

typedef struct {
    int32_t n_views, n_points, n_queries;
    int32_t min_weight;             /* th = 15 (KeyFrame.cc:408); >= 1                                                      */
    int32_t max_out;                /* entries of the ordered list handed out per query, >= 0                               */
    int32_t pad;
    const int32_t *obs_ptr;         /* n_points + 1, as movba_normals_desc::obs_ptr; n_obs = obs_ptr[n_points]              */
    const int32_t *obs_view;        /* n_obs: the observers of each point (MapPoint::GetObservations, :390)                 */
    const uint8_t *eligible;        /* n_views or NULL (all): 0 = the view is never counted (isBad() || GetMap() != mpMap,
                                       KeyFrame.cc:394; isBad, Tracking.cc:1269)                                            */
    const int32_t *query_ptr;       /* n_queries + 1, ascending, [0] = 0; n_items = query_ptr[n_queries]                    */
    const int32_t *query_point;     /* n_items: the non-null, non-bad mvpMapPoints of the query, slot order (:380-388)      */
    const int32_t *query_self;      /* n_queries or NULL (all -1): the query's own view (mnId == mnId is skipped,
                                       KeyFrame.cc:394); -1: a Frame, nothing is skipped (Tracking.cc:1217)                 */
} movba_covis_desc;     /* 72 bytes */

typedef struct {
    int32_t *n_counted;             /* n_queries: views with a count > 0 (KFcounter.size())                                 */
    int32_t *n_connected;           /* n_queries: see below                                                                 */
    int32_t *best_view;             /* n_queries: pKFmax (:421, Tracking.cc:1275), -1 when n_counted == 0                   */
    int32_t *best_weight;           /* n_queries: nmax, 0 when n_counted == 0                                               */
    int32_t *out_view;              /* n_queries x max_out, or NULL when max_out == 0                                       */
    int32_t *out_weight;            /* n_queries x max_out, or NULL when max_out == 0                                       */
    int32_t  status, pad;
} movba_covis_result;   /* 56 bytes */

/* Restated as written, query by query:
 *   count      weight[q][v] = sum over the items i of query q of the number of times v occurs in the list of query_point[i]
 *              (:380-398), for the views v with eligible[v] != 0 and v != query_self[q]; the others are never counted.  A point
 *              that occupies two slots counts twice, as in the loop over mvpMapPoints.  The lists are not checked for duplicate
 *              observers: one that names a view twice counts it twice.
 *   order      the reference sorts vPairs ascending by (weight, pointer) and pushes to the front (:436-443).  Here the view
 *              index stands where the pointer stood, and that is the only freedom taken: the ordered list of a query is all its
 *              counted views by weight descending, ties by view index descending.  out_view / out_weight of query q hold its
 *              first min(n_counted, max_out) entries; behind those out_view holds -1 and out_weight 0.  With max_out <
 *              n_counted the hand-out is a prefix of the full order, and n_counted shows the truncation.
 *   best       `>` in map order (:418, Tracking.cc:1272) keeps the first maximum: best_view is the LOWEST view index among
 *              the views of maximal weight.  On a tie at the top best_view != out_view[0] - as written in the reference, where
 *              mpParent is the front of the list (:454) and pKFmax is not.
 *   connected  n_connected = the number of counted views with weight >= min_weight, not capped by max_out: they are the leading
 *              entries of the order (mvpOrderedConnectedKeyFrames, mvOrderedWeights).  If no view reaches min_weight and
 *              n_counted > 0, n_connected = 1 and the one connection is (best_view, best_weight) (:430-434), not necessarily
 *              out_view[0].  n_counted == 0: n_connected = 0 (the reference returns at :401).
 * What stays with the caller: AddConnection on the other keyframes, the parent / child bookkeeping and
 * mConnectedKeyFrameWeights as a map (the full counter is the ordered list with max_out = n_views); the neighbour / child /
 * parent expansion of UpdateLocalKeyFrames (Tracking.cc:1282-1332) with its breaks; the mnBALocalForKF marks of
 * LocalBundleAdjustment.
 * A query's result depends on its own items, its query_self entry, the lists those items name and `eligible` - not on the other
 * queries, their order, or how the queries are split over calls - and two calls give the same bits: the sums are integer (LDS
 * atomics, which commute), floating point does not occur.
 * Returns MOVBA_ERR_ARG for a NULL handle, descriptor or result; a negative count (n_views, n_points, n_queries, max_out);
 * n_views > MOVBA_MAX_COVIS_VIEWS; n_queries > MOVBA_MAX_COVIS_QUERIES; n_obs or n_items above 2^28; n_queries x max_out above
 * 2^28; min_weight < 1; obs_ptr or query_ptr not ascending or not starting at 0; an observer index outside 0 .. n_views - 1; a
 * point index outside 0 .. n_points - 1; a query_self outside -1 .. n_views - 1; a query whose items' lists hold more than
 * 2^31 - 1 entries together (its weights would not fit); a NULL array that the counts make necessary (the four per-query result
 * arrays, query_ptr, and out_view / out_weight when max_out > 0, when n_queries > 0; obs_ptr when n_points > 0; obs_view when
 * n_obs > 0; query_point when n_items > 0).  MOVBA_ERR_HIP as elsewhere.  Every argument is checked before anything is queued,
 * and on a non-zero status nothing is written except `status`.  n_queries == 0 (with counts that are otherwise in range):
 * MOVBA_OK and nothing else written, the arrays are not looked at.
 * One packed copy to the device, one launch - k_covis, one workgroup per query: the query's counters and sort keys live in the
 * workgroup's LDS, which is what bounds n_views; a caller whose map is larger renumbers the views its queries can reach - and
 * one synchronisation; result arrays that lie in movba_host_alloc memory are written by the kernel itself.  May share a handle
 * with an uploaded or solved window, waiting for the window's arrays before it reuses the staging buffer: the window, its
 * results, its marginals and later runs stay as they were. */
int  movba_covisibility(movba_handle *h, const movba_covis_desc *desc, movba_covis_result *res);

/* The track-id joins of MOVMatcher for many views per call.  In this fork every matcher function is a join on
 * VideoFeature::trackId: SearchForTriangulation (MOVMatcher.h:139-168) is a double loop over the slots of two keyframes, run once
 * per neighbour of a new keyframe; both SearchByVideoFeature (:35-103), SearchForInitialization (:105-137) and the keypoint loop
 * at the tail of Fuse (:249-273) look ids up in a view.  This call is what stands between the other calls: movba_covisibility
 * picks the neighbours, this call joins them, movba_triangulate takes the matches; movba_view_points followed by this call is
 * SearchByVideoFeature and Fuse.  Everything is integer: the result is exact. */
#define MOVBA_TM_TRIANGULATION 0   /* SearchForTriangulation, MOVMatcher.h:139-168                                          */
#define MOVBA_TM_LOOKUP        1   /* the mvVFMap lookups: both SearchByVideoFeature (:35-103), SearchForInitialization
                                      (:105-137), and the keypoint loop of Fuse (:249-273)                                  */
#define MOVBA_MAX_TRACK_SLOTS   16384   /* slots of one view */
#define MOVBA_MAX_TRACK_QUERIES 4096

typedef struct {
    int32_t n_views, n_queries;
    const int32_t *view_ptr;        /* n_views + 1, ascending, [0] = 0: the slots of view v are [view_ptr[v], view_ptr[v + 1]);
                                       n_slots = view_ptr[n_views]                                                          */
    const int32_t *slot_track;      /* n_slots: mvVF[j].trackId in slot order; any int32 is an id (0, negatives, INT32_MIN) */
    const uint8_t *slot_taken;      /* n_slots or NULL (no slot is taken): != 0 where GetMapPointMatches()[j] != NULL       */
    /* per-slot payload, gathered for the TRIANGULATION matches; each may be NULL */
    const double  *slot_obs;        /* n_slots x 2: the keypoint (mvKeysUn[j].pt)                                           */
    const double  *slot_ur;         /* n_slots: mvuRight[j]                                                                 */
    const double  *slot_depth;      /* n_slots: mvDepth[j]                                                                  */
    /* queries */
    const int32_t *query_mode;      /* n_queries: MOVBA_TM_*                                                                */
    const int32_t *query_view;      /* n_queries x 2.  TRIANGULATION: (view 1 = the current keyframe, view 2 = the neighbour),
                                       which may be equal; LOOKUP: (-1, the view searched)                                  */
    const int32_t *query_ptr;       /* n_queries + 1, ascending, [0] = 0; n_items = query_ptr[n_queries]                    */
    const int32_t *item_track;      /* n_items: the ids a LOOKUP query looks up; a TRIANGULATION query has an empty range   */
} movba_track_desc;     /* 88 bytes */

/* match_cap = the sum over the TRIANGULATION queries of the slot count of view 1: what the caller allocates for. */
typedef struct {
    int32_t *pair_ptr;              /* n_queries + 1: dense ascending prefix of the queries' match counts (LOOKUP queries
                                       contribute 0): the layout movba_tri_desc::pair_ptr takes                             */
    int32_t *match_slot1;           /* match_cap: slot in view 1, local to the view (vMatchedIndices), dense in query order,
                                       ascending within a query; -1 behind pair_ptr[n_queries]                              */
    int32_t *match_slot2;           /* match_cap: slot in view 2                                                            */
    /* the payload of the matched slots, in the layout of movba_tri_desc::obs1 .. depth2; each NULL or match_cap entries (x 2
       for obs), NaN behind the last match.  An output whose source array is NULL must be NULL.                             */
    double  *obs1, *obs2;
    double  *ur1, *ur2;
    double  *depth1, *depth2;
    int32_t *item_slot;             /* n_items: per item of a LOOKUP query the slot found, local to the view, or -1         */
    int32_t *n_found;               /* n_queries: items found (the nmatches the lookups return); 0 for TRIANGULATION        */
    int32_t  n_matches;             /* pair_ptr[n_queries]                                                                  */
    int32_t  status;
} movba_track_result;   /* 96 bytes */

/* Restated as written, query by query:
 *   TRIANGULATION  for every slot i of view 1 in ascending order with taken[i] == 0: the lowest slot j of view 2 with
 *              taken[j] == 0 and the id of i; if there is one, (i, j) is a match (the inner loop's `break`, :150-163).  Nothing
 *              makes matches unique: two slots of view 1 that carry one id both match the same j, as in the reference.  The
 *              matches of a query stand in ascending i.  The reference returns an uninitialised nmatches; here the count of a
 *              query is vMatchedPairs.size(), pair_ptr[q + 1] - pair_ptr[q].
 *   LOOKUP     for every item the lowest slot of the view that carries the id, or -1; slot_taken is not looked at.  That is
 *              what std::map::insert leaves in mvVFMap when the map is filled in slot order - the first insertion wins - and
 *              what the ascending scan with `break` of Fuse finds.  MOVExtractor.cc:249 sorts the previous frame's mvVF without
 *              rebuilding its map: a caller who wants that stale map passes the ids in the order the map was built.
 * What stays with the caller: applying the hits in item order (F.mvpMapPoints[slot] = pMP: a later item overwrites an earlier
 * one on the same slot), the isBad, mbTrackInView and far-point filters (a filtered point is simply not passed), Replace and
 * AddObservation.
 * A query's result depends on the slots of its own views, or on its own items and the view it searches - not on the other
 * queries, their order, or how the queries are split over calls - and two calls give the same bits: the join is integer, the
 * payload is copied bit for bit (NaN payloads included), floating-point arithmetic does not occur.
 * Returns MOVBA_ERR_ARG for a NULL handle, descriptor or result; a negative count; n_queries > MOVBA_MAX_TRACK_QUERIES; a view of
 * more than MOVBA_MAX_TRACK_SLOTS slots; n_slots, n_items or match_cap above 2^28 (match_cap is at most 2^26 under the two bounds before it); view_ptr or query_ptr not ascending or not
 * starting at 0; an unknown mode; a view index outside 0 .. n_views - 1, a LOOKUP query whose first view is not -1, a
 * TRIANGULATION query with items; a NULL array that the counts make necessary (query_mode, query_view, query_ptr, view_ptr,
 * pair_ptr and n_found when n_queries > 0; slot_track when n_slots > 0; item_track and item_slot when n_items > 0; match_slot1
 * and match_slot2 when match_cap > 0); a payload output given without its source.  MOVBA_ERR_HIP as elsewhere.  Every argument
 * is checked before anything is queued, and on a non-zero status nothing is written except `status`.  n_queries == 0 (with counts
 * that are otherwise in range): MOVBA_OK and nothing else written, the arrays are not looked at.
 * One packed copy to the device, two launches - k_tm_match, one workgroup per query with an open-addressing table over the
 * searched view's slots in its LDS, which is what bounds the slots of a view, then k_tm_pack, which makes the matches dense,
 * gathers the payload and pads the tail - and one synchronisation; result arrays that lie in movba_host_alloc memory are written
 * by the kernels themselves.  May share a handle with an uploaded or solved window, waiting for the window's arrays before it
 * reuses the staging buffer: the window, its results, its marginals and later runs stay as they were. */
int  movba_track_match(movba_handle *h, const movba_track_desc *desc, movba_track_result *res);

/* EXPRESS detection and descriptors for many frames per call: the pixel arithmetic of MOVExtractor::operator()
 * (MOVExtractor.cc:63-455), which is the EXPRESS code of EXPRESS.h:79-192 - compute_center, compute_descriptor, compute_express,
 * compute_distance - block by block: about 8 000 blocks for a 1080p intra frame or a low-coverage frame (extract_moves, :37-61,
 * :123-156, :418-451), a few thousand for an inter frame (:254-334, :380-416).  It is what produces VideoFeature::trackId's
 * carriers and mvKeysUn[j].pt, which movba_track_match and movba_triangulate take.  Everything is integer: the result is exact.
 * cv::calcOpticalFlowPyrLK (:91, :196, :347) is not part of it. */
#define MOVBA_EX_DETECT   0   /* compute_express, then compute_descriptor where it returns true (:50-52, :132-134, :391-395) */
#define MOVBA_EX_DESCRIBE 1   /* compute_descriptor alone (:223, :290, :313)                                                 */
#define MOVBA_MAX_EXPRESS_IMAGES 1024
#define MOVBA_MAX_EXPRESS_ITEMS  4194304   /* 2^22 */
/* movba_express_result::code, in the order the reference tests */
#define MOVBA_EX_FEATURE      1   /* DETECT passed, descriptor written                                                       */
#define MOVBA_EX_DESCRIBED    2   /* DESCRIBE, descriptor written                                                            */
#define MOVBA_EX_REJ_BOUNDS  16   /* the reference's `if` failed: !(x >= 0 && y >= 0 && x + w < cols && y + h < rows), strict
                                     as written: a block that touches the last column or row is rejected                     */
#define MOVBA_EX_REJ_SHAPE   17   /* (w, h) is not one of 8x8, 16x8, 8x16, 16x16: diagonal() handles no other shape and the
                                     reference reads garbage there                                                           */
#define MOVBA_EX_REJ_FLAT    18   /* the precheck failed                                                                     */
#define MOVBA_EX_REJ_NO_EDGE 19   /* neither diagonal pass succeeded                                                         */

typedef struct {
    int32_t n_images, pad;
    const uint8_t *const *image;    /* n_images pointers to 8-bit grey pixels (imGray, CV_8UC1); may be NULL for an image without
                                       items                                                                                */
    const int32_t *rows, *cols;     /* n_images each, >= 1; the sum of rows * cols over the images is at most 2^28          */
    const int32_t *stride;          /* n_images: bytes from one row to the next, >= cols; only the first cols bytes of a row are
                                       read                                                                                 */
    const int32_t *threshold;       /* n_images: 0 .. 255 (MOVExtractor.threshold: 25 and 40 in the shipped configurations) */
    const int32_t *item_ptr;        /* n_images + 1, ascending, [0] = 0: the items of image i are [item_ptr[i], item_ptr[i + 1]);
                                       n_items = item_ptr[n_images] <= MOVBA_MAX_EXPRESS_ITEMS                              */
    const int32_t *item_rect;       /* n_items x 4: x y w h = cv::Rect; w is img.cols, h is img.rows of the block           */
    const int32_t *item_mode;       /* n_items: MOVBA_EX_*                                                                  */
    const uint64_t *item_ref;       /* n_items x 4 or NULL: the descriptor to measure against (pvf.desc, :291, :314)        */
} movba_express_desc;   /* 80 bytes */

typedef struct {
    uint8_t  *code;                 /* n_items: MOVBA_EX_*                                                                  */
    uint64_t *desc;                 /* n_items x 4: bit k of the bitset<256> is bit k & 63 of word k >> 6; zeros where none was
                                       computed                                                                             */
    int32_t  *count;                /* n_items: desc.count(), the sort key at :252; -1 where no descriptor was computed     */
    int32_t  *distance;             /* n_items or NULL: compute_distance(item_ref, desc); -1 without a descriptor or without
                                       item_ref                                                                             */
    int32_t  *n_features;           /* n_images: the items of the image with MOVBA_EX_FEATURE                               */
    int32_t   status, pad;
} movba_express_result; /* 48 bytes */

/* Restated as written, quirks included, item by item.  I is the item's image, (x0, y0, w, h) its rect.
 *   Tests    MOVBA_EX_REJ_BOUNDS, then MOVBA_EX_REJ_SHAPE; neither kind of rectangle is ever read.
 *   Centre   r = w / 2, c = h / 2.  compute_center hands at<>() its arguments swapped, so r - from the WIDTH - is the ROW offset
 *            and c - from the HEIGHT - is the COLUMN offset: center = (I(y0+r, x0+c) + I(y0+r-1, x0+c-1) + I(y0+r, x0+c-1) +
 *            I(y0+r-1, x0+c)) / 4, the integer quotient.  On 16x8 and 8x16 blocks this reads one pixel right of, or below, the
 *            block; the bounds test keeps it inside the image.
 *   Bounds   low = (center - threshold) mod 256, high = (center + threshold) mod 256 (uint8 wrap-around);
 *            outside(p) = low > p || high < p.
 *   Shifted  the descriptor and the precheck read s(y, x) = I(y0 + y, x0 + x + 1): the `p++` in front of the read (:103, :130).
 *            Descriptor: bit y * h + x (img.rows, not img.cols) is set for outside(s(y, x)), y < h, x < w; where w = 16 and
 *            h = 8 the indices overlap and are OR-ed.  Precheck: passes when the number of outside shifted pixels is at least
 *            (uint8)(h * w * 0.125); the row-wise early `break` only keeps the uint8 counter from wrapping, the decision is the
 *            full count's.
 *   Votes    read the TRUE pixels t(y, x) = I(y0 + y, x0 + x).  slices = h + w - 1; diagonal i of pass 0 is {(y, x): x - y =
 *            i - (h - 1)}, of pass 1 {(y, x): (w - 1 - x) - y = i - (h - 1)} (what the tables at EXPRESS.h:20-38 encode).
 *            rounds = round(0.25 * slices) = 4, 6, 6, 8; u_rounds = slices - rounds.  Per pass wins = losses = 0; for i = 0 ..
 *            slices - 1: win = the outside pixels on the diagonal, loss = its length - win;
 *            if wins < rounds: wins = (win >= loss) ? wins + 1 : 0; if losses < rounds: losses = (loss > win) ? losses + 1 : 0;
 *            break when i > u_rounds && (wins == 0 || losses == 0).  The pass succeeds when wins >= rounds && losses >= rounds;
 *            pass 1 runs only if pass 0 failed.
 *   DETECT   MOVBA_EX_REJ_FLAT when the precheck fails, else MOVBA_EX_REJ_NO_EDGE when both passes fail, else
 *            MOVBA_EX_FEATURE with the descriptor.  DESCRIBE: MOVBA_EX_DESCRIBED with the descriptor, no other test.
 *   count    desc.count(); distance = (item_ref ^ desc).count().
 * What stays with the caller of THIS call: mCurrentId, the lbFound bookkeeping (order-dependent), the float-to-int truncation
 * that makes a cv::Rect, the sort at :249 - all of which movba_advance, below, does for an inter frame - and the LK calls
 * (INTEGRATION.md).
 * An item's result depends on its rect, its mode, its item_ref and its image alone - not on other items, other images, their
 * order, or how they are split over calls - and two calls give the same bits.
 * Returns MOVBA_ERR_ARG for a NULL handle, descriptor or result; n_images negative or above MOVBA_MAX_EXPRESS_IMAGES; item_ptr
 * NULL, not ascending, not starting at 0 or ending above MOVBA_MAX_EXPRESS_ITEMS; a NULL array that the counts make necessary
 * (image, rows, cols, stride, threshold, item_rect, item_mode, code, desc, count, n_features when n_items > 0); a NULL image
 * pointer for an image that has items; rows or cols below 1, stride < cols, or a sum of rows * cols above 2^28; a threshold
 * outside 0 .. 255; an unknown mode.  MOVBA_ERR_HIP as elsewhere.  Every argument is checked before anything is queued, and on a
 * non-zero status nothing is written except `status`.  n_images == 0, or no items at all: MOVBA_OK and nothing else written.
 * One packed copy to the device - the pixels of the images that have items go tightly, row by row without the stride's padding -
 * two launches - k_express, one wavefront per item, then k_express_counts, which hands the per-image counts over - and one
 * synchronisation; result arrays that lie in movba_host_alloc memory are written by the kernels themselves.  May share a handle
 * with an uploaded or solved window, waiting for the window's arrays before it reuses the staging buffer: the window, its
 * results, its marginals and later runs stay as they were. */
int  movba_express(movba_handle *h, const movba_express_desc *desc, movba_express_result *res);
/* The lattice of extract_moves (host only, no device): for y = 8; y < rows - 8; y += 16, and inside that x = 8; x < cols - 8;
 * x += 16, the rect (x - 8, y - 8, 16, 16), in that order; the keypoint of a rect is (x, y).  Writes the first `cap` of them
 * (x y w h) to `rects` and returns the number of rects of the lattice, which may be larger than cap (rects may be NULL when cap
 * is 0); 0 for an image of 16 or fewer rows or columns.  The bounds test is left to movba_express (the loop's own bounds
 * already keep every rect of the lattice inside it: an image of 240 x 320 has 14 x 19 rects).  MOVBA_ERR_ARG for a negative cap, rects NULL
 * with cap > 0, or a lattice of more than 2^31 - 1 rects. */
int  movba_express_grid(int32_t rows, int32_t cols, int32_t *rects, int32_t cap);

/* The inter-frame walk of MOVExtractor::operator() for many frames (streams) per call: from the previous frame's features, the
 * frame's motion vectors and macroblocks to the frame's _vf segments with their track ids (MOVExtractor.cc:245-335, :380-451) -
 * the sort at :249, the choice among up to four motion vectors, the float-to-int truncation that makes a cv::Rect, the lbFound
 * claims of :306-309, the dist <= 40 gate, the new macroblocks, mov_cnt, the grid of :418-451 and mCurrentId.  It is what
 * produces VideoFeature::trackId, the join key of movba_track_match.  Everything is integer except one fp32 add and one fp32
 * subtract per rectangle: the result is exact.  cv::calcOpticalFlowPyrLK (:91, :196, :347), the I-frame path and the
 * relocalisation block (:161-243) are not part of it. */
#define MOVBA_MAX_ADVANCE_PREV 16384   /* previous features of one frame: what one workgroup sorts in LDS (8-byte keys, 128 KiB) */
/* movba_advance_result::fate */
#define MOVBA_ADV_KEPT        1   /* arrived, won its claim (or claimed nothing), dist <= 40: a feature of the kept segment     */
#define MOVBA_ADV_COVERAGE    2   /* prev_coverage != 0: covFeat, handed back untouched for the caller's LK call (:337-377)     */
#define MOVBA_ADV_NO_MV      16   /* cand[0] == -1: no motion vector reaches the feature                                       */
#define MOVBA_ADV_REJ_BOUNDS 17   /* the final rect fails movba_express's bounds test; it claims nothing                       */
#define MOVBA_ADV_LOST_CLAIM 18   /* an in-bounds feature at a lower position reached the same macroblock first (:306)         */
#define MOVBA_ADV_FAR        19   /* arrived and won, but dist > 40 (:311); the macroblock stays found                         */

typedef struct {
    int32_t n_frames, pad;          /* 0 .. MOVBA_MAX_EXPRESS_IMAGES; frames are independent                                */
    const uint8_t *const *image;    /* n_frames pointers to the frame's 8-bit grey pixels; may be NULL for a frame without
                                       previous features, macroblocks and lattice.  The PREVIOUS frame has the same size: the
                                       reference tests :306, :388, :429 against _prev_frame->imageCols/Rows and then reads
                                       imGrey, which only makes sense for one size                                          */
    const int32_t *rows, *cols, *stride, *threshold;   /* n_frames each, as movba_express_desc                              */
    const uint8_t *force_grid;      /* n_frames: _smv->coverageArea < mCoverageThreshold (:418), evaluated by the caller    */
    const int32_t *first_id;        /* n_frames: mCurrentId on entry, >= 0                                                  */
    const int32_t *prev_ptr;        /* n_frames + 1, ascending, [0] = 0: the previous features of frame f, in the caller's
                                       current mvVF order, are [prev_ptr[f], prev_ptr[f + 1]), at most MOVBA_MAX_ADVANCE_PREV */
    const float    *prev_pt;        /* n_prev x 2: VideoFeature::pt, finite, |.| <= 2^20                                    */
    const int32_t  *prev_mb;        /* n_prev x 2: mb.width, mb.height, each 8 or 16                                        */
    const int32_t  *prev_age;       /* n_prev: 0 .. 2^31 - 2                                                                */
    const int32_t  *prev_track;     /* n_prev: trackId                                                                      */
    const uint64_t *prev_desc;      /* n_prev x 4: desc, movba_express's bit order                                          */
    const uint8_t  *prev_coverage;  /* n_prev: VideoFeature::coverage                                                       */
    const int32_t  *prev_cand;      /* n_prev x 4: _smv->mvi.at<Vec4i>((int)pt.y, (int)pt.x), gathered by the caller: -1 or an
                                       index into the frame's motion vectors                                                */
    const int32_t *mv_ptr;          /* n_frames + 1: the motion vectors of frame f                                          */
    const float   *mv_pt;           /* n_mv x 2: MotionVector::pt, finite, |.| <= 2^20                                      */
    const int32_t *mv_dindx;        /* n_mv: -1 or an index into the frame's macroblocks                                    */
    const int32_t *kp_ptr;          /* n_frames + 1: the macroblocks of frame f                                             */
    const int32_t *kp_rect;         /* n_kps x 4: _smv->kps[i] as x y w h                                                   */
    const int32_t *grid_ptr;        /* n_frames + 1, or NULL: nothing is covered.  The range of frame f has exactly
                                       movba_express_grid(rows[f], cols[f]) entries                                         */
    const uint8_t *grid_covered;    /* per rect of the lattice, in lattice order: non-zero where mvi(kp.pt.y, kp.pt.x)[0] >= 0
                                       (:431)                                                                               */
} movba_advance_desc;   /* 184 bytes */

typedef struct {
    int32_t  *order;                /* n_prev: order[prev_ptr[f] + i] = the input index, within the frame, at position i    */
    uint8_t  *fate;                 /* n_prev, by input index: MOVBA_ADV_*                                                  */
    int32_t  *chosen_mv;            /* n_prev, by input index: indx, -1 for MOVBA_ADV_COVERAGE and MOVBA_ADV_NO_MV          */
    int32_t  *distance;             /* n_prev, by input index: compute_distance of the final rect; -1 where no final descriptor
                                       was computed (COVERAGE, NO_MV, REJ_BOUNDS).  A LOST_CLAIM feature has one: the call
                                       describes the final rect before the claims are settled                               */
    uint8_t  *kp_found;             /* n_kps: lbFound                                                                       */
    uint8_t  *kp_code;              /* n_kps: MOVBA_EX_* of DETECT on kp_rect; 0 where kp_found skipped it                  */
    int32_t  *mov_cnt;              /* n_frames: the features of the new segment                                            */
    uint8_t  *grid_ran;             /* n_frames: force_grid || mov_cnt < 60                                                 */
    int32_t  *next_id;              /* n_frames: mCurrentId on exit                                                         */
    int32_t  *seg_ptr;              /* n_frames x 4 + 1: [4 f] .. [4 f + 3] = where the kept, the new and the grid segment of
                                       frame f start and where the frame ends ([4 f + 3] = [4 f + 4]); the last = the total */
    int32_t  *feat_src;             /* capacity each = n_prev + n_kps + n_grid (all frames); kept: position i (qIndx), new:
                                       the macroblock's index, grid: the lattice index                                      */
    int32_t  *feat_track;           /* trackId                                                                              */
    float    *feat_pt;              /* capacity x 2                                                                         */
    int32_t  *feat_rect;            /* capacity x 4: mb as x y w h                                                          */
    int32_t  *feat_age;
    uint64_t *feat_desc;            /* capacity x 4                                                                         */
    int32_t   status, pad;
} movba_advance_result; /* 136 bytes */

/* Restated as written, quirks included, per frame.  n = the frame's previous features; R, C = rows, cols.
 *   Sort     (:249-252) position i = 0 .. n - 1 orders the features by age descending, then desc.count() descending.  std::sort
 *            leaves ties unspecified; HERE TIES STAND IN ASCENDING INPUT INDEX - the one place where the call is more definite
 *            than the reference.  The reference sorts mvVF in place and qIndx is a position in the sorted vector: the caller
 *            reorders its mvVF by `order`.
 *   Feature  at position i, independent of the others.  coverage != 0: MOVBA_ADV_COVERAGE.  cand[0] == -1: MOVBA_ADV_NO_MV.
 *            Otherwise indx = cand[0], and if cand[1] >= 0: bestDesc = 256; for j = 0 .. 3, stopping at the first cand[j] ==
 *            -1: if the rect of cand[j] passes movba_express's bounds test, dist = compute_distance(prev_desc,
 *            compute_descriptor(rect)), and if dist < bestDesc (strict: ties keep the earlier j) bestDesc = dist, indx =
 *            cand[j].  If no candidate is in bounds indx stays cand[0].
 *   Rect     of a vector m: pt = prev_pt + mv_pt[m], one fp32 add per component; x = (int)(pt.x - (float)(w / 2)), y =
 *            (int)(pt.y - (float)(h / 2)): w / 2 the integer quotient, the subtraction in fp32, the conversion truncating
 *            toward zero - pt.x - 8 = -0.5 gives x = 0, which passes the bounds test, as in the reference; (w, h) = prev_mb.
 *   Final    rect = the rect of indx, d = mv_dindx[indx].  Out of bounds: MOVBA_ADV_REJ_BOUNDS, no claim.  Else if d >= 0 the
 *            feature claims macroblock d.
 *   Claims   (:306-309) lbFound[d] is set by the lowest position among the in-bounds features whose chosen vector has dindx =
 *            d; every other such feature: MOVBA_ADV_LOST_CLAIM.  A feature with d = -1 never loses.  The claim comes before
 *            the distance: a winner with dist > 40 still marks the macroblock found.
 *   Gate     (:311-332) desc, dist of the final rect.  dist <= 40: MOVBA_ADV_KEPT, a feature with trackId = prev_track, qIndx =
 *            i, pt (the fp32 sum), mb = the final rect, age = prev_age + 1, the new desc.  Otherwise MOVBA_ADV_FAR.
 *   New      (:380-416) in macroblock order, skipping lbFound: movba_express's DETECT on kp_rect, its bounds and shape codes
 *            included.  MOVBA_EX_FEATURE: trackId = ++mCurrentId, qIndx = -1, pt = (x + w / 2, y + h / 2) - (br + tl) * 0.5,
 *            exact for the two widths that pass - mb = the rect, age = 0.  mov_cnt = their number.
 *   Grid     (:418-451) if force_grid || mov_cnt < 60: DETECT over the lattice of movba_express_grid; its features, in lattice
 *            order, where grid_covered == 0: trackId = ++mCurrentId, pt = (x + 8, y + 8), mb = the rect, age = 0, coverage =
 *            true.
 *   Ids      next_id = first_id + mov_cnt + the grid features emitted; new-segment ids precede grid-segment ids.
 * The feature list is dense over the call: frame after frame, per frame kept (position order) | new (macroblock order) | grid
 * (lattice order); entries behind the total are -1 (integers), NaN (feat_pt) and 0 (feat_desc).
 * What stays with the caller: _keypoints / dIndx numbering, _vfmap, the LK calls (coverage features come back by fate, in
 * position order), the relocalisation block, pushing `descriptors`.
 * A frame's result depends on that frame's data alone, and two calls give the same bits.
 * Returns MOVBA_ERR_ARG for a NULL handle, descriptor or result; n_frames negative or above MOVBA_MAX_EXPRESS_IMAGES; prev_ptr,
 * mv_ptr, kp_ptr NULL, or one of them or grid_ptr not ascending from 0; more than MOVBA_MAX_ADVANCE_PREV previous features in a
 * frame; n_prev + n_kps + n_grid (the wave items, n_grid the lattices' rects) above MOVBA_MAX_EXPRESS_ITEMS; a NULL array that
 * the counts make necessary, or a NULL result array; prev_mb not 8 or 16; prev_age outside 0 .. 2^31 - 2; prev_cand outside
 * -1 .. n_mv - 1 or mv_dindx outside -1 .. n_kps - 1 (the frame's counts); a prev_pt or mv_pt that is not finite or above 2^20
 * in magnitude; a grid_covered range whose length is not the lattice's; first_id negative or first_id + n_kps + n_grid above
 * INT32_MAX; and the image conditions of movba_express (a NULL image for a frame that has items).  MOVBA_ERR_HIP as elsewhere.
 * Every argument is checked before anything is queued, and on a non-zero status nothing is written except `status`.
 * n_frames == 0: MOVBA_OK and nothing else written.
 * One packed copy to the device, four launches - k_adv_sort (a workgroup per frame), k_adv_blocks (a wavefront per previous
 * feature, macroblock and lattice rect), k_adv_resolve (a workgroup per frame) and k_adv_emit - and one synchronisation; result
 * arrays that lie in movba_host_alloc memory are written by the kernels themselves.  May share a handle with an uploaded or
 * solved window, waiting for the window's arrays before it reuses the staging buffer: the window, its results, its marginals
 * and later runs stay as they were. */
int  movba_advance(movba_handle *h, const movba_advance_desc *desc, movba_advance_result *res);

/* The decoder's motion-vector image for many frames (streams) per call: the loop of VideoDecoder::NextImage over a frame's
 * AVMotionVector side data (VideoDecoder.cc:198-351) - the skip of records whose destination block leaves the frame, _smv->kps
 * and _smv->mvs, the source blocks painted into the CV_32SC4 image _smv->mvi, coverageArea - and the only reads MOVExtractor
 * makes of that image: at the previous features (MOVExtractor.cc:265-295) and at the lattice centres (:431).  It goes from
 * the records and the query points to movba_advance's input arrays: the image (16 bytes per pixel, cleared and painted per
 * frame) is never formed.  The P-frame path with one reference frame: every record has ref == 0 and source < 0, what the
 * reference's encoder line (ffmpeg.txt: bframes=0:ref=1) produces.  Block sizes are 4, 8 or 16, so every half-size is an
 * integer and the reference's float arithmetic is exact in integers; every area is a multiple of 16, so its fp32 running sum
 * is exact up to 2^28.  The result is exact. */
typedef struct {
    int32_t n_frames, pad;          /* 0 .. MOVBA_MAX_EXPRESS_IMAGES; frames are independent                                */
    const int32_t *rows, *cols;     /* n_frames each: height and width, 1 .. 32767                                          */
    const double  *coverage_threshold;  /* n_frames: mCoverageThreshold, finite                                             */
    const uint8_t *want_grid;       /* n_frames: non-zero also queries the lattice of movba_express_grid(rows, cols)        */
    const int32_t *rec_ptr;         /* n_frames + 1, ascending, [0] = 0: the records of frame f, in side-data order, are
                                       [rec_ptr[f], rec_ptr[f + 1]), at most 2^20 of them                                   */
    const int16_t *src_x, *src_y, *dst_x, *dst_y;  /* n_records each: AVMotionVector's fields of the same names             */
    const uint8_t *w, *h;           /* n_records each: 4, 8 or 16                                                           */
    const int32_t *source, *ref;    /* n_records each: source < 0 and ref == 0; checked, not sent to the device             */
    const int32_t *q_ptr;           /* n_frames + 1, ascending, [0] = 0: the point queries of frame f                       */
    const float   *q_pt;            /* n_q x 2: what movba_advance takes as prev_pt; finite, |.| <= 2^20.  The queried pixel
                                       is ((int)pt.x, (int)pt.y), truncating toward zero as the reference's cast does       */
} movba_mv_raster_desc;   /* 128 bytes */

typedef struct {
    int32_t *kept_ptr;              /* n_frames + 1: the kept records of frame f are rows [kept_ptr[f], kept_ptr[f + 1]) of
                                       kp_rect, mv_pt and mv_dindx: movba_advance's mv_ptr AND kp_ptr                       */
    int32_t *kp_rect;               /* capacity n_records x 4: _smv->kps as x y w h; behind kept_ptr[n_frames]: -1          */
    float   *mv_pt;                 /* capacity n_records x 2: MotionVector::pt; behind the total: NaN                      */
    int32_t *mv_dindx;              /* capacity n_records: MotionVector::dIndx, the index within the frame.  On this path kps
                                       and mvs are pushed together, so mv_dindx[kept_ptr[f] + m] = m; behind the total: -1  */
    int32_t *rec_kept;              /* n_records: the index m of the record among its frame's kept records, or -1           */
    int32_t *cand;                  /* n_q x 4: mvi.at<Vec4i>((int)pt.y, (int)pt.x): -1 or an index m into the frame's kept
                                       records: movba_advance's prev_cand                                                   */
    int32_t *grid_ptr;              /* n_frames + 1: the lattice rects of frame f, movba_express_grid(rows[f], cols[f]) of
                                       them for every frame: movba_advance's grid_ptr                                       */
    uint8_t *grid_covered;          /* per lattice rect (x, y, 16, 16), in lattice order: 1 where mvi(y + 8, x + 8)[0] >= 0,
                                       else 0; 0 throughout a frame whose want_grid is 0                                    */
    int32_t *cover_px;              /* n_frames: the sum of w * h over the kept records                                     */
    double  *coverage_area;         /* n_frames: _smv->coverageArea                                                         */
    uint8_t *force_grid;            /* n_frames: coverage_area < coverage_threshold: movba_advance's force_grid             */
    int32_t  status, pad;
} movba_mv_raster_result; /* 96 bytes */

/* Restated as written, quirks included, per frame.  W = cols, H = rows; records i in order.
 *   Keep     (:215-253) hx = w / 2, hy = h / 2.  The record is skipped if dst_x + hx >= W or dst_y + hy >= H.  There is no test
 *            on the low side: the rect is (max(dst_x - hx, 0), max(dst_y - hy, 0), w, h) and keeps its full size after the
 *            clamp.  Kept records are numbered densely m = 0, 1, ... in record order; kps[m] and mvs[m] are pushed together,
 *            so mv_dindx[m] = m.  mv_pt[m] = ((float)(dst_x - src_x), (float)(dst_y - src_y)).
 *   Coverage (:347-350) cover_px = the sum of w * h over the kept records; coverage_area = (double)cover_px / (double)(W * H);
 *            force_grid = coverage_area < coverage_threshold, a strict comparison as at MOVExtractor.cc:418.
 *   Extent   (:291-306) of kept record m: x0 = max(src_x - hx, 0), x1 = min(src_x + hx, W - 1), y0 = max(src_y - hy, 0), y1 =
 *            min(src_y + hy, H - 1), both ends inclusive: an unclipped block paints (w + 1) x (h + 1) pixels, as the
 *            reference's <= loops do.  The extent is empty if x0 > x1 or y0 > y1 - a source wholly left of, above, right of or
 *            below the frame - and still uses up its index m.
 *   Slots    (:330-345) of a pixel: with m_0 < m_1 < ... < m_(k-1) the kept records whose extent contains it, cand = (m_0,
 *            m_1, m_2, m_(k-1) if k >= 4 else -1), -1 for the missing ones: the first three records to reach a pixel take
 *            slots 0 .. 2 and every later one overwrites slot 3.  A function of the set alone.
 *   Queries  cand for every point query; grid_covered = cand[0] >= 0 at pixel (x + 8, y + 8) of lattice rect (x, y, 16, 16)
 *            where want_grid is set.  A query pixel outside the image gives four -1: the reference reads outside its matrix
 *            there - the one place where the call is more definite than the reference.
 * kept_ptr, kp_rect, mv_pt, mv_dindx, cand, grid_ptr, grid_covered and force_grid go into movba_advance_desc unchanged (kept_ptr
 * as mv_ptr and kp_ptr, cand as prev_cand).
 * What stays with the caller: the decoder and its queue, records with ref > 0 (they write into other frames of the queue),
 * records with source > 0 (B-frames: bmap, which nothing reads), the images.
 * A frame's result depends on that frame's data alone, and two calls give the same bits.
 * Returns MOVBA_ERR_ARG for a NULL handle, descriptor or result; n_frames negative or above MOVBA_MAX_EXPRESS_IMAGES; rec_ptr or
 * q_ptr NULL or not ascending from 0; more than 2^20 records in a frame; n_records + n_q + n_grid (the lattices' rects of all
 * frames) above MOVBA_MAX_EXPRESS_ITEMS; a NULL array that the counts make necessary (rows, cols, coverage_threshold, want_grid
 * always), or a NULL result array; rows or cols outside 1 .. 32767, or a sum of rows * cols above 2^28; w or h outside {4, 8,
 * 16}; ref != 0 or source >= 0; a q_pt that is not finite or above 2^20 in magnitude; a coverage_threshold that is not finite.
 * MOVBA_ERR_HIP as elsewhere.  Every argument is checked before anything is queued, and on a non-zero status nothing is written
 * except `status`.  n_frames == 0: MOVBA_OK and nothing else written.
 * One packed copy to the device, five launches - k_mvr_count and k_mvr_keep (a workgroup per chunk of 1024 records: keep flags,
 * the dense index from the counts of the chunks before, records per 16 x 16 tile), k_mvr_offsets (one workgroup: kept_ptr,
 * coverage, tile offsets), k_mvr_fill (a thread per kept record: its rows, its entries in at most 2 x 2 tiles' lists) and
 * k_mvr_query (a thread per query: its tile's list) - and
 * one synchronisation; result arrays that lie in movba_host_alloc memory are written by the kernels themselves.  May share a
 * handle with an uploaded or solved window, waiting for the window's arrays before it reuses the staging buffer: the window,
 * its results, its marginals and later runs stay as they were. */
int  movba_mv_raster(movba_handle *h, const movba_mv_raster_desc *desc, movba_mv_raster_result *res);

/* Sparse pyramidal Lucas-Kanade for the points of many independent frames (streams) per call: cv::calcOpticalFlowPyrLK as the
 * reference calls it in four places - every previous feature of an I-frame (MOVExtractor.cc:91, window 31), the relocalisation
 * block (:196, window 31), the coverage features of every P-frame (:347, window 31: movba_advance's MOVBA_ADV_COVERAGE) and every
 * keypoint of a stereo frame, left to right (Frame.cc:304, window 21) - all with 3 pyramid levels above the image,
 * TermCriteria(COUNT + EPS, 20, 0.01), OPTFLOW_LK_GET_MIN_EIGENVALS and a minimum-eigenvalue threshold of 1e-4.  The pyramids
 * of both images are built on the device, a wavefront walks each point from the top level down, and the gate that the extractor
 * applies behind the call (:98, :354) comes back as `keep` with the dense list of the kept points.
 * [opencv-upstream] OpenCV's source is not part of the reference tree: the rules below restate the non-SIMD path of OpenCV 4.6
 * (lkpyramid.cpp, pyramids.cpp) as SURVEY.md marks such text, and they - not a library build - are the contract of this call. */
#define MOVBA_LK_MAX_WIN      31
#define MOVBA_LK_MAX_LEVEL     3
#define MOVBA_LK_MAX_ITER     30
#define MOVBA_LK_MAX_PIXELS   67108864  /* 2^26: the sum of rows * cols over the frames of a call; both pyramids of all of them
                                           then take less than 2^28 bytes of the handle's device scratch and the two level-0
                                           images 2^27 bytes of its staging buffer                                           */
/* movba_lk_result::exit_code: why the loop at level 0 ended, or why it never ran */
#define MOVBA_LK_EPS           1  /* |delta|^2 <= eps^2                                                                      */
#define MOVBA_LK_OSCILLATION   2  /* delta + prevDelta below 0.01 on both axes: the stored point steps back by delta / 2     */
#define MOVBA_LK_MAX_ITER_RAN  3  /* all max_iter iterations ran                                                             */
#define MOVBA_LK_REJ_START    16  /* the window's corner is out of bounds at level 0 before anything is read: status 0, err 0 */
#define MOVBA_LK_REJ_MIN_EIG  17  /* level 0: minEig < min_eig_threshold or D < FLT_EPSILON: status 0                         */
#define MOVBA_LK_REJ_LOOP     18  /* the window's corner left the bounds inside the loop at level 0: status 0                 */

typedef struct {
    int32_t n_frames, pad;          /* 0 .. MOVBA_MAX_EXPRESS_IMAGES; frames are independent                                */
    const uint8_t *const *prev_image, *const *next_image;  /* n_frames pointers each to 8-bit grey pixels, as
                                       movba_express_desc::image; either may be NULL for a frame without points             */
    const int32_t *rows, *cols;     /* n_frames each, both > win; the sum of rows * cols is at most MOVBA_LK_MAX_PIXELS      */
    const int32_t *stride;          /* n_frames: bytes from one row to the next of BOTH images, >= cols                      */
    const int32_t *win;             /* n_frames: winSize (square), odd, 3 .. MOVBA_LK_MAX_WIN; the reference: 31 and 21      */
    const int32_t *pt_ptr;          /* n_frames + 1, ascending, [0] = 0: the points of frame f; n_pt = pt_ptr[n_frames] <=
                                       MOVBA_MAX_EXPRESS_ITEMS                                                              */
    const float   *pt;              /* n_pt x 2: prevPts, x y; finite, |.| <= 2^20                                          */
    int32_t max_level, max_iter;    /* maxLevel 0 .. MOVBA_LK_MAX_LEVEL (3); TermCriteria::maxCount 1 .. MOVBA_LK_MAX_ITER (20) */
    double  eps;                    /* TermCriteria::epsilon, finite, 0 < eps <= 10 (0.01)                                   */
    double  min_eig_threshold;      /* minEigThreshold, finite, > 0 (1e-4)                                                   */
} movba_lk_desc;   /* 96 bytes */

typedef struct {
    float   *next_pt;               /* n_pt x 2: nextPts                                                                    */
    uint8_t *pt_status;             /* n_pt: the call's `status` vector, 1 or 0                                             */
    float   *err;                   /* n_pt: the call's `err` vector: the minimum eigenvalue of the lowest level that formed
                                       its matrix (0 without one), what OPTFLOW_LK_GET_MIN_EIGENVALS makes of it            */
    uint8_t *exit_code;             /* n_pt: MOVBA_LK_*                                                                     */
    uint8_t *keep;                  /* n_pt: pt_status && 0 <= next_pt.x < cols && 0 <= next_pt.y < rows                    */
    int32_t *kept_ptr;              /* n_frames + 1: the kept points of frame f are entries [kept_ptr[f], kept_ptr[f + 1]) of
                                       kept_src                                                                             */
    int32_t *kept_src;              /* capacity n_pt, dense over the call: the index WITHIN THE FRAME of each kept point, in
                                       input order - what the reference's push order makes dIndx; behind the total: -1      */
    int32_t  status, pad;
} movba_lk_result; /* 64 bytes */

/* Restated as written [opencv-upstream], per frame.  W = cols, H = rows, win = the frame's window.
 *   Pyramid  of each image: level 0 is the image; level l + 1 has size ((w + 1) / 2, (h + 1) / 2) and pixel (x, y) =
 *            (sum over i, j in 0 .. 4 of k[i] k[j] src(r(2x + i - 2), r(2y + j - 2)) + 128) >> 8, k = [1 4 6 4 1], r the
 *            BORDER_REFLECT_101 index (-1 -> 1, w -> w - 2) on the source level; all integer.  The levels used are 0 .. L, L
 *            the largest value <= max_level such that every level 1 .. L has both sides > win (buildOpticalFlowPyramid stops
 *            there).
 *   Reads    a pixel outside a level is the REFLECT_101 pixel.  The derivative is Scharr, unscaled int16: Ix = 3 d(y - 1) +
 *            10 d(y) + 3 d(y + 1) with d(y) = p(x + 1, y) - p(x - 1, y), Iy the transpose, with REFLECT_101 neighbours at a
 *            position inside the level; at a position OUTSIDE the level the derivative is 0, the constant border of the
 *            derivative buffer.  Both pyramids carry a border of win pixels, which the bounds test below never leaves.
 *   Point    status = 1; for l = L .. 0 on level l (w_l x h_l):
 *     Start    prevPt = pt * 2^-l, exact.  nextPt = prevPt at level L, else 2 * nextPt; it is stored.  half = (win - 1) * 0.5f;
 *              p = prevPt - half; ip = floor(p).  If ip.x < -win || ip.x >= w_l || ip.y < -win || ip.y >= h_l: at level 0 status
 *              = 0, err = 0, MOVBA_LK_REJ_START; on to the next level - an upper level that fails leaves the stored point as it
 *              is and the walk continues.
 *     Weights  a = p.x - ip.x, b = p.y - ip.y in fp32; iw00 = rint((1 - a)(1 - b) * 16384), iw01 = rint(a (1 - b) * 16384), iw10
 *              = rint((1 - a) b * 16384), to nearest with ties to even; iw11 = 16384 - iw00 - iw01 - iw10.
 *     Patch    for (x, y) in win x win: I = descale(p(ip + (x, y)) iw00 + p(+ (1, 0)) iw01 + p(+ (0, 1)) iw10 + p(+ (1, 1))
 *              iw11, 9) on the previous image, Ix and Iy = descale(the same sum over the derivative, 14); descale(v, n) = (v +
 *              (1 << (n - 1))) >> n, an arithmetic shift.  |Ix|, |Iy| <= 4080, I <= 8160.
 *     Sums     A11 = sum Ix^2, A12 = sum Ix Iy, A22 = sum Iy^2 and, in the loop, b1 = sum diff Ix, b2 = sum diff Iy are EXACT
 *              integers (961 terms stay below 2^36), converted once to fp32 and multiplied by 2^-20.  OpenCV keeps fp32 running
 *              sums whose value depends on its SIMD width: the exact sum is the one place where the call is more definite than
 *              the reference.
 *     Matrix   in fp32, one rounding per operation: D = A11 A22 - A12^2; minEig = (A22 + A11 - sqrt((A11 - A22)^2 + 4 A12^2)) /
 *              (2 win win); err = minEig.  If minEig < min_eig_threshold (compared in fp64) or D < FLT_EPSILON: at level 0
 *              status = 0, MOVBA_LK_REJ_MIN_EIG; on to the next level.  D = 1 / D.
 *     Loop     nextPt -= half; for j = 0 .. max_iter - 1: ip = floor(nextPt); the bounds test of Start - at level 0 status = 0
 *              (MOVBA_LK_REJ_LOOP) - break.  Weights from nextPt.  diff = descale(the weighted sum over the NEXT image, 9) - I.
 *              delta = ((A12 b2 - A22 b1) D, (A12 b1 - A11 b2) D); nextPt += delta; nextPt + half is stored.  Break if
 *              (double)dx^2 + (double)dy^2 <= eps^2 (MOVBA_LK_EPS).  If j > 0 && |dx + prevdx| < 0.01 && |dy + prevdy| < 0.01
 *              (the fp32 sums against the fp64 constant): the stored point -= delta * 0.5f; break (MOVBA_LK_OSCILLATION).
 *              prevDelta = delta.  Otherwise MOVBA_LK_MAX_ITER_RAN.  The bounds tests compare floor()'s float, so a point that
 *              has run beyond the integers fails them like any other.
 *     With OPTFLOW_LK_GET_MIN_EIGENVALS nothing runs behind the loop: no final bounds test and no patch error.
 *   keep     pt_status && 0 <= next_pt.x < W && 0 <= next_pt.y < H on the fp32 values (:98, :354); kept_ptr and kept_src
 *            list the kept points in input order.
 * What stays with the caller: the choice of the points and of the image pair; the feature construction behind :98 and :354
 * (track ids, ages, descriptors: movba_express's DESCRIBE on the new rect); relocalisation's choice of the best point (:196 on);
 * the stereo gates of Frame.cc:306-353 (row difference, disparity range, depth, the median rule) are movba_stereo_points, which
 * takes pt, next_pt and pt_status as they are.
 * A frame's result depends on that frame's data alone, a point's on its frame's images, window and its own coordinates, and two
 * calls give the same bits.
 * Returns MOVBA_ERR_ARG for a NULL handle, descriptor or result; n_frames negative or above MOVBA_MAX_EXPRESS_IMAGES; pt_ptr NULL
 * or not ascending from 0; n_pt above MOVBA_MAX_EXPRESS_ITEMS; a NULL array that the counts make necessary (prev_image,
 * next_image, rows, cols, stride, win always, pt when n_pt > 0), or a NULL result array; a NULL image pointer for a frame that has
 * points; win even or outside 3 .. MOVBA_LK_MAX_WIN; rows or cols <= win (so that one reflection always suffices at level 0);
 * stride < cols; a sum of rows * cols above MOVBA_LK_MAX_PIXELS; max_level outside 0 .. 3, max_iter outside 1 .. 30; eps not
 * finite, <= 0 or > 10 (beyond which OpenCV clamps it); min_eig_threshold not finite or <= 0; a pt that is not finite or above
 * 2^20 in magnitude.  MOVBA_ERR_HIP as elsewhere.  Every argument is checked before anything is queued, and on a non-zero status
 * nothing is written except `status`.  n_frames == 0: MOVBA_OK and nothing else written.
 * One packed copy to the device - level 0 of both images of the frames that have points, row by row without the stride's
 * padding - at most five launches - k_lk_pyr per level 1 .. 3 (a thread per pixel), k_lk_track (a wavefront per point: lane t
 * owns window entries t, t + 64, ..., integer wave sums, the same fp32 tail in every lane) and k_lk_keep (a workgroup per frame:
 * kept_ptr, kept_src) - and one synchronisation; result arrays that lie in movba_host_alloc memory are written by the kernels
 * themselves.  May share a handle with an uploaded or solved window, waiting for the window's arrays before it reuses the
 * staging buffer: the window, its results, its marginals and later runs stay as they were. */
int  movba_lk_track(movba_handle *h, const movba_lk_desc *desc, movba_lk_result *res);

/* Stereo depths and new map points for the keypoints of many independent stereo frames per call: what the reference does
 * between the left-to-right LK call and the use of mvuRight / mvDepth - the gates of Frame::ComputeStereoMatches behind the LK
 * call (Frame.cc:306-338), its median-distance pruning (:340-353), Frame::UnprojectStereo (:836-851) and the choice of the
 * points that Tracking::StereoInitialization (Tracking.cc:532-547), Tracking::CreateNewKeyFrame (:1022-1098) and
 * Tracking::UpdateLastFrame (:828-887) turn into map points.  It takes movba_lk_track's arrays as they are and gives u_right
 * and depth in the layout that movba_lba_solve (obs_right), movba_triangulate (ur1 / depth1) and movba_track_match read.
 * Arithmetic marked [opencv-upstream] restates OpenCV 4.6 as SURVEY.md marks such text. */
#define MOVBA_MAX_STEREO_POINTS 16384   /* keypoints of one frame: what one workgroup sorts in LDS (8-byte keys, 128 KiB) */
/* movba_stereo_desc::select */
#define MOVBA_STEREO_SELECT_NONE   0  /* depths only                                                                          */
#define MOVBA_STEREO_SELECT_ALL    1  /* StereoInitialization: every point with depth > 0, in index order; all are new        */
#define MOVBA_STEREO_SELECT_CLOSE  2  /* CreateNewKeyFrame / UpdateLastFrame: by depth, up to th_depth and max_point          */
/* movba_stereo_result::code */
#define MOVBA_STEREO_OK             1
#define MOVBA_STEREO_REJ_STATUS    16  /* pt_status 0 or next_pt outside the right image                                       */
#define MOVBA_STEREO_REJ_ROW       17  /* |next_pt.y - pt.y| > max_row_diff                                                    */
#define MOVBA_STEREO_REJ_DISPARITY 18  /* pt.x - next_pt.x outside [min_disparity, max_disparity)                              */
#define MOVBA_STEREO_REJ_FAR       19  /* accepted by the gates, pruned by the median rule                                     */

typedef struct {
    int32_t n_frames, pad;          /* 0 .. MOVBA_MAX_EXPRESS_IMAGES; frames are independent                                */
    const int32_t *pt_ptr;          /* n_frames + 1, ascending, [0] = 0: the points of frame f, at most MOVBA_MAX_STEREO_POINTS
                                       of them; n_pt = pt_ptr[n_frames] <= MOVBA_MAX_EXPRESS_ITEMS - as movba_lk_desc          */
    const float   *pt;              /* n_pt x 2: mvKeys[i].pt, the very array given to movba_lk_track; finite, |.| <= 2^20     */
    const float   *next_pt;         /* n_pt x 2: movba_lk_result::next_pt; finite, |.| <= 2^20 where pt_status != 0           */
    const uint8_t *pt_status;       /* n_pt: movba_lk_result::pt_status                                                      */
    const float   *pt_un;           /* n_pt x 2 or NULL: mvKeysUn[i].pt, what is un-projected; NULL: pt (zero distortion)     */
    const int32_t *rows, *cols;     /* n_frames each, >= 1: the RIGHT image's                                                */
    const float   *bf;              /* n_frames: mbf, finite, > 0                                                            */
    const float   *max_disparity;   /* n_frames: maxD, finite.  An input: the reference reads mb before it is assigned (below);
                                       the intended value is mbf / (mbf / fx), computed in fp32                              */
    const float   *th_depth;        /* n_frames: mThDepth, finite (read for MOVBA_STEREO_SELECT_CLOSE)                        */
    const float   *cam;             /* n_frames x 4: fx fy cx cy, finite, fx fy > 0                                          */
    const int32_t *select;          /* n_frames: MOVBA_STEREO_SELECT_*                                                       */
    const double  *poses;           /* n_frames x 7 or NULL: Tcw as movba_view_desc::poses (qx qy qz qw tx ty tz, the quaternion
                                       normalised first); NULL: the identity for every frame (SetPose(SE3f()), Tracking.cc:524) */
    const uint8_t *has_point;       /* n_pt or NULL: 1 where mvpMapPoints[i] is a map point with at least one observation;
                                       NULL: all 0                                                                           */
    float   max_row_diff;           /* finite (4)                                                                            */
    float   min_disparity;          /* minD, finite (0)                                                                      */
    int32_t max_point, pad2;        /* maxPoint >= 0 (100)                                                                   */
} movba_stereo_desc;   /* 136 bytes */

typedef struct {
    float   *u_right, *depth;       /* n_pt each: mvuRight, mvDepth; -1 where there is no stereo observation, after pruning   */
    uint8_t *code;                  /* n_pt: MOVBA_STEREO_*                                                                  */
    int32_t *n_stereo;              /* n_frames: the frame's points left with depth > 0                                      */
    int32_t *median_dist;           /* n_frames: the upper median of the int distances; -1 without a candidate               */
    float   *th_dist;               /* n_frames: thDist; 0 without a candidate                                               */
    int32_t *sel_ptr;               /* n_frames + 1: the selected points of frame f are entries [sel_ptr[f], sel_ptr[f + 1]) of
                                       the four arrays below, dense over the call                                            */
    int32_t *sel_src;               /* capacity n_pt: the index WITHIN THE FRAME, in walk order; behind the total: -1         */
    uint8_t *sel_new;               /* capacity n_pt: 1 where the walk creates a map point; behind the total: 0               */
    float   *sel_cam;               /* capacity n_pt x 3: x y z of Frame.cc:843-845; behind the total: NaN                    */
    double  *sel_point;             /* capacity n_pt x 3: x3D, world; behind the total: NaN                                   */
    int32_t  status, pad;
} movba_stereo_result; /* 96 bytes */

/* Restated as written, per frame.  W = cols, H = rows of the right image.
 *   Gates    per keypoint i, fp32, one rounding per operation; L = pt[i], R = next_pt[i]:
 *     1  pt_status[i] == 0 || R.x < 0 || R.y < 0 || R.x >= (float)W || R.y >= (float)H: MOVBA_STEREO_REJ_STATUS (-0.0 passes).
 *     2  fabsf(R.y - L.y) > max_row_diff: MOVBA_STEREO_REJ_ROW (std::abs(float): Frame.h:36 has `using namespace std`).
 *     3  disparity = L.x - R.x; unless disparity >= min_disparity && disparity < max_disparity: MOVBA_STEREO_REJ_DISPARITY.
 *     4  if disparity <= 0: disparity = (float)0.01 and bestUr = (float)((double)L.x - 0.01) - the source subtracts a double
 *        literal; otherwise bestUr = R.x.
 *     5  depth = bf / disparity; u_right = bestUr.
 *     6  d = L - R in fp32; dist = (float)sqrt((double)d.x d.x + (double)d.y d.y) (cv::norm(Point2f), [opencv-upstream]), stored
 *        into pair<int, int>: TRUNCATED to an int.
 *     max_disparity: the reference computes mbf / mb (Frame.cc:290-292), but mb is assigned at :255, behind the call of
 *     ComputeStereoMatches at :230, and the constructor's initialiser list (:192-195) does not set it: the value read is
 *     indeterminate.  So it is an input here.
 *   Pruning  (:340-353) median = the int distance of rank size / 2 among the accepted points' sorted distances - the UPPER
 *            median; thDist = 1.5f * 1.4f * (float)median, left to right; every accepted point with (float)dist >= thDist
 *            loses its observation: u_right = depth = -1, MOVBA_STEREO_REJ_FAR.  (Walking the sorted pairs from the back until
 *            the first below thDist is exactly that: no order is observable, only the median's value.)  A median of 0 gives
 *            thDist 0 and prunes EVERY accepted point - kept as it is.  Without an accepted point the reference indexes an
 *            empty vector; here nothing is pruned, median_dist = -1 and th_dist = 0.
 *   Point    (:836-851) for z = depth[i] > 0: x = (u - cx) * z * invfx, y = (v - cy) * z * invfy, left to right in fp32 with
 *            invfx = 1.0f / fx, (u, v) = pt_un[i] - mvKeysUn, which is mvKeys whenever mDistCoef[0] == 0 (:684-688); sel_cam =
 *            (x, y, z).  sel_point = Rwc * (double)sel_cam + Ow in fp64: each row's three products summed left to right, then +
 *            Ow, without FMA.  Rwc and Ow come from the pose through the function behind movba_view_points' views and
 *            movba_point_normals' centres, but evaluated once per frame on the HOST, without FMA, so that the device and the
 *            header's host walk give the same sel_point bit for bit.  Those two calls evaluate the same statements on the
 *            device, where a product may be fused with the add of its statement: a frame's centre here can differ from theirs
 *            in the last bit.
 *   Select   MOVBA_STEREO_SELECT_ALL (Tracking.cc:532-547): every i with depth > 0, in index order; sel_new = 1 unless
 *            has_point says otherwise.  MOVBA_STEREO_SELECT_CLOSE (:1022-1098, :828-887): the pairs (z, i) with z > 0 sorted
 *            ascending by z, then i; entry j = 0, 1, ... is listed, new iff has_point[i] == 0; nPoints counts either way, so
 *            nPoints == j + 1; behind entry j the walk stops if z_j > th_depth && nPoints > max_point.  With c candidates at z
 *            <= th_depth that lists min(n_cand, max(c, max_point) + 1) entries: max_point + 1 where few are close, not the
 *            max_point the source's comment promises.
 * What stays with the caller: cv::undistortPoints for non-zero distortion (pass pt_un); the N > 500 test of
 * StereoInitialization; MapPoint and KeyFrame construction, track ids, UpdateNormalAndDepth (movba_point_normals);
 * AssignFeaturesToGrid; the fisheye branches (Nleft != -1), which never run in this fork.
 * A frame's result depends on that frame's data alone - the same frame alone or in any batch gives the same bits - and two calls
 * give the same bits.
 * Returns MOVBA_ERR_ARG for a NULL handle, descriptor or result; n_frames negative or above MOVBA_MAX_EXPRESS_IMAGES; pt_ptr NULL
 * or not ascending from 0; more than MOVBA_MAX_STEREO_POINTS points in a frame; n_pt above MOVBA_MAX_EXPRESS_ITEMS; a NULL array
 * that the counts make necessary (rows, cols, bf, max_disparity, th_depth, cam, select always; pt, next_pt, pt_status when n_pt
 * > 0), or a NULL result array; rows or cols < 1; a select outside 0 .. 2; max_point < 0; bf, max_disparity, th_depth, cam,
 * max_row_diff or min_disparity that is not finite, or fx, fy or bf <= 0; a pt or pt_un that is not finite or above 2^20 in
 * magnitude; a next_pt of a point with pt_status != 0 that is not finite or above 2^20 in magnitude (so that the truncation to
 * int is defined); a pose entry that is not finite, or a zero quaternion.  MOVBA_ERR_HIP as elsewhere.  Every argument is checked
 * before anything is queued, and on a non-zero status nothing is written except `status`.  n_frames == 0: MOVBA_OK and nothing
 * else written.
 * One packed copy to the device, two launches - k_st_frame (a workgroup per frame: the gates, the exact upper median by a radix
 * select over the int distances, the pruning, and the selection - a compaction in index order or a bitonic sort of 8-byte keys,
 * the depth's bits above the index, in LDS) and k_st_emit (sel_ptr from the frames' counts, the selected points' rows, the
 * padding) - and one synchronisation; result arrays that lie in movba_host_alloc memory are written by the kernels themselves.
 * May share a handle with an uploaded or solved window, waiting for the window's arrays before it reuses the staging buffer:
 * the window, its results, its marginals and later runs stay as they were. */
int  movba_stereo_points(movba_handle *h, const movba_stereo_desc *desc, movba_stereo_result *res);

#ifdef __cplusplus
}
#endif
#endif /* MOVBA_H */
