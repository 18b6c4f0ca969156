/*
 * psba_hip.h -- C ABI of the MI355X-native Schur-complement bundle-adjustment
 * normal-equations path (drop-in for the operator layer of eglrp/PSBA).
 *
 * What it replaces (paths relative to the reference checkout):
 *   PSBA/sba_func.h:10-138      the per-kernel host wrappers called by levmar()/trust_region()
 *   PSBA/cl_spdinv.h:7-18       SPDinv / cholesky / trigMat_inv / trigMat_mul
 *   PSBA/cl_linearalg.h:8-9     matVec_mul
 *   PSBA/cl_psba.h:9-126        PSBA_struct, setup_cl, fill_initBuffer2, fill_idxBuffer,
 *                               release_buffer
 *   PSBA/misc.cpp:178-217       generate_idxs (dense blk_idx/comm3DIdx tables -> CSR inside)
 *   PSBA/levmar.cpp:45-256      levmar() (restated over this ABI as psba_levmar)
 *   PSBA/readparams.cpp:444-519 readInitialSBAEstimate (restated as psba_read_problem)
 *
 * Conventions are the reference's: cnp = 6 (local-quaternion vector part 3 + translation 3),
 * pnp = 3, mnp = 2 (CL_files/PSBA.cl:5-7); all arithmetic fp64; K[5] = (fu,u0,v0,ar,s) per
 * camera, held fixed; initrot = unit quaternion, scalar first; observations sorted
 * point-major, camera ascending inside a point (PSBA/misc.cpp:189-216).
 *
 * Plain pointers and sizes only.  Host arrays are owned by the caller; everything on the
 * device is owned by the opaque handle.  One handle = one GPU = one host thread.  Calls
 * are asynchronous on the handle's stream and synchronise only where a value is returned
 * to the host.  No call exits the process: every entry point returns an int status
 * (0 ok, > 0 numerical, < 0 API / usage error) and psba_last_error() gives the text.
 */
#ifndef PSBA_HIP_H
#define PSBA_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psba_ctx *psba_handle;

/* ---- status codes ------------------------------------------------------------------- */
#define PSBA_OK 0
#define PSBA_NOT_SPD 1     /* Cholesky met a non-positive / non-finite pivot (SPDinv ret==1.0,
                              PSBA/cl_spdinv.cpp:85-102, CL_files/SPD_inv.cl:35-38,66) */
#define PSBA_SINGULAR_V 2  /* some |det V_i| < 1e-16 (compute_Vinv ret==1.0,
                              CL_files/compute_Vinv.cl:31-32) */
#define PSBA_PCG_MAXIT 4   /* psba_schur_solve under PSBA_SOLVER_PCG: max_iter iterations without reaching
                              tol; dpa holds the last iterate (an inexact step), psba_pcg_info the residual */
#define PSBA_E_INVALID (-1)
#define PSBA_E_HIP (-2)
#define PSBA_E_RCCL (-3)
#define PSBA_E_IO (-4)
#define PSBA_E_NOMEM (-5)
#define PSBA_E_STATE (-6)  /* verb called before the state it needs exists */

/* iteration flags of the optimiser loops, PSBA/psba.h:12-18 (same numbering) */
#define PSBA_ITER_TURN_TO_LM 1
#define PSBA_ITER_TURN_TO_TR 2
#define PSBA_ITER_CONTINUE 3
#define PSBA_ITER_ERR 4
#define PSBA_ITER_DP_NO_CHANGE 5
#define PSBA_ITER_ERR_SMALL_ENOUGH 6
#define PSBA_ITER_PASS 7

/* which parameter set a verb evaluates: cams_buffer/pts3D_buffer or
 * newCams_buffer/newPts3D_buffer (PSBA/sba_func.h:15-16, PSBA/levmar.cpp:93,188-189) */
#define PSBA_PARAMS_CUR 0
#define PSBA_PARAMS_NEW 1

/* ---- lifecycle: setup_cl / release_buffer (PSBA/cl_psba.h:93-94) --------------------- */
int psba_create(int device, psba_handle *out);
int psba_destroy(psba_handle h);
/* text of the last error on this handle (h may be NULL: last error of a failed create) */
const char *psba_last_error(psba_handle h);
/* version string of the library and the code-object architecture it was built for */
const char *psba_version(void);

/* ---- problem upload: fill_initBuffer2 + generate_idxs + fill_idxBuffer ----------------
 * (PSBA/cl_psba.h:114-126, PSBA/misc.cpp:178-217, call order PSBA/main.cpp:177-189).
 * Kparas[nCams*5], impts[n2Dprojs*2], initrot[nCams*4], camsEx[nCams*6], pts3D[n3Dpts*3],
 * iidx/jidx[n2Dprojs] (point / camera of each observation, point-major sorted).
 * The dense blk_idx / comm3DIdx tables of the reference are not needed: a point CSR and
 * point-aligned observation tiles are built inside. */
int psba_upload_problem(psba_handle h, int nCams, int n3Dpts, int n2Dprojs, const double *Kparas,
                        const double *impts, const double *initrot, const double *camsEx,
                        const double *pts3D, const int *iidx, const int *jidx);
/* overwrite the current parameters (cams[nCams*6], pts[n3Dpts*3]) */
int psba_set_params(psba_handle h, const double *camsEx, const double *pts3D);
/* back to the parameters given to psba_upload_problem (device-side copy, no synchronisation):
 * what a driver that reruns the loop from the same start, like bench.py, would otherwise do
 * with psba_set_params */
int psba_reset_params(psba_handle h);
/* read back the current (PSBA_PARAMS_CUR) or proposed (PSBA_PARAMS_NEW) parameters */
int psba_get_params(psba_handle h, int which, double *camsEx, double *pts3D);
int psba_get_dims(psba_handle h, int *nCams, int *n3Dpts, int *n2Dprojs);

/* ---- free intrinsics ---------------------------------------------------------------
 * The reference's driver reads 11 parameters per camera -- (fu, u0, v0, ar, s), quaternion -> local rotation,
 * translation (PSBA/main.cpp:73,140-149; data/54camsvarK.txt) -- and then strips the intrinsics: its kernels
 * optimise six (CL_files/PSBA.cl:5-7).  PSBA_CAMERA_FREE_K optimises all eleven: the camera block becomes
 * (fu, u0, v0, ar, s | v0, v1, v2 | t0, t1, t2), nA = 11 nCams, dp = [11 per camera ; 3 per point].
 * psba_upload_problem takes the same arrays (Kparas and camsEx are joined inside); psba_get_params /
 * psba_set_params then move 11 doubles per camera.  The route is PSBA_CAMERA_FREE_KD's (kernels_free.hip, templated on
 * the block: a 16 x 16 MFMA tile with five idle rows and columns, no floating-point atomics, two runs bit-identical;
 * psba_schur_path = 5), single rank, dense solver; the fused verbs and psba_levmar work, the
 * sba_func.h mirror, the trust-region operators and psba_solve return PSBA_E_STATE.  The reference has no
 * arithmetic for this (it never implemented it): PARITY UNPINNED -- checked against the oracle's twin, finite
 * differences and a dense solve of the full normal equations.  Before psba_upload_problem. */
#define PSBA_CAMERA_FIXED_K 0
#define PSBA_CAMERA_FREE_K 1
#define PSBA_CAMERA_FREE_KD 2
int psba_set_camera_model(psba_handle h, int model);
int psba_camera_block(psba_handle h, int *cnp); /* 6, 11 or 16 */

/* ---- free intrinsics together with lens distortion ---------------------------------------
 * PSBA_CAMERA_FREE_KD optimises the five intrinsics and the five distortion coefficients with the pose: the camera
 * block is (fu, u0, v0, ar, s | k1, k2, k3, k4, k5 | v0, v1, v2 | t0, t1, t2), nA = 16 nCams, dp = [16 per camera ;
 * 3 per point]; psba_get_params / psba_set_params move 16 doubles per camera.  Model (the same in
 * psba_amd/csrc/camera_model.h and DESIGN.md; kc order and distortion as for psba_set_distortion below): with (x, y)
 * the normalised point, r2 = x^2 + y^2 and (xd, yd) the distorted point,
 *   d(u, v) / d(fu, u0, v0, ar, s) = [ xd, 1, 0, 0, yd ;  ar yd, 0, 1, fu yd, 0 ]
 *   d xd / d(k1..k5) = (r2 x, r2^2 x, 2 x y, r2 + 2 x^2, r2^3 x),  d yd / d(k1..k5) = (r2 y, r2^2 y, r2 + 2 y^2, 2 x y, r2^3 y)
 *   d u / dk = fu d xd + s d yd,  d v / dk = fu ar d yd;  the extrinsic columns and B as with fixed distortion.
 * Starting distortion: under this model psba_set_distortion(h, kc) is allowed after psba_upload_problem and sets the
 * starting kc -- columns 5..9 of the current parameters and of the copy psba_reset_params restores (an upload starts
 * from zeros, NULL means zeros); it discards a linearization queued ahead and returns PSBA_E_STATE while a try is in
 * flight.  psba_lens_model reports has_distortion = 1.
 * Per-parameter mask: free10[k] != 0 = intrinsic k (order fu, u0, v0, ar, s, k1..k5) is optimised, 0 = it is held at
 * its current value on every camera.  NULL = all ten free; all ten zero is legal (extrinsics only); the problem of
 * Bundle Adjustment in the Large is {fu, k1, k2}.  After psba_upload_problem (a new upload resets to all free);
 * PSBA_E_STATE under another camera model and while a try is in flight; a refused call changes nothing; setting the
 * mask discards a linearization queued ahead.  Semantics as for fixed blocks, per coordinate: the column
 * of A is zero, the stored diagonal entry of U_j is the placeholder coeff, g and dp are exactly 0, the proposed and
 * accepted values are bit-identical to the current ones, psba_max_diag / psba_begin take the maximum over the free
 * entries, row and column of S are zero off the diagonal with coeff + mu on it, and e_a is 0.
 * Route (kernels_free.hip, psba_schur_path = 5): camera-major linearization and S assembly on
 * v_mfma_f64_16x16x4_f64, no floating-point atomics -- two runs give bit-identical reduce buffers and logs.  Single
 * rank; the dense solver, or PSBA_SOLVER_SPARSE (psba_set_solver: the same assembly into a block-sparse S,
 * psba_schur_path = 6).  The fused verbs, psba_levmar, psba_get_dp, psba_get_gradient and psba_get / set_reduce_buffer
 * work; covariances, robust losses, psba_set_fixed, PSBA_SOLVER_PCG, rank layouts, the sba_func.h mirror, the
 * trust-region operators, psba_solve and psba_obs_sq_residuals return PSBA_E_STATE with a text that names
 * PSBA_CAMERA_FREE_KD.  The reference has no arithmetic for this: PARITY UNPINNED -- checked against a numpy twin,
 * central differences and a dense solve of the full normal equations. */
int psba_set_intrinsics_mask(psba_handle h, const unsigned char free10[10]);
int psba_intrinsics_mask(psba_handle h, unsigned char out10[10]);

/* ---- per-camera masks of the ten intrinsics (PSBA_CAMERA_FREE_KD) ------------------------------
 * Mixed jobs: some cameras calibrated (a rig, a lab calibration), some not; new images added to a finished
 * reconstruction; images that must stay where they are.  free10_per_cam [10 nCams], row j = camera j, order (fu, u0,
 * v0, ar, s, k1..k5), non-zero = optimised.  Intrinsic k of camera j is optimised iff psba_set_intrinsics_mask frees k
 * AND row j frees k; psba_intrinsics_mask keeps returning the global ten flags.  NULL, or a table with no zero entry,
 * is no table: the handle then runs the code of one that never called this and produces the same bits.
 * A coordinate that is not optimised is, bit for bit, what a coordinate masked by psba_set_intrinsics_mask is: the
 * column of A is zero; W, U off the diagonal, g_a, e_a and dp are exactly 0; the placeholder coeff is on the diagonal
 * of U and coeff + mu (coeff + mu D) on that of S; psba_max_diag / psba_begin skip it; its row and column of a camera
 * prior are dropped while the gradient of the free coordinates takes the whole d; the proposal carries the current
 * bits; the cost is untouched.  A camera with no free intrinsic and a held pose (psba_set_held) is a wholly fixed
 * camera; nothing else is needed for one.  Under PSBA_SOLVER_SPARSE its diagonal block and the inverse the
 * preconditioner keeps are diagonal.  psba_free_covariance_compute returns exact zeros in the rows and columns of a
 * masked coordinate, and sigma 0.
 * Groups: the members of a group with more than one camera carry equal rows -- whichever of psba_set_camera_masks and
 * psba_set_intrinsics_groups is called second checks it before it touches the device and returns PSBA_E_INVALID with
 * the first offending camera and coordinate.  A shared coordinate is then free or masked for the whole group.
 * The table composes in either order with the global mask, held poses and points, priors, the observation weighting,
 * the damping rule and both solvers.  After psba_upload_problem (a new upload resets to no table); PSBA_E_STATE under
 * another camera model (blocks of 11 have no mask) and while a try is in flight; a refused call changes nothing;
 * setting the table discards a linearization queued ahead and invalidates psba_get_free_obs_blocks and
 * psba_get_damping_diag.  No floating-point atomics: two runs stay bit-identical.  psba_camera_masks: the table as
 * set, 0 / 1 per entry; all ones when there is none. */
int psba_set_camera_masks(psba_handle h, const unsigned char *free10_per_cam /* 10 nCams */);
int psba_camera_masks(psba_handle h, unsigned char *out10_per_cam /* 10 nCams */);

/* ---- intrinsics shared between cameras (PSBA_CAMERA_FREE_KD) ----------------------------------
 * One physical camera takes many images: group_of_cam[j] is any int, cameras with equal labels share their ten
 * intrinsics (fu, u0, v0, ar, s, k1..k5).  The representative rep(j) of a group is its lowest camera index; P maps
 * the reduced parameters to the per-camera ones (a free intrinsic coordinate k of a member j takes the value of
 * coordinate k of rep(j)), J_shared = J P, and because P leaves the points alone the Schur complement commutes with it:
 *   S_shared = P^T (U - W (V + mu I)^-1 W^T) P + mu I,   e_a,shared = P^T e_a.
 * The fold is stored embedded in the full-size system (nA = 16 nCams stays): row and column of a free intrinsic
 * coordinate of a representative are the sums of its members' rows and columns in ascending camera order, mu added
 * once after the sum; a free intrinsic coordinate of a non-representative member becomes what a masked coordinate is
 * (zero off the diagonal, coeff + mu on it, e_a = 0).  Coordinates held by psba_set_intrinsics_mask stay held on every
 * camera and are not summed; mask and groups compose in either order.  After the solve the representative's dp is
 * copied to its members: psba_get_dp returns the expanded per-camera step, and members that start bit-identical stay
 * bit-identical.  Every reduction counts a shared parameter once: psba_max_diag / psba_begin take the maximum over the
 * folded diagonal of U (the group sum for shared coordinates, free entries only); dp_l2 and newp_l2 skip the
 * intrinsic entries of non-representatives; gain_den = sum over all entries of dp g + mu times the sum over the
 * distinct parameters of dp^2.  psba_get_gradient keeps returning the per-camera g: the sum over a group is the
 * derivative with respect to the shared parameter.  psba_get_reduce_buffer returns the folded, embedded [S | e_a].
 * NULL or a labelling in which every camera is alone is no grouping: the handle runs exactly the kernels of one that
 * never set any.  Members must hold bit-identical intrinsics (columns 0..9) in the current parameters and in the copy
 * psba_reset_params restores: PSBA_E_INVALID names the first offending camera and column; while groups are set
 * psba_set_params and psba_set_distortion make the same check on their host arrays before touching the device.
 * After psba_upload_problem (a new upload resets to none); PSBA_E_STATE under another camera model and while a try is
 * in flight; a refused call changes nothing; setting groups discards a linearization queued ahead.  No floating-point
 * atomics: two runs stay bit-identical.  psba_intrinsics_groups: rep_of_cam[j] = rep(j) (j itself without groups;
 * may be NULL) and the number of groups (nCams without groups). */
int psba_set_intrinsics_groups(psba_handle h, const int *group_of_cam);
int psba_intrinsics_groups(psba_handle h, int *rep_of_cam, int *n_groups);
/* ---- ... under PSBA_SOLVER_SPARSE on blocks of 16 ----
 * The same model, labels, checks and state rules as psba_set_intrinsics_groups, on a PSBA_SOLVER_SPARSE handle, where
 * that verb keeps returning PSBA_E_STATE; on any other handle this one returns PSBA_E_STATE with a text that names
 * psba_set_intrinsics_groups.  Nothing is folded into the stored blocks.  Conjugate gradients need only the product
 *     A x = P^T (S0 (P x)) + mu D x
 * (P copies a representative's shared coordinates to its members, S0 is the undamped list, P^T sums over the members
 * in ascending camera order), so with groups set
 *   * psba_schur_assemble stores S0, the unfolded blocks WITHOUT damping, and the folded e_a (a representative's shared
 *     entry is the sum over its members in ascending order, as on the dense route and with its bits; folded-away
 *     entries are 0);
 *   * psba_get_sparse_S / psba_set_sparse_S return and take these two objects (entries of ea at folded-away
 *     coordinates are taken as 0);
 *   * psba_schur_solve runs the recurrences, the stop rule and the bursts of the ungrouped solve on the embedded
 *     operator: the search direction is kept expanded, a launch behind the block product folds q and adds mu D p.
 *     mu and D are those of the last psba_schur_assemble.  The preconditioner is the block Jacobi of A: the diagonal
 *     block of a representative is the folded one (cross-member blocks included), a folded-away coordinate is
 *     coeff + mu D on the diagonal and zero elsewhere;
 *   * psba_sparse_S_times returns A x for the embedded A (entries of x at folded-away coordinates meet their
 *     placeholder alone: y = (coeff + mu D) x there);
 *   * psba_sparse_camera_covariance, psba_sparse_point_covariance and psba_sparse_S_times_many return PSBA_E_STATE
 *     with a text that names this verb: covariance under groups is not supported.
 * The step is expanded and every reduction counts a shared parameter once, as on the dense route.  NULL or a labelling
 * in which every camera is alone clears the tables: the handle then launches exactly what one that never called the
 * verb launches, and gives the same bits.  No floating-point atomics: two runs stay bit-identical. */
int psba_set_sparse_intrinsics_groups(psba_handle h, const int *group_of_cam);

/* ---- the damping rule of the free-intrinsics models (PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD) --------
 * A camera block with free intrinsics mixes scales: the diagonal of J^T J runs from about 1 (a focal length in
 * pixels) to 1e7 (a rotation), and mu I with mu_0 = 1e-3 max diag freezes the small entries until mu has come down.
 * PSBA_DAMPING_MARQUARDT damps with N + mu D instead, D_k = min(max(N_kk, dmin), dmax) (Marquardt's scaling, with the
 * clamps production solvers use).  N_kk is the stored diagonal of the linearization: U_j[k][k] for cameras (scaled by
 * coeff; the placeholder coeff of a coordinate held by psba_set_intrinsics_mask), the diagonal of V_i for points.
 * dmin = 0 / dmax = 0 mean the defaults 1e-6 / 1e32; otherwise 0 < dmin <= dmax, both finite.  PSBA_E_INVALID for
 * other clamps and for an unknown kind.
 * What the fused verbs do with mu: in psba_schur_assemble(mu), psba_backsub(mu) and psba_backsub_async(mu) it
 * multiplies D -- the point system is V_i + mu diag(D_i), the camera diagonal U_kk + mu D_k,
 * gain_den = sum dp g + mu sum D dp^2, and psba_get_reduce_buffer returns that S.  psba_max_diag and psba_begin are
 * unchanged.  With psba_set_intrinsics_groups mu D is added once, after the fold: D of a shared coordinate of a
 * representative is the clamp of the sum of its members' U_kk in ascending camera order (the folded diagonal
 * psba_max_diag takes its maximum over), D of a folded-away coordinate of a non-representative is clamp(coeff), as
 * for a masked one, and the mu sum D dp^2 term counts a shared parameter once.  Mask, groups and damping compose in
 * any order of calls.  psba_levmar under Marquardt starts from mu_0 = tau (see psba_lm_options.init_mu) and is
 * otherwise the same loop.
 * After psba_upload_problem (a new upload resets to PSBA_DAMPING_IDENTITY with the default clamps); PSBA_E_STATE
 * before an upload, while a try is in flight and on six-parameter camera blocks (free-intrinsics models only: the
 * fixed-K routes keep the reference's N + mu I); a refused call changes nothing; setting the rule discards a
 * linearization queued ahead.  PSBA_DAMPING_IDENTITY is bit for bit the handle that never called this, also after a
 * Marquardt run on the same handle.  No floating-point atomics: two runs stay bit-identical.  PARITY UNPINNED, like
 * the models it belongs to. */
#define PSBA_DAMPING_IDENTITY  0   /* N + mu I: the reference's rule, the default */
#define PSBA_DAMPING_MARQUARDT 1   /* N + mu D, D_k = min(max(N_kk, dmin), dmax) */
int psba_set_damping(psba_handle h, int kind, double dmin, double dmax);
int psba_damping(psba_handle h, int *kind, double *dmin, double *dmax);

/* ---- held poses and points of the free-intrinsics models (PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD) ----
 * Without held blocks S is singular at mu = 0 on these models (the gauge is free): no Gauss-Newton step, no
 * reference frame, no control points.  held_poses[j] != 0 holds the POSE of camera j -- the six pose coordinates, the
 * last six of its block (indices NI .. CNP-1, NI = 5 / 10) -- and held_pts[i] != 0 the three coordinates of point i.
 * The camera's intrinsics stay under psba_set_intrinsics_mask and psba_set_intrinsics_groups: one physical camera
 * whose first two poses fix the gauge is the common case, which holding whole blocks would forbid.  psba_set_fixed
 * keeps refusing both models, and so does psba_covariance_compute.
 * Model.  The problem solved is the reduced one (the held columns of J deleted, the held values constants of the
 * residual), stored embedded in the full-size system; per held coordinate exactly what a coordinate held by
 * psba_set_intrinsics_mask is: the column of A is zero for a held pose coordinate and B is zero for a held point, applied
 * before W = coeff A^T B, so the W rows (the whole W of a held point) are exactly 0; the stored diagonal entry of U_j
 * or V_i is the placeholder coeff and the off-diagonal entries of a held V_i are 0; g and dp are exactly 0; the
 * proposed and the accepted values are bit-identical to the current ones; psba_max_diag / psba_begin take the maximum
 * over the free entries; row and column of S are zero off the diagonal with coeff + mu on it (coeff + mu clamp(coeff)
 * under PSBA_DAMPING_MARQUARDT: D is the clamp of the stored diagonal); e_a is 0.  The cost is untouched: every
 * observation counts, and a held point's observations enter new_cost at the moved cameras.  psba_set_params may still
 * move a held block.  Held blocks, mask, groups and damping compose in any order of calls (the fold of the groups
 * touches intrinsic coordinates only).
 * NULL = none of that kind, two NULLs clear the masks; a mask without a non-zero entry is no mask: the handle then
 * runs the kernels of one that never called this and produces the same bits.  After psba_upload_problem (a new upload
 * resets to none); PSBA_E_STATE before an upload, while a try is in flight and on six-parameter camera blocks (those
 * are held as a whole by psba_set_fixed); PSBA_E_INVALID if every pose and every point would be held (a resection of
 * the intrinsics alone is not supported); a refused call changes nothing; setting the masks discards a linearization
 * queued ahead and invalidates psba_get_free_obs_blocks and psba_get_damping_diag.  No floating-point atomics: two
 * runs stay bit-identical.  PARITY UNPINNED, like the models it belongs to.  psba_held_counts: the numbers of held
 * poses and points (either pointer may be NULL). */
int psba_set_held(psba_handle h, const unsigned char *held_poses /* nCams */, const unsigned char *held_pts /* n3Dpts */);
int psba_held_counts(psba_handle h, int *n_held_poses, int *n_held_pts);

/* ---- Gaussian priors on cameras and points of the free-intrinsics models ----
 * Between leaving a parameter free and freezing it: a focal length known to a few percent, a principal point near the
 * image centre, k3..k5 pulled towards zero, a GPS position per camera, surveyed control points with a deviation.
 * Model.  A camera j may carry a mean m_j [cnp], in the order of the camera block as psba_get_params returns it, and
 * a symmetric positive semi-definite information matrix L_j [cnp x cnp] (the inverse covariance); a point i n_i [3]
 * and G_i [3 x 3].  A diagonal L = diag(1 / sigma^2) is the common case; full blocks allow correlated knowledge.  With
 * d = m - p, the sign convention of e = measured - projected, the cost is
 *     F = sum_a |e_a|^2 + sum_j d_j^T L_j d_j + sum_i d_i^T G_i d_i
 * The priors are extra residual rows: psba_residual, psba_begin, new_cost of the try scalars and the costs of
 * psba_levmar's log and result are all F, and stop_cost tests F.  The rotation coordinates of a block are the local
 * rotation about the uploaded initrot: a prior with mean 0 on them says "stay near the starting rotation".
 * Normal equations, with coeff and coeff_g those of psba_linearize and s the sums over the observations:
 *     U_j[r][c] = coeff (s_rc + L_j[r][c])      g_a,j[r] = coeff_g (s_r + sum_c L_j[r][c] d_j[c])
 * the inner sum in ascending c, d at the parameter set being linearized (the proposal for psba_linearize_ahead);
 * points the same with G_i: the six stored entries of V_i, and g_b,i.  psba_max_diag / psba_begin, Marquardt's D, Y, S,
 * e_a, the back-substitution and gain_den run on the stored U, V, g, prior included.  Under
 * psba_set_intrinsics_groups the fold sums the members' rows and columns: a shared intrinsic gets the sum of its
 * members' priors, and psba_get_gradient keeps returning the per-camera g.
 * Held coordinates (mask, psba_set_held, folded away by the groups): the held column is deleted from the prior rows
 * too -- row and column of L (G) are dropped from U (V) before the placeholder coeff goes on the diagonal, g, e_a and
 * dp stay exactly 0 there -- while the gradient of a free coordinate uses the full d, (L d)_free, and the cost always
 * counts the full quadratic form.  Every exact guarantee of the mask, the groups, the damping and the holds keeps
 * holding with priors set.
 * cam_mean [nCams cnp], cam_info [nCams cnp cnp] row-major; pt_mean [n3Dpts 3], pt_info [n3Dpts 9].  The mean and the
 * information of a kind are both NULL or both given (PSBA_E_INVALID otherwise); four NULLs clear the priors.  A block
 * whose information is all zero has no prior; psba_prior_counts counts the others (either pointer may be NULL).  If
 * no block has a prior the handle runs the kernels of one that never called this and produces the same bits.
 * After psba_upload_problem (a new upload resets to none); PSBA_E_STATE before an upload, while a try is in flight and
 * on six-parameter camera blocks; PSBA_E_INVALID, naming the first offending camera or point and entry, for a
 * non-finite entry, a negative diagonal entry and a block that is not symmetric to 1e-12 relative to its largest
 * entry (the rule of psba_set_obs_covariance; the two halves are averaged).  Positive semi-definiteness beyond that is
 * the caller's contract: an indefinite block may surface as PSBA_NOT_SPD.  A refused call changes nothing.  Setting
 * priors discards a linearization queued ahead and invalidates psba_get_damping_diag and psba_get_free_obs_blocks.
 * psba_set_params / psba_reset_params move the parameters, not the means.  Priors, mask, groups, damping and holds
 * compose in any order of calls.  No floating-point atomics: every new sum has an order the upload fixes, two runs are
 * bit-identical.  PARITY UNPINNED, like the models it belongs to.
 * psba_prior_cost: the two prior sums of F at PSBA_PARAMS_CUR / PSBA_PARAMS_NEW (either pointer may be NULL);
 * synchronises; PSBA_E_STATE while a try is in flight (it shares the try's reduction scratch). */
int psba_set_priors(psba_handle h, const double *cam_mean, const double *cam_info, const double *pt_mean,
                    const double *pt_info);
int psba_prior_counts(psba_handle h, int *n_cam_priors, int *n_pt_priors);
int psba_prior_cost(psba_handle h, int which, double *cams_part, double *pts_part);

/* ---- observation weighting on the free-intrinsics models: robust loss and sigmas ----
 * Real tracks carry mismatches, and a plain least-squares self-calibration is ruined by them.  psba_set_robust_loss,
 * psba_set_obs_covariance and psba_obs_sq_residuals keep refusing these models; this verb is their counterpart here.
 * Model (the same in psba_amd/csrc/kernels_free.hip and DESIGN 7k).  Observation a may carry a standard deviation
 * sigma_a > 0; without sigmas sigma_a = 1.  A loss (kind, c) may be set, with the kinds, formulas and conventions of
 * the robust losses below (PSBA_LOSS_*).  With e_a the route's residual:
 *     s_a = |e_a / sigma_a|^2        F = sum_a rho(s_a) + the priors' two sums (the priors are not weighted)
 * IRLS without the rho'' term: omega_a = sqrt(rho'(s_a)).  The kernel first multiplies e, both rows of A, and B by
 * 1 / sigma_a (the reciprocal is stored once at the setter) and then by omega_a: two roundings per entry.  Everything
 * behind the per-observation blocks reads the weighted blocks and is otherwise unchanged: W, Be, U, g_a, V, g_b, D of
 * Marquardt, Y, S, e_a, the fold of the groups, the back-substitution and gain_den.  A zeroed column stays zero under
 * the scaling, so every exact guarantee of the mask, the groups, the damping, the holds and the priors keeps holding.
 * psba_residual, psba_begin, new_cost of the try and the costs and stop_cost of psba_levmar are all F;
 * psba_get_free_obs_blocks returns the weighted W and B | e.  psba_linearize_ahead takes its weights at the proposal.
 * sigma [n2Dprojs] in the uploaded observation order, or NULL.  (PSBA_LOSS_NONE, any scale, NULL) is no weighting: the
 * handle then runs the kernels of one that never called this and produces the same bits, also after a weighted run.
 * After psba_upload_problem (a new upload resets to (PSBA_LOSS_NONE, 1, no sigmas)); PSBA_E_STATE before an upload,
 * while a try is in flight and on six-parameter camera blocks (those have psba_set_robust_loss /
 * psba_set_obs_covariance); PSBA_E_INVALID for an unknown kind, for a scale that is not finite and > 0 (checked for
 * every kind) and for a sigma that is not finite and > 0 (the text names the first offending observation).  A refused
 * call changes nothing.  Setting the weighting discards a linearization queued ahead and invalidates
 * psba_get_free_obs_blocks and psba_get_damping_diag.  No floating-point atomics: two runs are bit-identical.
 * Still refused on these models: full 2 x 2 observation covariances, psba_covariance_compute, PSBA_SOLVER_PCG, rank
 * layouts and the sba_func.h mirror.  PARITY UNPINNED, like the models it belongs to.
 * psba_obs_weighting: what is set (any pointer may be NULL).
 * psba_get_obs_weights: s[n2Dprojs], w[n2Dprojs] (either may be NULL) at PSBA_PARAMS_CUR / PSBA_PARAMS_NEW, uploaded
 * observation order: s_a as above, w_a = omega_a / sigma_a, the factor the blocks were multiplied by.  Works with no
 * weighting set (s = |e|^2, w = 1).  Synchronises.  PSBA_E_STATE on six-parameter blocks, while a try is in flight,
 * and for PSBA_PARAMS_NEW without a proposal. */
int psba_set_obs_weighting(psba_handle h, int loss_kind, double loss_scale, const double *sigma /* n2Dprojs or NULL */);
int psba_obs_weighting(psba_handle h, int *loss_kind, double *loss_scale, int *has_sigma);
int psba_get_obs_weights(psba_handle h, int which, double *s, double *w);

/* ---- lens distortion and per-observation image covariances --------------------------
 * Model (the same in psba_amd/csrc/camera_model.h and DESIGN.md): P = R'(q) M + t, (x, y) = (Px, Py) / Pz,
 * r2 = x^2 + y^2, kc = (k1, k2, k3, k4, k5) in the Camera Calibration Toolbox order (the column order of the
 * 17-column sba cams files: K5, kc(1:5), quaternion, translation):
 *   radial = 1 + k1 r2 + k2 r2^2 + k5 r2^3
 *   xd = radial x + 2 k3 x y + k4 (r2 + 2 x^2),   yd = radial y + k3 (r2 + 2 y^2) + 2 k4 x y
 *   u = fu xd + s yd + u0,   v = fu ar yd + v0,   e = m - (u, v)
 * Covariances: observation a has an SPD 2x2 Sigma_a and the cost is sum e_a^T Sigma_a^-1 e_a.  The library
 * factors Sigma_a^-1 = L_a^T L_a (L_a upper triangular) once, here, and the kernels whiten right after the
 * projection (e <- L e, A <- L A, B <- L B).  Every verb then works on the whitened quantities: psba_residual,
 * the try scalars and the loop logs report the weighted cost, and psba_compute_exQT / psba_compute_jacobiQT
 * (and the U, V, W, g, S, e_a of the mirror) return the whitened e, A and B.
 * The fixed-intrinsics camera block only: PSBA_E_STATE before psba_upload_problem and under PSBA_CAMERA_FREE_K
 * (under PSBA_CAMERA_FREE_KD psba_set_distortion sets the starting kc instead, see above; covariances are refused).
 * Call after psba_upload_problem (a new upload resets both to none), while no try is in flight; setting either
 * discards a linearization queued ahead.  The reference reads both and uses neither (PSBA/readparams.cpp:272-283,
 * 380-412; PSBA/main.cpp:112): PARITY UNPINNED -- checked against an independent numpy twin that is itself pinned to
 * the oracle where the models coincide (kc = 0, Sigma = I). */
/* kc: nCams * 5 (camera order of the upload); NULL = no distortion */
int psba_set_distortion(psba_handle h, const double *kc);
/* cov: n2Dprojs * 4 (row-major 2x2 per observation, in the uploaded observation order; under a rank layout, this
 * rank's observations); NULL = none.  PSBA_E_INVALID for a Sigma that is not SPD or not symmetric to 1e-12
 * relative (the error text names the observation) */
int psba_set_obs_covariance(psba_handle h, const double *cov);
int psba_lens_model(psba_handle h, int *has_distortion, int *has_covariance);

/* ---- robust losses --------------------------------------------------------------------
 * Model (the same in psba_amd/csrc/camera_model.h and DESIGN.md): s_a = ||L_a e_a||^2 is the whitened squared
 * residual (L_a = I without covariances) and the cost becomes F = sum_a rho(s_a).  The scale c > 0 is in whitened
 * units (pixels when Sigma = I), c2 = c^2:
 *   PSBA_LOSS_NONE     rho = s                                          rho' = 1
 *   PSBA_LOSS_HUBER    rho = s if s <= c2, else 2 c sqrt(s) - c2          rho' = 1, else c / sqrt(s)
 *   PSBA_LOSS_CAUCHY   rho = c2 log(1 + s / c2)                           rho' = 1 / (1 + s / c2)
 *   PSBA_LOSS_SOFT_L1  rho = 2 c2 (sqrt(1 + s / c2) - 1)                  rho' = 1 / sqrt(1 + s / c2)
 * rho(0) = 0 and rho'(0) = 1 for every loss (no 1/2, the reference's convention).  The normal equations are those
 * of weighted Gauss-Newton (IRLS): w_a = sqrt(rho'(s_a)) after the whitening, e <- w e, A <- w A, B <- w B, so
 * g = A~^T e~ is the gradient of F (halved, in the sign convention of g).  The rho'' term of the Hessian is left
 * out (negative for these losses: it would break positive definiteness).  psba_residual, the try scalars and the
 * loop logs report F; the LM gain ratio compares the drop of F with the drop the weighted model predicts.
 * The mirror verbs return what the normal equations see: psba_compute_exQT w L e, psba_compute_jacobiQT w L A and
 * w L B, psba_compute_Jmultiply J~ x.
 * Rules as for the lens model above: PSBA_E_STATE before psba_upload_problem, under PSBA_CAMERA_FREE_K and while a
 * try is in flight; PSBA_E_INVALID for an unknown kind or a scale that is not finite and > 0 (checked for every
 * kind).  Setting a loss discards a linearization queued ahead; an upload resets it to PSBA_LOSS_NONE with scale 1.
 * PSBA_LOSS_NONE runs exactly the kernels of a handle that never set a loss.  The reference has no robust loss:
 * PARITY UNPINNED -- checked against a numpy twin, finite differences and a dense solve. */
#define PSBA_LOSS_NONE 0
#define PSBA_LOSS_HUBER 1
#define PSBA_LOSS_CAUCHY 2
#define PSBA_LOSS_SOFT_L1 3
int psba_set_robust_loss(psba_handle h, int kind, double scale);
int psba_robust_loss(psba_handle h, int *kind, double *scale);
/* s[n2Dprojs]: s_a = ||L_a e_a||^2 of each of this rank's observations (uploaded order) at the current
 * (PSBA_PARAMS_CUR) or proposed (PSBA_PARAMS_NEW) parameters, under any loss: observations with s_a well above c2
 * are the ones the loss down-weights.  Fixed-intrinsics camera block only. */
int psba_obs_sq_residuals(psba_handle h, int which, double *s);

/* ---- fixed parameter blocks -------------------------------------------------------------
 * Model (the same in psba_amd/csrc/camera_model.h and DESIGN.md): cameras and points marked fixed are held constant.
 * The problem solved is the reduced one: the columns of J that belong to fixed blocks are deleted and the fixed
 * values enter the residual as constants.  It is stored embedded in the full-size system, so no plan, index table or
 * buffer size changes:
 *   linearization  A_ij = 0 for a fixed camera j, B_ij = 0 for a fixed point i (after the whitening and the loss
 *                  weight), hence W_ij = 0 if either is fixed, g_a,j = 0 and g_b,i = 0 exactly.  The stored diagonal
 *                  block of a fixed camera (U_j) or point (V_i) is the placeholder coeff I (coeff of psba_linearize),
 *                  so V_i + mu I and S stay positive definite at mu = 0.  Under a rank layout only rank 0 (the rank
 *                  that owns the camera terms) writes the camera placeholder into its partial U, the others zero:
 *                  the summed diagonal block of a fixed camera is coeff I as on a single handle.
 *   psba_max_diag / psba_begin / psba_maxElmOfUV  the maximum over the free blocks only.
 *   S and e_a      block row and column j of a fixed camera are zero off the diagonal, the diagonal block is the
 *                  placeholder + mu I, e_a,j = 0.
 *   step           dp is exactly 0 on every fixed entry; the proposed and the accepted parameters of fixed blocks
 *                  are bit-identical to the current ones.  psba_set_step ignores (and zeroes) the fixed entries of dp.
 *   J x            psba_compute_Jmultiply / psba_jmul_dots use the masked J: fixed entries of x are not read.
 *   cost           psba_residual, the try scalars and psba_obs_sq_residuals count every observation as before.
 *   mirror verbs   return what the normal equations see: masked A, B, W, g, the placeholder blocks in U, V, S.
 *   psba_set_params may still move a fixed block: an explicit act of the caller.
 * fixed_cams[nCams], fixed_pts[n3Dpts]: non-zero = the parameter block is held constant.  NULL = none of that kind;
 * two NULLs clear the mask, and a mask without a non-zero entry is no mask: the handle runs exactly the kernels of
 * one that never set any.  Under a rank layout fixed_pts covers this rank's points (like cov), fixed_cams is the
 * same on every rank.
 * Rules as for the lens model above: PSBA_E_STATE before psba_upload_problem, under PSBA_CAMERA_FREE_K and while a
 * try is in flight; PSBA_E_INVALID if the mask would leave no free parameter at all on a single-rank handle.  A
 * refused call changes nothing.  Setting the mask discards a linearization queued ahead; an upload resets it to none.
 * Structure-only: when every camera is fixed there is no coupled system (dpa = 0, dpb_i = (V_i + mu I)^-1 g_b,i), and
 * psba_schur_assemble / psba_schur_reduce / psba_schur_solve queue no S assembly, no S-reduce and no factorization;
 * psba_get_reduce_buffer / psba_set_reduce_buffer / psba_get_sparse_S / psba_set_sparse_S then return PSBA_E_STATE
 * (nothing was assembled).  PSBA_FIXED_NO_SHORTCUT=1 in the environment keeps the general route; the mirror verbs
 * (psba_compute_S ...) always take it; psba_cholmod_lambda returns PSBA_E_STATE between the psba_schur_assemble and the
 * psba_schur_solve of a structure-only try.  The reference has no fixed blocks: PARITY UNPINNED -- checked against a
 * numpy twin, the oracle's own sums on masked blocks, finite differences and a dense solve of the reduced system. */
int psba_set_fixed(psba_handle h, const unsigned char *fixed_cams, const unsigned char *fixed_pts);
int psba_fixed_counts(psba_handle h, int *n_fixed_cams, int *n_fixed_pts);

/* ---- covariance of the refined cameras and points (fixed-K dense route) ------------------------
 * Definition (the same text in psba_amd/csrc/kernels_cov.hip and DESIGN.md).  The covariance is taken at the current
 * parameters and uses the linearization of psba_linearize(h, 1, 1): whitened, loss-weighted and masked by
 * psba_set_fixed, i.e. exactly what the normal equations see.  N = J^T J on the free blocks.  For mu >= 0 and
 * scale > 0,
 *   C = scale (N + mu I)^-1 on the free entries, zero on rows and columns of fixed blocks
 * (not the inverse of the placeholder).  Through the Schur complement:
 *   cameras   C_aa = scale S(mu)^-1; rows and columns of fixed cameras are removed and returned as zeros
 *   point i   C_bb,i = scale V*_i^-1 + sum_{j,k in cams(i)} Y_ij^T C_jk Y_ik,  Y_ij = W_ij V*_i^-1,  V*_i = V_i + mu I
 *             (ordered pairs of the point's free cameras, j == k included); a fixed point gives zeros, a point whose
 *             cameras are all fixed gives scale V*_i^-1; with every camera fixed no S is assembled and C_aa = 0
 * The cross blocks C_ab are not returned.  mu = 0 is the true covariance and needs the gauge fixed (two fixed cameras;
 * DESIGN 7c shows S is positive definite then); mu > 0 gives a regularised inverse, which is NOT a covariance.
 * scale is the variance factor (1: unit-weight residuals; the reduced chi-square psba_residual / (2 n2Dprojs - free
 * parameters) is the usual a-posteriori choice).
 * psba_covariance_compute: with reassemble != 0 it linearizes at the current parameters with coefficients (1, 1)
 * unless that linearization is current, runs psba_schur_assemble(mu) and psba_schur_reduce, copies S out of the reduce
 * buffer into a workspace of its own and inverts the copy there (a blocked Cholesky of its own on 16 x 16 MFMA tiles;
 * the Cholesky chain of psba_schur_solve and its factor are not touched).  The handle is left exactly as after
 * psba_schur_reduce: psba_get_reduce_buffer then returns the S that was inverted.  reassemble = 0 inverts what the
 * reduce buffer holds (psba_schur_assemble or psba_set_reduce_buffer before it, as for psba_cholmod_lambda: the hook
 * the tests use to invert a chosen matrix); only the camera part exists afterwards and psba_get_point_covariance
 * returns PSBA_E_STATE.  Returns PSBA_OK, PSBA_NOT_SPD or PSBA_SINGULAR_V (bit-or; the outputs are invalid then) and
 * synchronises.  PSBA_E_INVALID for mu < 0, scale <= 0 or non-finite values; PSBA_E_STATE, with a text that names the
 * reason, before an upload, while a try is in flight, on 11- or 16-parameter camera blocks, under PSBA_SOLVER_PCG and
 * under a rank layout or communicator; a refused call changes nothing.
 * The getters return PSBA_E_STATE until a compute has returned PSBA_OK and again after anything that moves the
 * parameters or the model (psba_accept, psba_set_params, psba_reset_params, psba_set_distortion,
 * psba_set_obs_covariance, psba_set_robust_loss, psba_set_fixed, psba_upload_problem), PSBA_E_INVALID for a camera
 * index out of range.  Workspaces (two n32 x n32 squares, 18 doubles per observation, 9 per point) are allocated on
 * first use and released by the next upload and by psba_destroy.  No floating-point atomics: two computes on the
 * same state return bit-identical arrays; C_aa and every point block are bit-symmetric.  PARITY UNPINNED: the
 * reference's SPDinv inverse is an intermediate of its solve and is never returned -- checked against an
 * extended-precision inverse of the device's own S, per-entry long-double sums of the point formula and the dense
 * inverse of a numpy twin's reduced normal matrix. */
int psba_covariance_compute(psba_handle h, double mu, double scale, int reassemble);
/* pairs[2 n_pairs] = (j, k) in any order, out[36 n_pairs] row-major = C_jk; pairs NULL: n_pairs must be nCams, the
 * diagonal blocks */
int psba_get_camera_covariance(psba_handle h, int n_pairs, const int *pairs, double *out);
int psba_get_covariance_matrix(psba_handle h, double *Caa /* (6 nCams)^2 row-major, symmetric */);
int psba_get_point_covariance(psba_handle h, double *out /* n3Dpts*9, full symmetric 3x3 */);
/* measurement: HIP-event milliseconds of the last psba_covariance_compute that returned PSBA_OK -- factor (with the
 * compaction), inverse (with the mirror), points.  Linearization and assembly are timed by psba_profile_get. */
int psba_covariance_times(psba_handle h, double ms3[3]);

/* ---- covariance of the refined cameras and points with free intrinsics (PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD;
 * DESIGN 7l) -- verbs of their own: psba_covariance_compute keeps refusing both models and its getters return 6 x 6
 * blocks ------------------------------------------------------------------------------------------------------------
 * Definition (the same text in psba_amd/csrc/kernels_cov.hip and DESIGN.md).  The covariance is taken at the
 * current parameters, on the linearization of psba_linearize(h, 1, 1).  That linearization is exactly what the route's
 * normal equations see: the intrinsics mask, the groups, held poses and points, the priors' information in U and V,
 * blocks weighted by omega / sigma.  Let N be that system and D the diagonal of psba_set_damping (I for the identity
 * rule).  For mu >= 0 and scale > 0 the covariance is built in three steps.
 *   reduced camera part   X = S(mu)^-1 on the live coordinates of the folded S.  A live coordinate is not masked, is
 *                         not a held pose coordinate, is not folded away by the groups, and is not padding
 *   returned camera part  C_aa = scale E X E^T, where E copies a representative's shared intrinsic to the members of
 *                         its group: rows and columns of masked and held coordinates are exactly 0 (not the inverse
 *                         of the placeholder); a folded-away coordinate's row and column are bit-identical to its
 *                         representative's, because shared intrinsics are perfectly correlated; C_aa is bit-symmetric
 *   point i               C_bb,i = scale V*_i^-1 + sum_{j,k in cams(i)} Y_ij^T C_jk Y_ik, with the expanded C_aa,
 *                         V*_i = V_i + mu D_i and Y_ij the block that k_free_Y stored for this mu.  A held point gives
 *                         zeros; a point without observations, and one whose blocks Y are all zero, scale V*^-1
 * mu = 0 is the covariance and needs a gauge: held poses or priors.  mu > 0 is a regularised inverse and NOT a
 * covariance.  The cross blocks C_ab are not returned.  PARITY UNPINNED, as for psba_covariance_compute.
 * psba_free_covariance_compute follows the rules of psba_covariance_compute.  With reassemble != 0 it linearizes with
 * (1, 1) unless that linearization is current, then runs psba_schur_assemble(mu) and psba_schur_reduce; the handle is
 * left as after those calls (a psba_schur_solve may follow; psba_get_reduce_buffer returns the S that was inverted),
 * and a psba_levmar after a compute takes the path it would have taken without it.  reassemble = 0 inverts what the
 * reduce buffer holds; only the camera part is valid afterwards.  The inverse is that of psba_covariance_compute (its
 * blocked Cholesky and inverse on 16 x 16 MFMA tiles, on a private copy of S) between a compaction to the live
 * coordinates and an expansion over the groups.  Returns PSBA_OK, PSBA_NOT_SPD or PSBA_SINGULAR_V (bit-or; the
 * outputs are invalid then) and synchronises.  PSBA_E_STATE before an upload, while a try is in flight and on
 * six-parameter blocks (the text names psba_covariance_compute); PSBA_E_INVALID for a mu that is not finite and >= 0
 * and for a scale that is not finite and > 0; a refused call changes nothing.
 * The getters return PSBA_E_STATE until a compute has returned PSBA_OK and again after anything that moves the
 * parameters or the model: every setter of the route, psba_set_params, psba_reset_params, psba_accept,
 * psba_upload_problem.  psba_get_free_point_covariance and psba_get_free_sigmas also return PSBA_E_STATE after a
 * compute with reassemble = 0.  No floating-point atomics: two computes on the same state return bit-identical
 * arrays. */
int psba_free_covariance_compute(psba_handle h, double mu, double scale, int reassemble);
/* pairs[2 n_pairs] = (j, k) in any order, out[cnp^2 n_pairs] row-major = C_jk (cnp = psba_camera_block); pairs NULL:
 * n_pairs must be nCams, the diagonal blocks */
int psba_get_free_camera_covariance(psba_handle h, int n_pairs, const int *pairs, double *out);
int psba_get_free_covariance_matrix(psba_handle h, double *Caa /* (cnp nCams)^2 row-major, symmetric */);
int psba_get_free_point_covariance(psba_handle h, double *out /* n3Dpts*9, full symmetric 3x3 */);
/* sigma[nT] = [cnp per camera ; 3 per point]: the square roots of the diagonals of C_aa and of the C_bb,i (one small
 * kernel); a coordinate with variance 0 (masked, held) gives 0 */
int psba_get_free_sigmas(psba_handle h, double *sigma);
/* test hook in the style of psba_get_free_obs_blocks: V [n3Dpts][9] = V_i as the linearization stored it (undamped,
 * full symmetric; the priors' information included, a held point's placeholder) and Y [n2Dprojs][cnp][3] = the blocks
 * k_free_Y stored at the last psba_schur_assemble.  Either pointer may be null.  Needs an assembled try
 * (psba_schur_assemble, or psba_free_covariance_compute with reassemble != 0, and no psba_schur_solve since):
 * PSBA_E_STATE otherwise and for six-parameter blocks. */
int psba_get_free_point_blocks(psba_handle h, double *V, double *Y);
/* measurement: HIP-event milliseconds of the last psba_free_covariance_compute that returned PSBA_OK -- factor (with
 * the compaction), inverse (with the expansion), points */
int psba_free_covariance_times(psba_handle h, double ms3[3]);
/* which S-assembly route the uploaded problem takes: 0 = LDS-resident partitions of the block
 * triangle with the static schedule (fewer than 2048 cameras, up to 8 GB of partial-sum slabs on
 * this rank), 1 = the owner route for larger problems (one thread per block segment,
 * products sorted by camera pair, sums in registers; PSBA_SCHUR_OWNER=1 forces it), 2 = global
 * fp64 atomics straight into S (the
 * first-generation kernel, kept for cross-checks: PSBA_SCHUR_ATOMIC=1), 3 = the ring route (opt-in
 * experiment, PSBA_SCHUR_RING=1), 4 = block-sparse S (PSBA_SOLVER_PCG), 5 = the free-intrinsics route (blocks of 11
 * and 16: products sorted by block, one MFMA per product), 6 = the same assembly into a block-sparse S of those
 * blocks (PSBA_SOLVER_SPARSE).  The reference has one
 * route for every size (CL_files/compute_S.cl:6-78). */
int psba_schur_path(psba_handle h, int *path);

/* ---- fused verbs (what the optimiser loops call) --------------------------------------
 * One damping try = psba_schur_assemble -> psba_schur_reduce -> psba_schur_solve ->
 * psba_backsub; nothing is copied to the host in between. */

/* ||e||^2 at a parameter set (the robust cost sum rho(s_a) under a loss): compute_exQT + compute_L2_sq
 * (PSBA/sba_func.h:10-19, PSBA/levmar.cpp:93-94,188-193, PSBA/misc.cpp:151-157).
 * With a communicator attached the value is summed over all ranks. */
int psba_residual(psba_handle h, int which, double *cost);
/* compute_jacobiQT + compute_U + compute_V + compute_Wblks + compute_g in one kernel
 * (PSBA/sba_func.h:26-56,74-81,103-109; PSBA/levmar.cpp:103-108).  coeff scales U,V,W
 * (1 in LM, 2 in TR), coeff_g scales g (1 in LM, -2 in TR; PSBA/trust_region.cpp:122,133-137).
 * A/B/e are never written to memory. */
int psba_linearize(psba_handle h, double coeff, double coeff_g);
/* maxElmOfUV (PSBA/sba_func.h:58): max over diag(U), diag(V); global over ranks */
int psba_max_diag(psba_handle h, double *out);
/* The loop's prologue in one call and one synchronisation (PSBA/levmar.cpp:93-120): the cost at
 * the current parameters, their linearization (as psba_linearize) and its largest diagonal
 * entry.  The psba_linearize that follows with the same coefficients has nothing left to do. */
int psba_begin(psba_handle h, double coeff, double coeff_g, double *cost, double *max_diag);
/* update_UV + compute_Vinv + compute_Yblks + compute_S + compute_ea
 * (PSBA/sba_func.h:60-68,84-98,114-119; PSBA/levmar.cpp:126-131).  mu is applied on the
 * fly, U/V are not modified, so there is no restore_UVdiag.  Leaves this rank's
 * contribution to [S | ea] in the reduce buffer. */
int psba_schur_assemble(psba_handle h, double mu);
/* sum [S | ea] over ranks with one RCCL all-reduce on the handle's stream; no-op without a
 * communicator.  (No counterpart in the reference: it is single-device.) */
int psba_schur_reduce(psba_handle h);
/* SPDinv + matVec_mul as one Cholesky factorisation and two triangular solves
 * (PSBA/cl_spdinv.h:7-8, PSBA/cl_linearalg.h:8-9, PSBA/levmar.cpp:134-140).  The status
 * (PSBA_OK / PSBA_NOT_SPD) stays on the device until psba_backsub returns it. */
int psba_schur_solve(psba_handle h);

typedef struct {
  int status;       /* PSBA_OK, PSBA_NOT_SPD, PSBA_SINGULAR_V (bit-or) */
  double dp_l2;     /* ||dp||^2                         PSBA/levmar.cpp:157 */
  double gain_den;  /* sum dp*(mu*dp+g)                 PSBA/levmar.cpp:271-280 */
  double new_cost;  /* ||e(p+dp)||^2                    PSBA/levmar.cpp:188-193 */
  double newp_l2;   /* ||p+dp||^2                       PSBA/levmar.cpp:212 */
} psba_try_scalars;

/* compute_eb + compute_dpb + compute_newp + compute_exQT(new) + the host reductions the
 * loop needs, in one kernel (PSBA/sba_func.h:124-137, PSBA/levmar.cpp:151-195).
 * Synchronises and fills *out (all-reduced over ranks). */
int psba_backsub(psba_handle h, double mu, psba_try_scalars *out);
/* The same in two halves, so that the host's decision (PSBA/levmar.cpp:169-223) no longer idles
 * the GPU: psba_backsub_async queues the kernel and the copy of its scalars and returns;
 * psba_linearize_ahead then queues psba_linearize's work for the PROPOSED parameters into a
 * second set of linearization buffers (the current linearization stays valid); psba_backsub_wait
 * waits for the scalars only.  If the step is accepted, psba_accept makes the proposed
 * parameters AND the linearization computed ahead current, and the next psba_linearize (same
 * coefficients) has nothing left to do; if it is rejected the work done ahead is dropped. */
int psba_backsub_async(psba_handle h, double mu);
int psba_linearize_ahead(psba_handle h);
int psba_backsub_wait(psba_handle h, psba_try_scalars *out);
/* update_p (PSBA/sba_func.h:138): the proposed parameters become current (pointer swap) */
int psba_accept(psba_handle h);

/* ---- how a try's scalars reach the host, and hooks to test it (psba_amd/csrc/scal_publish.h states the format) ----
 * The device publishes a block of 104 words (doubles), a stamp and a check word over both into pinned memory;
 * psba_backsub_wait copies the 106 words and accepts the copy iff it carries the wanted stamp and its own check.
 * Everything is decided on bit patterns: NaN payloads and the sign of a zero count.
 * psba_scal_block_check: *check = the check word (its bits, in a double) of block[104] under the stamp.
 * psba_scal_block_take: the host's take applied to caller memory, words[106] = block, stamp, check; out[104] receives
 * the private copy of the block; returns 1 accepted, 0 refused.  Neither needs a handle or a GPU. */
int psba_scal_block_check(const double *block, double stamp, double *check);
int psba_scal_block_take(const double *words, double want_stamp, double *out);
/* Since psba_create: *takes = blocks psba_backsub_wait accepted from a linearization queued ahead (one rank, the
 * default route; a try whose scalars travel behind an event is not counted), *torn = tries among them in which a
 * reading carried the wanted stamp over a block that failed its check, and was read again. */
int psba_publish_stats(psba_handle h, long long *takes, long long *torn);
/* Test hook: one workgroup of threads = 64, 128 or 256 runs nothing but the publishing prologue of the linearization
 * kernels with the next stamp, the stream is waited for and raw[106] receives the pinned words: block, stamp, check.
 * block[104] stands in the device scalar block for that launch (the device's own block is put back behind it); NULL
 * publishes the device's block as it is, which is how a test reads it.  PSBA_E_STATE while a try is in flight; the
 * try's result is dropped (psba_accept needs a new try). */
int psba_test_publish(psba_handle h, const double *block, int threads, double *raw);

/* ---- 1:1 mirror of sba_func.h for per-kernel parity tests -----------------------------
 * Same names and argument meaning as the reference; the dimension arguments and
 * PSBA_structPtr collapse into the handle.  A NULL host pointer means "stay on device"
 * exactly as in the reference.  Each verb leaves the device state as the reference's
 * wrapper of the same name does. */
/* ex: the residual the normal equations see (w L e under a robust loss and covariances) */
int psba_compute_exQT(psba_handle h, int which, double *ex);             /* sba_func.h:10-19 */
int psba_compute_jacobiQT(psba_handle h, double *jac_A, double *jac_B);  /* sba_func.h:26-32 */
int psba_compute_U(psba_handle h, double coeff, double *out);            /* sba_func.h:38-44 */
int psba_compute_V(psba_handle h, double coeff, double *out);            /* sba_func.h:50-56 */
int psba_maxElmOfUV(psba_handle h, double *out);                         /* sba_func.h:58 */
int psba_update_UV(psba_handle h, double mu, double *U, double *V);      /* sba_func.h:60-61 */
int psba_restore_UVdiag(psba_handle h);                                  /* sba_func.cpp:694 */
int psba_compute_Vinv(psba_handle h, double *Vinv /* n3Dpts*9, full symmetric */); /* :63-68 */
int psba_compute_Wblks(psba_handle h, double coeff, double *Wblks);      /* sba_func.h:74-81 */
int psba_compute_Yblks(psba_handle h, double *Yblks);                    /* sba_func.h:84-90 */
int psba_compute_S(psba_handle h, double *S /* (6 nCams)^2 row-major */); /* sba_func.h:93-98 */
int psba_compute_g(psba_handle h, double coeff, double *g);              /* sba_func.h:103-109 */
int psba_compute_ea(psba_handle h, double *ea);                          /* sba_func.h:114-119 */
/* SPDinv + matVec_mul: returns PSBA_OK / PSBA_NOT_SPD like SPDinv's 0.0 / 1.0; dpa[6 nCams] */
int psba_SPDinv_matVec(psba_handle h, double *dpa);          /* cl_spdinv.h:7, cl_linearalg.h:8 */
int psba_compute_eb(psba_handle h, double *eb /* 3 n3Dpts */);           /* sba_func.h:124-129 */
int psba_compute_dpb(psba_handle h, double *dp /* whole dp, nT */);      /* sba_func.h:131-135 */
int psba_compute_newp(psba_handle h, double *new_p /* nT */);            /* sba_func.h:137 */
int psba_update_p(psba_handle h, double *p /* nT */);                    /* sba_func.h:138 */

/* ---- the Levenberg-Marquardt caller, PSBA/levmar.cpp:45-256 --------------------------- */
typedef struct {
  int max_iter;     /* literal 50 in the reference (levmar.cpp:100) */
  int tr_handoff;   /* 1: return PSBA_ITER_TURN_TO_TR after 5 consecutive |rho-1|<0.2
                       (levmar.cpp:215-219); 0: stay in LM */
  int verbose;      /* print the reference's per-try line (levmar.cpp:197) */
  int log_cap;      /* rows available in log (5 doubles each), 0 = none */
  int start_itno;   /* the reference shares itno between LM and TR (main.cpp:193-208) */
  double init_mu;   /* mu_0 = init_mu * max diag(U, V); 0 = the reference's PSBA_INIT_MU 1e-3 (psba.h:6,
                       levmar.cpp:114-116), a compile-time constant there.  Under PSBA_DAMPING_MARQUARDT
                       (psba_set_damping) mu_0 = init_mu itself, 0 = 1e-3: D carries the scale, the largest diagonal
                       entry does not enter; psba_lm_result.mu0 reports it */
  double stop_cost; /* the loop ends with PSBA_ITER_ERR_SMALL_ENOUGH once ||e||^2 <= stop_cost; 0 = the reference's
                       PSBA_STOP_THRESH 1e-12 (psba.h:7, levmar.cpp:247-248), an absolute figure in squared image
                       units that ends a noise-free problem before fp64 is used up; negative = no such test (the
                       relative tests on dp still end the loop) */
} psba_lm_options;

typedef struct {
  int flag;         /* PSBA_ITER_* */
  int iters;        /* value of itno at exit */
  int tries;        /* damping tries executed */
  double init_err, final_err, mu0, mu_final;
  int n_log;
  double seconds;   /* wall time inside the loop */
  int pcg_unconverged; /* PSBA_SOLVER_PCG: solves of this call that returned PSBA_PCG_MAXIT */
} psba_lm_result;

void psba_lm_default_options(psba_lm_options *o);
/* log rows: (itno, new ||e||^2, rho, mu, accepted{1,0,-1=solve failed}) per damping try */
int psba_levmar(psba_handle h, const psba_lm_options *opts, psba_lm_result *res, double *log);
/* The linearizations psba_levmar queues ahead take a lean form on an eligible handle: K1 stores the Jacobian factors
 * (A | B | e, 160 bytes per observation) and neither W nor the per-camera sums, and the Schur assembly forms S, e_a
 * and g_a from them.  Eligible: six-parameter camera blocks, one rank without a communicator, the LDS-partition
 * Schur route in its rows layout (psba_schur_path 0), the dense solver, K3 in its recompute form, no lens model,
 * covariance weights, robust loss, fixed blocks or priors, no point seen by more than 256 cameras; PSBA_LEAN_LIN=0
 * (read at upload) forces the standard form.  Every other handle takes the standard form.  When psba_levmar returns,
 * every linearization a later verb can reach is a standard one.  *lean = 1: the last psba_levmar of this handle
 * queued lean linearizations, 0: standard ones (or none yet). */
int psba_lm_ran_lean(psba_handle h, int *lean);
/* For tests of the lean assembly at a chosen mu and chosen coefficients: linearizes the CURRENT parameters once more,
 * in the lean form, behind a psba_linearize with the handle's coefficients.  W, U and g_a of that psba_linearize stay
 * valid; psba_schur_assemble then takes the lean route (and its reduce rewrites g_a from the lean sums) until the
 * next linearization.  The sba_func.h mirror verbs that assemble S (they dump Y and V^-1, which the lean route does
 * not form) return PSBA_E_STATE until then.  PSBA_E_STATE on a handle that is not eligible, or that could not
 * allocate the records. */
int psba_linearize_lean(psba_handle h);

/* ---- the trust-region caller, PSBA/trust_region.cpp:49-595, and its extra operators -------
 * (B = 2 J^T J, g = -2 J^T e through psba_linearize(h, 2, -2); with a communicator the points may be
 * sharded: psba_jmul_dots sums its dot products over the ranks, psba_get_gradient returns the
 * complete g_a, the modified Cholesky runs replicated on the all-reduced S). */
/* compute_Jmultiply (PSBA/sba_func.cpp:19-75, CL_files/compute_Jmultiply.cl:6-52): J x for a host
 * vector x[nT].  Jmul has 2 values per OBSERVATION (2 * n2Dprojs, observation order) -- the
 * non-zeros, in the same order, of the reference's dense nP x nC x 2 grid. */
int psba_compute_Jmultiply(psba_handle h, const double *x, double *Jmul);
/* what the loop needs of it: dots = (Jx1.Jx1, Jx1.Jx2, Jx2.Jx2); x2 NULL = x1
 * (trust_region.cpp:125-126,166-176,209-211 take these dot products on the host) */
int psba_jmul_dots(psba_handle h, const double *x1, const double *x2, double dots[3]);
/* v[0..n) (n <= 8) summed over the ranks of the communicator, in place; no communicator: untouched.
 * What a host loop over sharded points needs for its inner products: the point parts of two
 * vectors are rank-local, so a dot product is (camera part) + sum over ranks of (point part). */
int psba_allreduce_scalars(psba_handle h, double *v, int n);
/* g = [g_a ; g_b] of the last linearization (the host output of compute_g, sba_func.h:103-109) */
int psba_get_gradient(psba_handle h, double *g);
/* dp = [dpa ; dpb] of the last solve + back-substitution (host output of compute_dpb) */
int psba_get_dp(psba_handle h, double *dp);
/* dp_buffer <- dp, then compute_newp: proposed parameters = current + dp
 * (trust_region.cpp:183-187); psba_residual(PSBA_PARAMS_NEW) evaluates them, psba_accept takes them */
int psba_set_step(psba_handle h, const double *dp);
/* the lambda estimate taken when S is not positive definite at lambda = 0
 * (trust_region.cpp:341-363): S is assembled again without damping, factored by the modified
 * Cholesky of PSBA/cl_cholmod.cpp:25-201 / CL_files/cholmod_blk.cl:87-846, and
 * lambda = |sum_i E_i| / (6 nCams) with E = diag(L L^T) - diag(S).  info3 (may be NULL) =
 * (delta, beta, number of block columns that took the one-column route).  reassemble = 0 skips
 * the assembly and factors what the reduce buffer holds (psba_schur_assemble or
 * psba_set_reduce_buffer before it): the hook the tests use to factor a chosen matrix.
 * PSBA_SOLVER_PCG (no dense S, and the reference has no sparse mode): lambda is the Gershgorin shift of the
 * stored blocks instead, max(0, -min_i (S_ii - sum_{c != i} |S_ic|)) -- the smallest shift that makes S + lambda I
 * diagonally dominant -- or 1e-6 max_i of those margins when S is diagonally dominant already;
 * info3 = (min margin, max margin, 0). */
int psba_cholmod_lambda(psba_handle h, int reassemble, double *lambda, double *info3);
/* ---- test hook: the factor L of that modified Cholesky, L[6 nCams][6 nCams] row-major (the strict upper triangle
 * holds the zeros the kernel wrote).  Valid only directly after a dense-mode psba_cholmod_lambda: the factor lives in
 * the buffer of the Cholesky chain, so psba_schur_assemble, psba_schur_solve, psba_chol_dist_*, the sba_func.h mirror's
 * assembly and solve and psba_upload_problem invalidate it -- PSBA_E_STATE then, as before any psba_cholmod_lambda and
 * under PSBA_SOLVER_PCG (no factor exists: the estimate is a Gershgorin shift). */
int psba_get_cholmod_factor(psba_handle h, double *L);
/* ---- test hook: the per-observation blocks of the free-intrinsics linearization (PSBA_CAMERA_FREE_K /
 * PSBA_CAMERA_FREE_KD), as the fused kernel itself stored them: W [n2Dprojs][cnp][3] row-major = coeff A^T B of
 * observation a (cnp = psba_camera_block: 11 or 16; a masked intrinsic's row is zero), Be [n2Dprojs][8] = B (2 x 3
 * row-major) | e (2).  Either pointer may be null.  A device-to-host copy, no kernel.  Valid after a psba_linearize
 * (or psba_begin) at the current parameters until something overwrites the buffers or moves the parameters:
 * psba_linearize_ahead (it reuses the B | e buffer), psba_accept of a proposal that was not linearized ahead,
 * psba_set_params, psba_reset_params, psba_set_distortion, psba_set_intrinsics_mask, psba_set_camera_masks,
 * psba_set_intrinsics_groups, psba_upload_problem -- PSBA_E_STATE then, as before any linearization and for six-parameter camera blocks (whose
 * blocks the sba_func.h mirror reads: psba_compute_jacobiQT, psba_compute_Wblks). */
int psba_get_free_obs_blocks(psba_handle h, double *W, double *Be);
/* ---- test hook: D[nT] = [cnp per camera ; 3 per point] of the current linearization under PSBA_DAMPING_MARQUARDT
 * (psba_set_damping), as the kernel behind the linearization stored it.  A device-to-host copy, no kernel.  Valid
 * after a psba_linearize or psba_begin under Marquardt -- and after the psba_accept of a proposal that was linearized
 * ahead, whose D comes with it -- until the parameters or the model change: psba_accept of a proposal that was not
 * linearized ahead, psba_set_params, psba_reset_params, psba_set_distortion, psba_set_intrinsics_mask,
 * psba_set_camera_masks, psba_set_intrinsics_groups, psba_set_damping, psba_upload_problem -- PSBA_E_STATE then, as under
 * PSBA_DAMPING_IDENTITY and for six-parameter camera blocks.  (psba_linearize_ahead writes the second set: the
 * diagonal of a rejected step's current parameters stays readable.) */
int psba_get_damping_diag(psba_handle h, double *D);

typedef struct {
  int max_iter;     /* literal 50, shared with levmar() through itno (trust_region.cpp:112) */
  int start_itno;
  int verbose;      /* print the reference's per-step line (trust_region.cpp:250) */
  int log_cap;      /* rows available in log (6 doubles each), 0 = none */
  double init_lambda; /* damping the loop starts with; 0 = the reference's (trust_region.cpp:95-96), where the
                         first factorization of the gauge-free S fails and the modified Cholesky picks lambda */
} psba_tr_options;

typedef struct {
  int flag;         /* PSBA_ITER_* */
  int iters;        /* value of itno at exit */
  int tries;        /* steps evaluated */
  int chol_fail;    /* factorizations of S that failed (each followed by a larger lambda) */
  double init_err, final_err, lambda, delta;
  int n_log;
  double seconds;
} psba_tr_result;

void psba_tr_default_options(psba_tr_options *o);
/* log rows: (itno, ||e(p + step)||^2, rho, delta after the update, lambda, accepted{1,0}) per step */
int psba_trust_region(psba_handle h, const psba_tr_options *opts, psba_tr_result *res, double *log);

/* the driver's alternation, PSBA/main.cpp:193-208: levmar() until ITER_TURN_TO_TR, trust_region()
 * until ITER_TURN_TO_LM, max_iter iterations in total */
typedef struct {
  int flag, iters, lm_calls, tr_calls;
  double init_err, final_err, seconds;
} psba_solve_result;
int psba_solve(psba_handle h, int max_iter, int verbose, psba_solve_result *res);

/* ---- multi-GPU: 3-D points sharded over ranks, one process per GPU -------------------- */
/* contiguous point ranges balanced on observation count; pt_begin[nranks+1] */
int psba_partition_points(int n3Dpts, const int *iidx, int n2Dprojs, int nranks, int *pt_begin);
/* 128-byte RCCL unique id, created on rank 0 and handed to every rank by the launcher */
int psba_comm_unique_id(void *id128);
int psba_comm_init(psba_handle h, int nranks, int rank, const void *id128);
int psba_comm_rank(psba_handle h, int *nranks, int *rank);
/* Bring-your-own reduction (MPI, host staging, tests): declare the rank layout without an RCCL
 * communicator, then sum the reduce buffer yourself between psba_schur_assemble and
 * psba_schur_solve.  The buffer is the padded [S | ea] block: psba_reduce_buffer_size doubles.
 * With a layout but no communicator psba_backsub / psba_residual / psba_max_diag return this
 * rank's partial sums (camera terms counted on rank 0 only), to be summed by the caller. */
int psba_set_rank_layout(psba_handle h, int nranks, int rank);
int psba_reduce_buffer_size(psba_handle h, long long *n_doubles);
int psba_get_reduce_buffer(psba_handle h, double *out);
int psba_set_reduce_buffer(psba_handle h, const double *in);

/* ---- on-disk format: readInitialSBAEstimate (PSBA/readparams.cpp:444-519) -------------
 * Reads an sba-format cams file (7 columns q,t with fixedK[5] replicated, or 12 columns
 * K5,q,t) and pts file; applies quat2vec (PSBA/misc.cpp:21-49), zeroes the local rotation
 * and splits K from the extrinsics (PSBA/main.cpp:131-149).  Arrays are malloc'ed by the
 * library and released with psba_free_problem. */
typedef struct {
  int nCams, n3Dpts, n2Dprojs;
  double *Kparas, *impts, *initrot, *camsEx, *pts3D;
  int *iidx, *jidx;
} psba_problem;
int psba_read_problem(const char *cams_file, const char *pts_file, const double *fixedK,
                      psba_problem *out);
void psba_free_problem(psba_problem *p);
/* The same reader, plus what psba_read_problem skips (see psba_set_distortion for the model): kc[nCams * 5] when the
 * cams file has 17 columns (K5, kc(1:5), q, t), else NULL; cov[n2Dprojs * 4] (row-major 2x2 per observation, in
 * the returned observation order; the 3-value form xx xy yy expanded) when the pts file carries covariances, else
 * NULL.  base is exactly what psba_read_problem returns.  Released with psba_free_problem_ex. */
typedef struct {
  psba_problem base;
  double *kc, *cov;
} psba_problem_ex;
int psba_read_problem_ex(const char *cams_file, const char *pts_file, const double *fixedK, psba_problem_ex *out);
void psba_free_problem_ex(psba_problem_ex *p);
/* The writer the reference declares and keeps commented out (printSBAMotionData /
 * printSBAStructureData / printSBAData, PSBA/readparams.h:13-25; output filter vec2quat,
 * PSBA/misc.cpp:60-85): cams file with one line per camera -- K5 when with_K != 0, then the full
 * quaternion q_l(v) (x) initrot and t -- and pts file "X Y Z nframes {frame x y}...".  The files
 * are valid input of psba_read_problem (which then returns initrot = that quaternion, v = 0). */
int psba_write_problem(const char *cams_file, const char *pts_file, int nCams, int n3Dpts, int n2Dprojs,
                       const double *Kparas, const double *initrot, const double *camsEx, const double *pts3D,
                       const double *impts, const int *iidx, const int *jidx, int with_K);
/* Bundle-Adjustment-in-the-Large text file -> sba cams / pts files in the reference's camera
 * model (how its data/Trafalgar-* files relate to the public BAL sets): camera turned to look
 * down +z, image y negated, K = (f,0,0,1,0); the radial terms k1, k2 are dropped (the reference
 * has no distortion) and their largest magnitude is returned in *max_abs_k (may be NULL). */
int psba_convert_bal(const char *bal_file, const char *cams_out, const char *pts_out, double *max_abs_k);
/* The same conversion with the radial terms kept: 17-column cams "f 0 0 1 0 k1 k2 0 0 0 q t".  BAL's normalised
 * point p = -P / P.z becomes (x', y') = (p.x, -p.y) here, with the same |p|^2, so BAL's f (1 + k1 |p|^2 + k2 |p|^4) p
 * is exactly the distortion model of psba_set_distortion with kc = (k1, k2, 0, 0, 0). */
int psba_convert_bal_kd(const char *bal_file, const char *cams_out, const char *pts_out);

/* ---- measurement ----------------------------------------------------------------------
 * HIP-event timing of the kernels launched by the fused verbs, on the handle's stream. */
#define PSBA_K_LINEARIZE 0
#define PSBA_K_SCHUR 1
#define PSBA_K_CHOLESKY 2
#define PSBA_K_BACKSUB 3
#define PSBA_K_RESIDUAL 4
#define PSBA_K_ALLREDUCE 5
#define PSBA_K_SCHUR_REDUCE 6 /* slab sum + U + mu I + mirror that finishes S after PSBA_K_SCHUR */
#define PSBA_K_COUNT 7
/* on < 0: time every kernel class; on > 0: bit mask (1 << PSBA_K_*) of the classes to time;
 * 0: off.  Every timed launch costs two event records on the stream (~3 us). */
int psba_profile_enable(psba_handle h, int on);
int psba_profile_reset(psba_handle h);
/* total_ms and launch count per kernel class since the last reset (synchronises) */
int psba_profile_get(psba_handle h, int kernel, double *total_ms, int *launches);
/* algorithmic bytes of one launch of a kernel class for the uploaded problem
 * (SURVEY.md section 8(d) formulas; stated in DESIGN.md) */
int psba_algorithmic_bytes(psba_handle h, int kernel, double *bytes);

/* ---- block-sparse S and an iterative solve -----------------------------------------
 * The reference forms the dense nA x nA S for every problem (CL_files/compute_S.cl:6-78) and inverts it
 * (PSBA/cl_spdinv.cpp:18-40).  With PSBA_SOLVER_PCG only the 6x6 blocks of camera pairs that see a
 * common point exist (the lower block triangle as a list; no dense buffer is allocated), and
 * psba_schur_solve runs conjugate gradients with a block-Jacobi preconditioner until
 * ||S x - e_a|| <= tol ||e_a|| or max_iter iterations; a diagonal block that is not positive definite or
 * a direction of non-positive curvature (or a residual that is not finite: NaN / Inf in S or e_a) reports
 * PSBA_NOT_SPD, so psba_levmar works unchanged; a solve
 * that uses up max_iter returns PSBA_PCG_MAXIT (> 0: the step is usable, the LM gain ratio judges it, and
 * psba_levmar counts such solves in psba_lm_result.pcg_unconverged); e_a == 0 or an exactly solved system
 * is a converged solve with x as it stands, not a break-down.  The
 * sba_func.h mirror verbs and the trust-region operators need the dense S and refuse this mode.
 * Sharded points: every rank must hold the same block list, the union of the blocks its ranks' points
 * produce.  With a communicator psba_upload_problem forms it by itself (one max all-reduce of a byte per
 * block); a host with its own transport computes psba_sparse_pattern on every rank (host only, no
 * handle), ORs the flags, and hands them to psba_set_sparse_pattern before psba_upload_problem; between
 * psba_schur_assemble and psba_schur_solve it then sums psba_get_sparse_S over the ranks and returns the
 * sums with psba_set_sparse_S (the conjugate gradients themselves run replicated on every rank).
 * psba_set_solver: before psba_upload_problem; tol <= 0 / max_iter <= 0 keep 1e-10 / 500.
 * PSBA_SOLVER_SPARSE is the block-sparse mode for whatever camera block the handle has.  With six-parameter blocks
 * it is PSBA_SOLVER_PCG itself (same code path, same bits).  Under PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD, where
 * PSBA_SOLVER_PCG stays refused at the upload, it selects the route of kernels_free_pcg.hip (psba_schur_path = 6):
 * the blocks are cnp x cnp (val[cnp cnp blocks] row-major, k <= j, every diagonal block present, also that of a
 * camera without observations), the assembly writes them with the fixed-order MFMA kernels, and the conjugate
 * gradients sum every inner product from per-workgroup partial sums in a fixed order -- no floating-point atomics, so
 * two solves of the same blocks give the same bits.  Nothing of size nA^2 is allocated.  psba_pcg_info,
 * psba_get_sparse_S, psba_set_sparse_S, psba_sparse_S_times, psba_schur_solve and psba_levmar work as under
 * PSBA_SOLVER_PCG; the intrinsics mask, held poses and points, observation weighting, priors and Marquardt damping
 * compose with it.  psba_set_intrinsics_groups, psba_free_covariance_compute and its getters, psba_get / set_reduce_buffer,
 * psba_SPDinv_matVec, psba_chol_dist_* and psba_get_cholmod_factor return PSBA_E_STATE with a text that names
 * PSBA_SOLVER_SPARSE, before any copy or launch.  Intrinsics shared between cameras have a verb of their own on this
 * route, psba_set_sparse_intrinsics_groups (blocks of 16): the list stays unfolded and the solve folds. */
#define PSBA_SOLVER_DENSE 0
#define PSBA_SOLVER_PCG 1
#define PSBA_SOLVER_SPARSE 2   /* block-sparse S of cnp x cnp blocks + block-Jacobi PCG, whatever the camera block */
int psba_set_solver(psba_handle h, int solver, double tol, int max_iter);
/* iterations and ||r|| / ||e_a|| of the last solve; blocks stored / blocks of the dense lower triangle */
int psba_pcg_info(psba_handle h, int *iters, double *relres, long long *blocks, long long *dense_blocks);
/* the assembled blocks: jk[2 blocks] = (j, k), k <= j; val[cnp cnp blocks] row-major (36 doubles per block
 * with six-parameter blocks, 121 / 256 under PSBA_SOLVER_SPARSE on blocks of 11 / 16); ea[nA]; any pointer may be NULL */
int psba_get_sparse_S(psba_handle h, int *jk, double *val, double *ea);
int psba_set_sparse_S(psba_handle h, const double *val, const double *ea);
/* ---- mirror verb: y[nA] = S x[nA] on the stored blocks, formed by the kernel that forms the products of the solve
 * (a stored block serves its own block row as it stands and its column's block row transposed; a diagonal block is
 * read through its lower triangle only, its strict upper triangle is never touched).  The order of the sums of a row
 * is fixed, so the same blocks and x give the same bits.  Same state as psba_get_sparse_S (between
 * psba_schur_assemble and psba_schur_solve, PSBA_SOLVER_PCG, no structure-only try; PSBA_E_STATE otherwise);
 * changes neither the blocks nor e_a nor a later solve.  Synchronises. */
int psba_sparse_S_times(psba_handle h, const double *x, double *y);
/* test hook: M[cnp cnp nCams], the inverses of the diagonal blocks that the last psba_schur_solve preconditioned with
 * (PSBA_SOLVER_SPARSE on blocks of 11 / 16; with psba_set_sparse_intrinsics_groups the inverses of the folded blocks).
 * A device-to-host copy.  PSBA_E_STATE unless that solve still stands: a new assembly, psba_set_sparse_S, a covariance
 * verb of this route and every setter of the model end it. */
int psba_get_sparse_precond(psba_handle h, double *M);
/* ---- covariance of chosen cameras under PSBA_SOLVER_SPARSE on camera blocks of 11 / 16 -------------
 * psba_free_covariance_compute inverts an nA x nA square that this route never allocates, and keeps refusing a sparse
 * handle.  Here the object is the joint covariance of a chosen set of cameras: C = scale (S(mu)^-1)[sel, sel], from
 * solving S X = E_sel -- every chosen camera contributes cnp right-hand sides, one panel of 16 columns
 * (kernels_free_pcg_many.hip).
 *   * The linearization is psba_linearize(h, 1, 1) at the current parameters, as for psba_free_covariance_compute: the
 *     mask, the per-camera masks, held poses and points, priors, observation weighting and the damping rule are in S.
 *   * A coordinate is live if it is neither masked nor a held pose coordinate (groups cannot be set on this route).
 *   * For a live chosen coordinate q the column x_q solves S(mu) x_q = e_q by the route's conjugate gradients: block-
 *     Jacobi preconditioning, psba_set_solver's tol and max_iter, the stop rule of psba_schur_solve on this route.
 *   * For a masked or held chosen coordinate nothing is solved: its row and column of C and its row of cols are exactly
 *     +0.0, not the inverse of the placeholder.
 *   * C is taken from the solved columns: block (a, b) of the chosen list with position a >= b from the columns solved
 *     for camera sel[b], rows of camera sel[a], written to both sides; inside a diagonal block the lower triangle is the
 *     matrix.  So C is bit-symmetric.
 *   * C = scale (...); cols is not scaled.
 *   * mu = 0 needs a gauge, held poses or priors; mu > 0 gives a regularised inverse and NOT a covariance.
 * Columns are independent: a column's bits, iteration count and relres depend neither on which other cameras are
 * chosen nor on their order; every inner product is summed in a fixed order and there are no floating-point atomics, so
 * two calls on the same state return the same bits.
 * reassemble != 0: linearizes with (1, 1) unless that linearization is current, then runs psba_schur_assemble(mu); the
 * handle is left as after that call (a psba_schur_solve may follow).  reassemble == 0: works on the blocks as they
 * stand, in the state of psba_get_sparse_S -- so also on the blocks of psba_set_sparse_S.  The verb uses buffers of its
 * own (six vectors of 16 nA doubles per panel, at most 8 panels at a time, allocated at first use and dropped at an
 * upload): a later psba_schur_solve, psba_backsub or psba_levmar runs as on a handle that never called it.
 * Returns PSBA_OK, PSBA_NOT_SPD (a bad pivot of a diagonal block, p.Sp <= 0 in any column, a residual that is not
 * finite) or PSBA_PCG_MAXIT (some column used up max_iter: iters and relres say which; C is still written), and
 * synchronises.  PSBA_E_STATE before an upload, while a try is in flight and on every handle that does not run
 * PSBA_SOLVER_SPARSE on blocks of 11 / 16 (dense free-intrinsics handles: psba_free_covariance_compute; six-parameter
 * blocks: psba_covariance_compute); PSBA_E_INVALID for a mu that is not finite and >= 0, a scale that is not finite
 * and > 0, n_sel < 1, an index out of range or listed twice, C == NULL.  A refused call changes nothing.
 * Not here: shared intrinsics, rank layouts.  Point covariances: psba_sparse_point_covariance. */
int psba_sparse_camera_covariance(psba_handle h, double mu, double scale, int reassemble, int n_sel, const int *sel,
                                  double *C      /* (n_sel cnp)^2 row-major, may not be NULL */,
                                  double *cols   /* [n_sel cnp][nA]: row q = the column of S(mu)^-1 of chosen coordinate q, NOT scaled; may be NULL */,
                                  int *iters     /* [n_sel cnp], may be NULL */,
                                  double *relres /* [n_sel cnp], may be NULL */);
/* ---- covariance of chosen points under PSBA_SOLVER_SPARSE on camera blocks of 11 / 16 ----------------
 * The other half of psba_sparse_camera_covariance: how well chosen 3-D points (control, check and tie points) are
 * determined.  psba_get_free_point_covariance needs the dense inverse and keeps refusing a sparse handle.  Here three
 * right-hand sides per point are solved, five points to a panel of 16 columns (kernels_free_pcg_points.hip).
 *   * The linearization is psba_linearize(h, 1, 1) at the current parameters, as for psba_sparse_camera_covariance: the
 *     mask, the per-camera masks, held poses and points, priors, observation weighting and the damping rule are in S, V
 *     and Y.
 *   * For a chosen point i and c < 3 the right-hand side b_{i,c} holds, in its rows of camera j in cams(i), column c of
 *     Y_ij (cnp x 3, as k_free_Y stored it for this mu); every other row is +0.0.  The column x_{i,c} solves
 *     S(mu) x = b_{i,c} by the route's conjugate gradients: block-Jacobi preconditioning, psba_set_solver's tol and
 *     max_iter, the stop rule of psba_schur_solve on this route with r.r judged against this column's own b.b.
 *   * Block (a, b) of the chosen list is scale [ delta_ab V*_a^-1 + sum_{j in cams(a)} Y_aj^T x_b[rows of j] ], the sum
 *     in ascending j.  V*_i = V_i + mu D_i is rebuilt with the route's own damping (D = I, or Marquardt's diagonal of
 *     psba_set_damping) and inverted by the closed form; |det| < 1e-16 gives PSBA_SINGULAR_V.
 *   * Block (a, b) with position a >= b is taken from the columns solved for sel_pts[b] and written to both sides;
 *     inside a diagonal block the lower triangle is the matrix.  So C is bit-symmetric.
 *   * A held point: nothing is solved; its rows and columns of C and its rows of cols are exactly +0.0, its iters 0 and
 *     its relres 0.  A point without observations, and one whose blocks Y are all zero: b = 0, the columns start stopped
 *     with x = 0 (iters 0, relres 0) and the diagonal block is scale V*^-1.
 *   * Masked and held-pose coordinates need no case of their own: their rows of W, and hence of Y, are +0.0 by
 *     construction, so b, every iterate and cols are zero there (cols: +0.0).
 *   * C = scale (...); cols is not scaled.
 *   * mu = 0 needs a gauge, held poses or priors; mu > 0 gives a regularised inverse and NOT a covariance.
 * Columns are independent: a column's bits, iteration count and relres depend on none of: which other points are
 * chosen, their order, the column's position in its panel, the batch (at most 8 panels = 40 points at a time); two calls
 * on the same state return the same bits.
 * State, arguments and reassemble are those of psba_sparse_camera_covariance; with reassemble == 0, mu must be the mu of
 * the psba_schur_assemble whose blocks, V and Y stand (it rebuilds V*).  The verb uses that verb's panel buffers and
 * touches none of dp, the solver's vectors and scalars or the try's status words: a later psba_schur_solve, psba_backsub
 * or psba_levmar runs as on a handle that never called it.  Returns PSBA_OK, PSBA_NOT_SPD, PSBA_SINGULAR_V (a chosen
 * V*_i) or PSBA_PCG_MAXIT (some column used up max_iter: iters and relres say which; C is still written), and
 * synchronises.  PSBA_E_STATE as there; PSBA_E_INVALID for a mu that is not finite and >= 0, a scale that is not finite
 * and > 0, n_sel < 1, a point out of range or listed twice, C == NULL.  A refused call changes nothing.
 * Not here: the camera-point cross blocks C_ab, all points at once, shared intrinsics, rank layouts. */
int psba_sparse_point_covariance(psba_handle h, double mu, double scale, int reassemble, int n_sel, const int *sel_pts,
                                 double *C      /* (3 n_sel)^2 row-major, may not be NULL */,
                                 double *cols   /* [3 n_sel][nA]: row 3 a + c = x_{sel_pts[a], c}, NOT scaled; may be NULL */,
                                 int *iters     /* [3 n_sel], may be NULL */,
                                 double *relres /* [3 n_sel], may be NULL */);
/* mirror verb of the product kernel of psba_sparse_camera_covariance: Y = S X for n_panels panels [nA][16] (column
 * n of panel m at X[(m nA + r) 16 + n]), in the state of psba_sparse_S_times.  A panel's result does not depend on its
 * position. */
int psba_sparse_S_times_many(psba_handle h, int n_panels, const double *X /* [n_panels][nA][16] */, double *Y);
/* The verbs that work on the dense reduce buffer or the Cholesky chain -- psba_SPDinv_matVec,
 * psba_get_reduce_buffer, psba_set_reduce_buffer, psba_chol_dist_begin / _superpanel / _block / _finish,
 * psba_get_cholmod_factor, psba_covariance_compute -- return PSBA_E_STATE under PSBA_SOLVER_PCG before they copy or
 * launch anything; the sba_func.h mirror's psba_compute_S / psba_compute_ea return PSBA_E_INVALID. */
/* flags[nCams (nCams + 1) / 2]: 1 where block tri(j) + k (k <= j) has a product, i.e. cameras j and k see a common point */
int psba_sparse_pattern(int nCams, int n3Dpts, int n2Dprojs, const int *iidx, const int *jidx, unsigned char *flags);
int psba_set_sparse_pattern(psba_handle h, const unsigned char *flags, long long n);

/* ---- the dense factorization sharded over ranks (large matrices: the two-level chain) --------------
 * The reference factors S on one device (PSBA/cl_spdinv.cpp:18-40, CL_files/SPD_inv.cl:165-179).
 * Here every rank holds the complete S after the all-reduce and factors the super-panels (NB columns)
 * itself; the K = NB update of everything to their right -- nearly all of the n^3 / 3 flops -- is
 * shared: a rank updates the 64-column blocks B (columns [64 B, 64 B + 64)) with B % nranks == rank,
 * and before a super-panel is factored the owners of its blocks send them (rows 64 B .. n32, the
 * e_a row included, packed row by row) to everybody.  With a communicator psba_schur_solve runs this
 * by itself (ncclBroadcast; PSBA_CHOL_REPLICATED=1 keeps the factorization replicated); the pieces
 * below let a host with its own transport -- or a test with several handles -- drive it:
 *   psba_chol_dist_shape     n32, NB, and whether the matrix is large enough for the sharded chain
 *   psba_chol_dist_begin     the first diagonal block
 *   psba_chol_dist_superpanel(J)  the 32-column steps of the super-panel at column J (its columns
 *                            must be complete on this rank) and this rank's share of the update
 *   psba_chol_dist_block(B, set, buf, &n)  get (set = 0) / set the packed block B; n = its doubles
 *   psba_chol_dist_finish    the backward solve: dpa, as after psba_schur_solve */
int psba_chol_dist_shape(psba_handle h, int *n32, int *NB, int *sharded);
/* read-only: the route psba_schur_solve / psba_SPDinv_matVec take for this handle's matrix, from the same size
 * limits and PSBA_CHOL_* switches the chain reads when it is enqueued (nothing is launched).  out8 =
 * {n32, fused (k_cholg_panel with the identity rows + k_cholg_solve), fused2 (k_cholg_panel without them + the
 * backward solve), blocked (the two-level chain; neither of the three: the flat trsm + update chain), NB,
 * diagonal-only steps (first super-panel), look-ahead, single workgroup (PSBA_CHOL_SINGLE)} */
int psba_chol_shape(psba_handle h, int *out8);
/* host only: the column exchange in front of the super-panel at column JE, as the RCCL path performs it --
 * out4[k] = {block B, owner rank (B mod nranks), slot of the exchange buffer, doubles}; returns the number of
 * blocks (0: none, the last super-panel), < 0 if cap is too small.  The owner of block B packs rows 64 B .. n32
 * (the e_a row) of its min(64, n32 - 64 B) columns, everybody else unpacks them. */
int psba_chol_dist_exchange_plan(int n32, int NB, int nranks, int JE, long long *out4, int cap);
int psba_chol_dist_begin(psba_handle h);
int psba_chol_dist_superpanel(psba_handle h, int J);
int psba_chol_dist_block(psba_handle h, int B, int set, double *buf, long long *n_doubles);
int psba_chol_dist_finish(psba_handle h);

/* ---- test hook: the static schedule of the S-assembly kernel, built on the host only ----
 * (no device needed).  The reference decides the same placement per launch through its
 * blkIdx_buffer look-ups (CL_files/compute_S.cl:13-22); here it is data that can be checked.
 * info[0..5] = groups, workgroups, item slots, products, slab doubles, blocks nC(nC+1)/2.
 * psba_schur_plan_copy: items[info[2]]; wg[info[1]][8] = group, blocks in partition, obs0, pt0,
 * first item, end item, slab offset, end of the pair items (the list begins with items that carry
 * two products of one observation a -- partners a - boff and a - boff + 1 -- as 18 bits a - obs0,
 * 16 bits i - pt0, 8 bits boff, 10 + 10 bits block positions; the single-product items follow:
 * 24 / 22 / 8 / 10 bits); blockpos[info[5]]; glo[groups+1]: group g owns the blocks
 * [glo[g], glo[g+1]) of the canonical order j (j + 1) / 2 + k.  Any pointer may be NULL. */
typedef struct psba_schur_plan *psba_schur_plan_t;
psba_schur_plan_t psba_schur_plan_create(int nCams, int n3Dpts, int n2Dprojs, const int *iidx,
                                         const int *jidx);
int psba_schur_plan_info(psba_schur_plan_t p, long long info[8]); /* info[6] > 0: the runs layout (items as [turn][512] per workgroup, a thread's consecutive items grouped into runs of one position), number of runs; info[7] = pair items */
int psba_schur_plan_copy(psba_schur_plan_t p, unsigned long long *items, long long *wg,
                         int *blockpos, int *glo);
void psba_schur_plan_destroy(psba_schur_plan_t p);

/* ---- test hook: the product lists of the owner route (K2 for >= 2048 cameras, for points seen by more
 * cameras than a tile holds, and for the block-sparse S), built on the host only.  Every product
 * Y_a W_b^T belongs to the block (camera of a, camera of b) of the lower block triangle; a thread owns a
 * unit = (block, segment of its products), 64 units to a wave, a wave's products in ELL rows.
 * info[0..3] = waves, ELL rows, products, blocks in the block list.
 * psba_owner_plan_copy: waves[waves][2] = first ELL row, rows; units[64 waves][4] = j, k, multi (the block
 * has several units), slot in the block list (-1: idle lane); prod[64 rows][2] = observations (a, b), a = -1
 * padding; blocks[blocks][2] = (j, k) in canonical order; diag_slot[nCams].  pattern (may be NULL): the
 * union pattern of psba_sparse_pattern -- blocks flagged there exist even without a product here. */
typedef struct psba_owner_plan *psba_owner_plan_t;
psba_owner_plan_t psba_owner_plan_create(int nCams, int n3Dpts, int n2Dprojs, const int *iidx, const int *jidx,
                                         const unsigned char *pattern);
int psba_owner_plan_info(psba_owner_plan_t p, long long info[4]);
int psba_owner_plan_copy(psba_owner_plan_t p, long long *waves, int *units, int *prod, int *blocks, int *diag_slot);
void psba_owner_plan_destroy(psba_owner_plan_t p);

/* ---- test hook: the S-assembly schedule of the 16-parameter camera block (PSBA_CAMERA_FREE_KD), host only.
 * Every product Y_a W_b^T (b <= a, both observations of one point) belongs to the block (camera of a, camera of b)
 * of the lower block triangle; the products are sorted by block (ascending (j, k)), inside a block by point, and a
 * block's list is cut into segments of at most seg_len products (PSBA_FKD_SEG at upload; one wave per segment).
 * info[0..3] = blocks, segments, products, partial tiles (segments of blocks that have several).
 * psba_blockprod_plan_copy: blocks[blocks][2] = (j, k); segs[segments][3] = block, first product, end product;
 * prods[products][2] = observations (a, b).  Any pointer may be NULL. */
typedef struct psba_blockprod_plan *psba_blockprod_plan_t;
psba_blockprod_plan_t psba_blockprod_plan_create(int nCams, int n3Dpts, int n2Dprojs, const int *iidx, const int *jidx,
                                                 int seg_len);
int psba_blockprod_plan_info(psba_blockprod_plan_t p, long long info[4]);
int psba_blockprod_plan_copy(psba_blockprod_plan_t p, int *blocks, int *segs, int *prods);
/* The block list and row walk PSBA_SOLVER_SPARSE derives from the plan on these camera blocks: the plan's blocks plus a
 * diagonal block for every camera without a product, ascending by (j, k).  info[0..2] = stored blocks, diagonal blocks
 * added, row entries.  jk[stored][2]; diag_slot[nCams]; rowptr[nCams + 1]; rowent[entries][2] = (slot, other camera |
 * how << 28) with how 0 = as stored, 1 = transposed, 2 = the diagonal block (read through its lower triangle).  Any
 * pointer may be NULL. */
int psba_blockprod_plan_rows_info(psba_blockprod_plan_t p, long long info[3]);
int psba_blockprod_plan_rows(psba_blockprod_plan_t p, int *jk, int *diag_slot, int *rowptr, int *rowent);
void psba_blockprod_plan_destroy(psba_blockprod_plan_t p);

#ifdef PSBA_BUILD_EXPERIMENTS
/* (Only in a library built with PSBA_BUILD_EXPERIMENTS=1: round 3's ring route is an experiment that lost,
 * DESIGN 5c, and is not part of the product library.)
 * ---- test hook: the schedule of the S-assembly kernel's ring route (few cameras), host only ----
 * The lower block triangle of S (reference CL_files/compute_S.cl:6-78) is cut into nR ranges of the
 * canonical block order and the point sequence into nS stretches; a workgroup per (range, stretch)
 * replays per-step lists: which runs of W records (up to 7, contiguous in W) are loaded into
 * which slots of its LDS, which observations get their Y = W V^-1 formed (jobs), and which
 * product every consumer lane takes.
 * info[0..15] = nR, nS, workgroups (0: the route does not apply), steps, lane entries, page
 * loads, jobs, products, lane-steps, lanes per workgroup, LDS slots, records per page load at most, steps between a
 * load and its first use, lane_blk entries, blk_lane0 entries, record loads.
 * psba_ring_plan_copy: wg[workgroups][13] = first block, blocks, first row, rows, copy, steps,
 * the first index of the workgroup in steps / entries / ops / jobs / lane_blk / blk_lane0, and its
 * W slots (Y slots are numbered from 0 and live behind them);
 * steps[.][4] = page loads [begin, end) and jobs [begin, end) of the step, relative to the
 * workgroup; entries[step][lanes] = partner W slot | Y slot << 16 (0xFFFFFFFF: idle);
 * ops[.][2] = first observation of a page load, first W slot | records << 16;
 * jobs[.][4] = observation, point, W slot | Y slot << 16, e_a row relative to the first row or -1;
 * lane_blk[wg][lanes] = block (relative) a lane owns; blk_lane0[.] per workgroup blocks + 1 first
 * lanes; rb[nR + 1] block range bounds.  Any pointer may be NULL. */
typedef struct psba_ring_plan *psba_ring_plan_t;
psba_ring_plan_t psba_ring_plan_create(int nCams, int n3Dpts, int n2Dprojs, const int *iidx,
                                       const int *jidx);
int psba_ring_plan_info(psba_ring_plan_t p, long long info[16]);
int psba_ring_plan_copy(psba_ring_plan_t p, long long *wg, int *steps, unsigned *entries, int *ops,
                        int *jobs, int *lane_blk, int *blk_lane0, int *rb);
void psba_ring_plan_destroy(psba_ring_plan_t p);
#endif /* PSBA_BUILD_EXPERIMENTS */

#ifdef __cplusplus
}
#endif
#endif
