"""ctypes binding of include/psba_hip.h (one method per entry point, same names)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PSBA_LIB: another build of the library (psba_amd/libpsba_hip_exp.so = PSBA_BUILD_EXPERIMENTS=1 python psba_amd/build.py)
lib_path = os.environ.get("PSBA_LIB") or os.path.join(_HERE, "libpsba_hip.so")

if not os.path.exists(lib_path):
    raise ImportError(
        f"{lib_path} is missing: build the HIP extension first (python -m psba_amd.build, or "
        "__graft_entry__.build()). psba_amd has no CPU fallback.")
lib = C.CDLL(lib_path)

PSBA_OK, PSBA_NOT_SPD, PSBA_SINGULAR_V = 0, 1, 2
PARAMS_CUR, PARAMS_NEW = 0, 1
LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY, LOSS_SOFT_L1 = 0, 1, 2, 3
CAMERA_FIXED_K, CAMERA_FREE_K, CAMERA_FREE_KD = 0, 1, 2
SOLVER_DENSE, SOLVER_PCG, SOLVER_SPARSE = 0, 1, 2
INTRINSICS_BAL = (1, 0, 0, 0, 0, 1, 1, 0, 0, 0)  # the free intrinsics of Bundle Adjustment in the Large: f, k1, k2
DAMPING_IDENTITY, DAMPING_MARQUARDT = 0, 1
ITER_TURN_TO_LM, ITER_TURN_TO_TR, ITER_CONTINUE, ITER_ERR = 1, 2, 3, 4
ITER_DP_NO_CHANGE, ITER_ERR_SMALL_ENOUGH, ITER_PASS = 5, 6, 7
K_LINEARIZE, K_SCHUR, K_CHOLESKY, K_BACKSUB, K_RESIDUAL, K_ALLREDUCE, K_SCHUR_REDUCE = range(7)
KERNEL_NAMES = ["linearize", "schur", "cholesky", "backsub", "residual", "allreduce", "schur_reduce"]

_h = C.c_void_p
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class TryScalars(C.Structure):
    _fields_ = [("status", C.c_int), ("dp_l2", C.c_double), ("gain_den", C.c_double),
                ("new_cost", C.c_double), ("newp_l2", C.c_double)]


class LmOptions(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("tr_handoff", C.c_int), ("verbose", C.c_int),
                ("log_cap", C.c_int), ("start_itno", C.c_int), ("init_mu", C.c_double),
                ("stop_cost", C.c_double)]


class LmResult(C.Structure):
    _fields_ = [("flag", C.c_int), ("iters", C.c_int), ("tries", C.c_int), ("init_err", C.c_double),
                ("final_err", C.c_double), ("mu0", C.c_double), ("mu_final", C.c_double),
                ("n_log", C.c_int), ("seconds", C.c_double), ("pcg_unconverged", C.c_int)]


class TrOptions(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("start_itno", C.c_int), ("verbose", C.c_int), ("log_cap", C.c_int),
                ("init_lambda", C.c_double)]


class TrResult(C.Structure):
    _fields_ = [("flag", C.c_int), ("iters", C.c_int), ("tries", C.c_int), ("chol_fail", C.c_int),
                ("init_err", C.c_double), ("final_err", C.c_double), ("lambda_", C.c_double),
                ("delta", C.c_double), ("n_log", C.c_int), ("seconds", C.c_double)]


class SolveResult(C.Structure):
    _fields_ = [("flag", C.c_int), ("iters", C.c_int), ("lm_calls", C.c_int), ("tr_calls", C.c_int),
                ("init_err", C.c_double), ("final_err", C.c_double), ("seconds", C.c_double)]


class CProblem(C.Structure):
    _fields_ = [("nCams", C.c_int), ("n3Dpts", C.c_int), ("n2Dprojs", C.c_int), ("Kparas", _dp),
                ("impts", _dp), ("initrot", _dp), ("camsEx", _dp), ("pts3D", _dp), ("iidx", _ip),
                ("jidx", _ip)]


class CProblemEx(C.Structure):
    _fields_ = [("base", CProblem), ("kc", _dp), ("cov", _dp)]


# every symbol include/psba_hip.h declares: (name, restype, argtypes)
SIGNATURES = [
    ("psba_create", C.c_int, [C.c_int, C.POINTER(_h)]),
    ("psba_destroy", C.c_int, [_h]),
    ("psba_last_error", C.c_char_p, [_h]),
    ("psba_version", C.c_char_p, []),
    ("psba_upload_problem", C.c_int, [_h, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip]),
    ("psba_set_params", C.c_int, [_h, _dp, _dp]),
    ("psba_reset_params", C.c_int, [_h]),
    ("psba_get_params", C.c_int, [_h, C.c_int, _dp, _dp]),
    ("psba_get_dims", C.c_int, [_h, _ip, _ip, _ip]),
    ("psba_schur_path", C.c_int, [_h, C.POINTER(C.c_int)]),
    ("psba_lm_ran_lean", C.c_int, [_h, C.POINTER(C.c_int)]),
    ("psba_linearize_lean", C.c_int, [_h]),
    ("psba_residual", C.c_int, [_h, C.c_int, _dp]),
    ("psba_linearize", C.c_int, [_h, C.c_double, C.c_double]),
    ("psba_max_diag", C.c_int, [_h, _dp]),
    ("psba_begin", C.c_int, [_h, C.c_double, C.c_double, _dp, _dp]),
    ("psba_schur_assemble", C.c_int, [_h, C.c_double]),
    ("psba_schur_reduce", C.c_int, [_h]),
    ("psba_schur_solve", C.c_int, [_h]),
    ("psba_backsub", C.c_int, [_h, C.c_double, C.POINTER(TryScalars)]),
    ("psba_backsub_async", C.c_int, [_h, C.c_double]),
    ("psba_linearize_ahead", C.c_int, [_h]),
    ("psba_backsub_wait", C.c_int, [_h, C.POINTER(TryScalars)]),
    ("psba_accept", C.c_int, [_h]),
    ("psba_scal_block_check", C.c_int, [_dp, C.c_double, _dp]),
    ("psba_scal_block_take", C.c_int, [_dp, C.c_double, _dp]),
    ("psba_publish_stats", C.c_int, [_h, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    ("psba_test_publish", C.c_int, [_h, _dp, C.c_int, _dp]),
    ("psba_compute_exQT", C.c_int, [_h, C.c_int, _dp]),
    ("psba_compute_jacobiQT", C.c_int, [_h, _dp, _dp]),
    ("psba_compute_U", C.c_int, [_h, C.c_double, _dp]),
    ("psba_compute_V", C.c_int, [_h, C.c_double, _dp]),
    ("psba_maxElmOfUV", C.c_int, [_h, _dp]),
    ("psba_update_UV", C.c_int, [_h, C.c_double, _dp, _dp]),
    ("psba_restore_UVdiag", C.c_int, [_h]),
    ("psba_compute_Vinv", C.c_int, [_h, _dp]),
    ("psba_compute_Wblks", C.c_int, [_h, C.c_double, _dp]),
    ("psba_compute_Yblks", C.c_int, [_h, _dp]),
    ("psba_compute_S", C.c_int, [_h, _dp]),
    ("psba_compute_g", C.c_int, [_h, C.c_double, _dp]),
    ("psba_compute_ea", C.c_int, [_h, _dp]),
    ("psba_SPDinv_matVec", C.c_int, [_h, _dp]),
    ("psba_compute_eb", C.c_int, [_h, _dp]),
    ("psba_compute_dpb", C.c_int, [_h, _dp]),
    ("psba_compute_newp", C.c_int, [_h, _dp]),
    ("psba_update_p", C.c_int, [_h, _dp]),
    ("psba_lm_default_options", None, [C.POINTER(LmOptions)]),
    ("psba_levmar", C.c_int, [_h, C.POINTER(LmOptions), C.POINTER(LmResult), _dp]),
    ("psba_partition_points", C.c_int, [C.c_int, _ip, C.c_int, C.c_int, _ip]),
    ("psba_comm_unique_id", C.c_int, [C.c_void_p]),
    ("psba_comm_init", C.c_int, [_h, C.c_int, C.c_int, C.c_void_p]),
    ("psba_comm_rank", C.c_int, [_h, _ip, _ip]),
    ("psba_set_rank_layout", C.c_int, [_h, C.c_int, C.c_int]),
    ("psba_reduce_buffer_size", C.c_int, [_h, C.POINTER(C.c_longlong)]),
    ("psba_get_reduce_buffer", C.c_int, [_h, _dp]),
    ("psba_set_reduce_buffer", C.c_int, [_h, _dp]),
    ("psba_read_problem", C.c_int, [C.c_char_p, C.c_char_p, _dp, C.POINTER(CProblem)]),
    ("psba_free_problem", None, [C.POINTER(CProblem)]),
    ("psba_profile_enable", C.c_int, [_h, C.c_int]),
    ("psba_profile_reset", C.c_int, [_h]),
    ("psba_profile_get", C.c_int, [_h, C.c_int, _dp, _ip]),
    ("psba_algorithmic_bytes", C.c_int, [_h, C.c_int, _dp]),
    ("psba_compute_Jmultiply", C.c_int, [_h, _dp, _dp]),
    ("psba_jmul_dots", C.c_int, [_h, _dp, _dp, _dp]),
    ("psba_get_gradient", C.c_int, [_h, _dp]),
    ("psba_get_dp", C.c_int, [_h, _dp]),
    ("psba_set_step", C.c_int, [_h, _dp]),
    ("psba_cholmod_lambda", C.c_int, [_h, C.c_int, _dp, _dp]),
    ("psba_get_cholmod_factor", C.c_int, [_h, _dp]),
    ("psba_get_free_obs_blocks", C.c_int, [_h, _dp, _dp]),
    ("psba_tr_default_options", None, [C.POINTER(TrOptions)]),
    ("psba_trust_region", C.c_int, [_h, C.POINTER(TrOptions), C.POINTER(TrResult), _dp]),
    ("psba_solve", C.c_int, [_h, C.c_int, C.c_int, C.POINTER(SolveResult)]),
    ("psba_write_problem", C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int]),
    ("psba_convert_bal", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, _dp]),
    ("psba_allreduce_scalars", C.c_int, [_h, _dp, C.c_int]),
    ("psba_set_solver", C.c_int, [_h, C.c_int, C.c_double, C.c_int]),
    ("psba_pcg_info", C.c_int, [_h, _ip, _dp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    ("psba_get_sparse_S", C.c_int, [_h, _ip, _dp, _dp]),
    ("psba_set_sparse_S", C.c_int, [_h, _dp, _dp]),
    ("psba_sparse_S_times", C.c_int, [_h, _dp, _dp]),
    ("psba_get_sparse_precond", C.c_int, [_h, _dp]),
    ("psba_sparse_S_times_many", C.c_int, [_h, C.c_int, _dp, _dp]),
    ("psba_sparse_camera_covariance", C.c_int, [_h, C.c_double, C.c_double, C.c_int, C.c_int, _ip, _dp, _dp, _ip, _dp]),
    ("psba_sparse_point_covariance", C.c_int, [_h, C.c_double, C.c_double, C.c_int, C.c_int, _ip, _dp, _dp, _ip, _dp]),
    ("psba_sparse_pattern", C.c_int, [C.c_int, C.c_int, C.c_int, _ip, _ip, C.POINTER(C.c_ubyte)]),
    ("psba_set_sparse_pattern", C.c_int, [_h, C.POINTER(C.c_ubyte), C.c_longlong]),
    ("psba_set_camera_model", C.c_int, [_h, C.c_int]),
    ("psba_camera_block", C.c_int, [_h, _ip]),
    ("psba_set_distortion", C.c_int, [_h, _dp]),
    ("psba_set_obs_covariance", C.c_int, [_h, _dp]),
    ("psba_lens_model", C.c_int, [_h, _ip, _ip]),
    ("psba_set_robust_loss", C.c_int, [_h, C.c_int, C.c_double]),
    ("psba_robust_loss", C.c_int, [_h, _ip, _dp]),
    ("psba_obs_sq_residuals", C.c_int, [_h, C.c_int, _dp]),
    ("psba_set_fixed", C.c_int, [_h, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    ("psba_fixed_counts", C.c_int, [_h, _ip, _ip]),
    ("psba_set_held", C.c_int, [_h, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    ("psba_held_counts", C.c_int, [_h, _ip, _ip]),
    ("psba_set_priors", C.c_int, [_h, _dp, _dp, _dp, _dp]),
    ("psba_prior_counts", C.c_int, [_h, _ip, _ip]),
    ("psba_prior_cost", C.c_int, [_h, C.c_int, _dp, _dp]),
    ("psba_set_obs_weighting", C.c_int, [_h, C.c_int, C.c_double, _dp]),
    ("psba_obs_weighting", C.c_int, [_h, _ip, _dp, _ip]),
    ("psba_get_obs_weights", C.c_int, [_h, C.c_int, _dp, _dp]),
    ("psba_read_problem_ex", C.c_int, [C.c_char_p, C.c_char_p, _dp, C.POINTER(CProblemEx)]),
    ("psba_free_problem_ex", None, [C.POINTER(CProblemEx)]),
    ("psba_convert_bal_kd", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p]),
    ("psba_chol_dist_exchange_plan", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]),
    ("psba_chol_dist_shape", C.c_int, [_h, _ip, _ip, _ip]),
    ("psba_chol_shape", C.c_int, [_h, _ip]),
    ("psba_chol_dist_begin", C.c_int, [_h]),
    ("psba_chol_dist_superpanel", C.c_int, [_h, C.c_int]),
    ("psba_chol_dist_block", C.c_int, [_h, C.c_int, C.c_int, _dp, C.POINTER(C.c_longlong)]),
    ("psba_chol_dist_finish", C.c_int, [_h]),
    ("psba_schur_plan_create", C.c_void_p, [C.c_int, C.c_int, C.c_int, _ip, _ip]),
    ("psba_schur_plan_info", C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    ("psba_schur_plan_copy", C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_longlong), _ip, _ip]),
    ("psba_schur_plan_destroy", None, [C.c_void_p]),
    ("psba_owner_plan_create", C.c_void_p, [C.c_int, C.c_int, C.c_int, _ip, _ip, C.POINTER(C.c_ubyte)]),
    ("psba_owner_plan_info", C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    ("psba_owner_plan_copy", C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), _ip, _ip, _ip, _ip]),
    ("psba_owner_plan_destroy", None, [C.c_void_p]),
    ("psba_set_intrinsics_mask", C.c_int, [_h, C.POINTER(C.c_ubyte)]),
    ("psba_intrinsics_mask", C.c_int, [_h, C.POINTER(C.c_ubyte)]),
    ("psba_set_camera_masks", C.c_int, [_h, C.POINTER(C.c_ubyte)]),
    ("psba_camera_masks", C.c_int, [_h, C.POINTER(C.c_ubyte)]),
    ("psba_set_intrinsics_groups", C.c_int, [_h, C.POINTER(C.c_int)]),
    ("psba_intrinsics_groups", C.c_int, [_h, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("psba_set_sparse_intrinsics_groups", C.c_int, [_h, C.POINTER(C.c_int)]),
    ("psba_set_damping", C.c_int, [_h, C.c_int, C.c_double, C.c_double]),
    ("psba_damping", C.c_int, [_h, _ip, _dp, _dp]),
    ("psba_get_damping_diag", C.c_int, [_h, _dp]),
    ("psba_blockprod_plan_create", C.c_void_p, [C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_int]),
    ("psba_blockprod_plan_info", C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    ("psba_blockprod_plan_copy", C.c_int, [C.c_void_p, _ip, _ip, _ip]),
    ("psba_blockprod_plan_rows_info", C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    ("psba_blockprod_plan_rows", C.c_int, [C.c_void_p, _ip, _ip, _ip, _ip]),
    ("psba_blockprod_plan_destroy", None, [C.c_void_p]),
    ("psba_covariance_compute", C.c_int, [_h, C.c_double, C.c_double, C.c_int]),
    ("psba_get_camera_covariance", C.c_int, [_h, C.c_int, _ip, _dp]),
    ("psba_get_covariance_matrix", C.c_int, [_h, _dp]),
    ("psba_get_point_covariance", C.c_int, [_h, _dp]),
    ("psba_covariance_times", C.c_int, [_h, _dp]),
    ("psba_free_covariance_compute", C.c_int, [_h, C.c_double, C.c_double, C.c_int]),
    ("psba_get_free_camera_covariance", C.c_int, [_h, C.c_int, _ip, _dp]),
    ("psba_get_free_covariance_matrix", C.c_int, [_h, _dp]),
    ("psba_get_free_point_covariance", C.c_int, [_h, _dp]),
    ("psba_get_free_sigmas", C.c_int, [_h, _dp]),
    ("psba_get_free_point_blocks", C.c_int, [_h, _dp, _dp]),
    ("psba_free_covariance_times", C.c_int, [_h, _dp]),
]
# only in a library built with PSBA_BUILD_EXPERIMENTS=1 (round 3's rejected ring route and its test hooks)
EXPERIMENT_SIGNATURES = [
    ("psba_ring_plan_create", C.c_void_p, [C.c_int, C.c_int, C.c_int, _ip, _ip]),
    ("psba_ring_plan_info", C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    ("psba_ring_plan_copy", C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), _ip, C.POINTER(C.c_uint), _ip, _ip, _ip, _ip, _ip]),
    ("psba_ring_plan_destroy", None, [C.c_void_p]),
]
HAS_EXPERIMENTS = hasattr(lib, "psba_ring_plan_create")
for _name, _res, _args in SIGNATURES + (EXPERIMENT_SIGNATURES if HAS_EXPERIMENTS else []):
    _f = getattr(lib, _name)
    _f.restype = _res
    _f.argtypes = _args


class PsbaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"psba error {code}: {msg}")
        self.code = code


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


def _c(a, dt=np.float64):
    return np.ascontiguousarray(a, dtype=dt)


class Problem(dict):
    """K[nC,5] initrot[nC,4] cams[nC,6] pts[nP,3] impts[nO,2] iidx[nO] jidx[nO] nC nP nO.
    Optional: kc[nC,5], cov[nO,2,2] (read_problem_ex); fixed_cams[nC], fixed_pts[nP] (masks for Psba.set_fixed)."""


def sparse_pattern(prob):
    """psba_sparse_pattern (host only): one byte per block tri(j) + k of the lower block triangle."""
    nC = int(prob["nC"])
    flags = np.zeros(nC * (nC + 1) // 2, dtype=np.uint8)
    ii = np.ascontiguousarray(prob["iidx"], dtype=np.int32)
    jj = np.ascontiguousarray(prob["jidx"], dtype=np.int32)
    rc = lib.psba_sparse_pattern(nC, int(prob["nP"]), int(prob["nO"]), _i(ii), _i(jj),
                                 flags.ctypes.data_as(C.POINTER(C.c_ubyte)))
    if rc != 0:
        raise PsbaError(rc, "psba_sparse_pattern failed")
    return flags


def _problem_from(cp):
    nC, nP, nO = cp.nCams, cp.n3Dpts, cp.n2Dprojs
    arr = lambda p, n, shape: np.ctypeslib.as_array(p, shape=(n,)).copy().reshape(shape)
    return Problem(K=arr(cp.Kparas, 5 * nC, (nC, 5)), initrot=arr(cp.initrot, 4 * nC, (nC, 4)),
                  cams=arr(cp.camsEx, 6 * nC, (nC, 6)), pts=arr(cp.pts3D, 3 * nP, (nP, 3)),
                  impts=arr(cp.impts, 2 * nO, (nO, 2)), iidx=arr(cp.iidx, nO, (nO,)).astype(np.int32),
                  jidx=arr(cp.jidx, nO, (nO,)).astype(np.int32), nC=nC, nP=nP, nO=nO)


def read_problem(cams_file, pts_file, fixedK=None):
    """psba_read_problem -> Problem (host only, works without a GPU)."""
    cp = CProblem()
    k = None if fixedK is None else _c(fixedK)
    rc = lib.psba_read_problem(os.fsencode(cams_file), os.fsencode(pts_file), _d(k), C.byref(cp))
    if rc != 0:
        raise PsbaError(rc, f"psba_read_problem({cams_file}, {pts_file}) failed")
    out = _problem_from(cp)
    lib.psba_free_problem(C.byref(cp))
    return out


def read_problem_ex(cams_file, pts_file, fixedK=None):
    """psba_read_problem_ex -> Problem with two more keys: kc [nC, 5] (17-column cams file) and cov [nO, 2, 2]
    (pts file with covariances, observation order), each None when the files do not carry it."""
    cp = CProblemEx()
    k = None if fixedK is None else _c(fixedK)
    rc = lib.psba_read_problem_ex(os.fsencode(cams_file), os.fsencode(pts_file), _d(k), C.byref(cp))
    if rc != 0:
        raise PsbaError(rc, f"psba_read_problem_ex({cams_file}, {pts_file}) failed")
    out = _problem_from(cp.base)
    nC, nO = out["nC"], out["nO"]
    out["kc"] = np.ctypeslib.as_array(cp.kc, shape=(5 * nC,)).copy().reshape(nC, 5) if cp.kc else None
    out["cov"] = np.ctypeslib.as_array(cp.cov, shape=(4 * nO,)).copy().reshape(nO, 2, 2) if cp.cov else None
    lib.psba_free_problem_ex(C.byref(cp))
    return out


def write_problem(cams_file, pts_file, prob, cams=None, pts=None, with_K=True):
    """psba_write_problem: the problem's data with the given (default: its own) parameters."""
    c = _c(prob["cams"] if cams is None else cams)
    p = _c(prob["pts"] if pts is None else pts)
    K, rot, im = _c(prob["K"]), _c(prob["initrot"]), _c(prob["impts"])
    ii, jj = _c(prob["iidx"], np.int32), _c(prob["jidx"], np.int32)
    rc = lib.psba_write_problem(cams_file.encode(), pts_file.encode(), int(prob["nC"]), int(prob["nP"]),
                                int(prob["nO"]), _d(K), _d(rot), _d(c), _d(p), _d(im), _i(ii), _i(jj), int(with_K))
    if rc != 0:
        raise PsbaError(rc, f"psba_write_problem({cams_file}, {pts_file}) failed")


def convert_bal(bal_file, cams_out, pts_out):
    """psba_convert_bal; returns the largest |k1|, |k2| that was dropped."""
    k = C.c_double()
    rc = lib.psba_convert_bal(bal_file.encode(), cams_out.encode(), pts_out.encode(), C.byref(k))
    if rc != 0:
        raise PsbaError(rc, f"psba_convert_bal({bal_file}) failed")
    return k.value


def convert_bal_kd(bal_file, cams_out, pts_out):
    """psba_convert_bal_kd: 17-column cams with kc = (k1, k2, 0, 0, 0) (read back with read_problem_ex)."""
    rc = lib.psba_convert_bal_kd(bal_file.encode(), cams_out.encode(), pts_out.encode())
    if rc != 0:
        raise PsbaError(rc, f"psba_convert_bal_kd({bal_file}) failed")


def partition_points(n_pts, iidx, nranks):
    iidx = _c(iidx, np.int32)
    out = np.zeros(nranks + 1, dtype=np.int32)
    rc = lib.psba_partition_points(int(n_pts), _i(iidx), int(iidx.size), int(nranks), _i(out))
    if rc != 0:
        raise PsbaError(rc, "psba_partition_points failed")
    return out


def schur_plan(n_cams, n_pts, iidx, jidx):
    """The static schedule of the S-assembly kernel for a sparsity pattern (host only, no
    device): dict with groups, items (uint64), wg [nWg,8], blockpos, glo and the counters."""
    iidx = _c(iidx, np.int32)
    jidx = _c(jidx, np.int32)
    p = lib.psba_schur_plan_create(int(n_cams), int(n_pts), int(iidx.size), _i(iidx), _i(jidx))
    if not p:
        raise PsbaError(-1, "psba_schur_plan_create failed")
    try:
        info = (C.c_longlong * 8)()
        lib.psba_schur_plan_info(p, info)
        groups, nwg, nslots, products, slab, nblocks, run_tasks, pair_items = (int(x) for x in info)
        items = np.zeros(nslots, dtype=np.uint64)
        wg = np.zeros((nwg, 8), dtype=np.int64)
        blockpos = np.zeros(nblocks, dtype=np.int32)
        glo = np.zeros(groups + 1, dtype=np.int32)
        lib.psba_schur_plan_copy(p, items.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                 wg.ctypes.data_as(C.POINTER(C.c_longlong)), _i(blockpos), _i(glo))
    finally:
        lib.psba_schur_plan_destroy(p)
    return dict(groups=groups, items=items, wg=wg, blockpos=blockpos, glo=glo, products=products,
                slab_doubles=slab, run_tasks=run_tasks, pair_items=pair_items)


def owner_plan(n_cams, n_pts, iidx, jidx, pattern=None):
    """The product lists of the owner route for a sparsity pattern (host only, no device): dict of the
    arrays psba_owner_plan_copy documents."""
    iidx = _c(iidx, np.int32)
    jidx = _c(jidx, np.int32)
    pat = None if pattern is None else np.ascontiguousarray(pattern, dtype=np.uint8)
    pp = None if pat is None else pat.ctypes.data_as(C.POINTER(C.c_ubyte))
    p = lib.psba_owner_plan_create(int(n_cams), int(n_pts), int(iidx.size), _i(iidx), _i(jidx), pp)
    if not p:
        raise PsbaError(-1, "psba_owner_plan_create failed")
    try:
        info = (C.c_longlong * 4)()
        lib.psba_owner_plan_info(p, info)
        nw, rows, products, nblk = (int(x) for x in info)
        waves = np.zeros((nw, 2), dtype=np.int64)
        units = np.zeros((64 * nw, 4), dtype=np.int32)
        prod = np.zeros((64 * rows, 2), dtype=np.int32)
        blocks = np.zeros((nblk, 2), dtype=np.int32)
        diag = np.zeros(int(n_cams), dtype=np.int32)
        lib.psba_owner_plan_copy(p, waves.ctypes.data_as(C.POINTER(C.c_longlong)), _i(units), _i(prod), _i(blocks), _i(diag))
    finally:
        lib.psba_owner_plan_destroy(p)
    return dict(waves=waves, units=units, prod=prod.reshape(rows, 64, 2), blocks=blocks, diag_slot=diag, products=products)


def blockprod_plan(n_cams, n_pts, iidx, jidx, seg_len):
    """The S-assembly schedule of the 16-parameter camera block (host only, no device): dict with blocks [nb, 2] =
    (j, k), segs [ns, 3] = (block, first, end product), prods [np, 2] = observations (a, b), tiles; and the stored blocks and
    row walk PSBA_SOLVER_SPARSE derives from it: jk [stored, 2], diag_added, diag_slot [nC], rowptr [nC + 1], rowent
    [entries, 2] = (slot, other camera | how << 28)."""
    iidx = _c(iidx, np.int32)
    jidx = _c(jidx, np.int32)
    p = lib.psba_blockprod_plan_create(int(n_cams), int(n_pts), int(iidx.size), _i(iidx), _i(jidx), int(seg_len))
    if not p:
        raise PsbaError(-1, "psba_blockprod_plan_create failed")
    try:
        info = (C.c_longlong * 4)()
        lib.psba_blockprod_plan_info(p, info)
        nb, ns, npr, tiles = (int(x) for x in info)
        blocks = np.zeros((nb, 2), dtype=np.int32)
        segs = np.zeros((ns, 3), dtype=np.int32)
        prods = np.zeros((npr, 2), dtype=np.int32)
        lib.psba_blockprod_plan_copy(p, _i(blocks), _i(segs), _i(prods))
        rinfo = (C.c_longlong * 3)()
        lib.psba_blockprod_plan_rows_info(p, rinfo)
        jk = np.zeros((int(rinfo[0]), 2), dtype=np.int32)
        diag_slot = np.zeros(int(n_cams), dtype=np.int32)
        rowptr = np.zeros(int(n_cams) + 1, dtype=np.int32)
        rowent = np.zeros((int(rinfo[2]), 2), dtype=np.int32)
        lib.psba_blockprod_plan_rows(p, _i(jk), _i(diag_slot), _i(rowptr), _i(rowent))
    finally:
        lib.psba_blockprod_plan_destroy(p)
    return dict(blocks=blocks, segs=segs, prods=prods, tiles=tiles, jk=jk, diag_added=int(rinfo[1]), diag_slot=diag_slot,
                rowptr=rowptr, rowent=rowent)


def chol_dist_exchange_plan(n32, NB, nranks, JE):
    """[(block, owner, slot, doubles)] of the column exchange in front of the super-panel at column JE."""
    out = np.zeros((64, 4), dtype=np.int64)
    n = lib.psba_chol_dist_exchange_plan(int(n32), int(NB), int(nranks), int(JE), out.ctypes.data_as(C.POINTER(C.c_longlong)), 64)
    if n < 0:
        raise PsbaError(n, "psba_chol_dist_exchange_plan failed")
    return [tuple(int(v) for v in row) for row in out[:n]]


SCAL_WORDS, SCAL_RAW = 104, 106  # the try's scalar block; with its stamp and check word (csrc/scal_publish.h)


def scal_block_check(block, stamp):
    """psba_scal_block_check (host only): the check word, as uint64, of a block of 104 words (float64 or uint64: bit
    patterns) under the stamp `stamp`."""
    b = np.ascontiguousarray(block).view(np.float64).reshape(SCAL_WORDS)
    out = np.zeros(1)
    rc = lib.psba_scal_block_check(_d(b), float(stamp), _d(out))
    if rc < 0:
        raise PsbaError(rc, "psba_scal_block_check failed")
    return out.view(np.uint64)[0]


def scal_block_take(raw, want_stamp):
    """psba_scal_block_take (host only): (accepted, block) for the 106 raw words `raw` (block, stamp, check; float64 or
    uint64), as psba_backsub_wait takes them from pinned memory; block: the 104 words of the private copy, uint64."""
    r = np.ascontiguousarray(raw).view(np.float64).reshape(SCAL_RAW)
    out = np.zeros(SCAL_WORDS)
    rc = lib.psba_scal_block_take(_d(r), float(want_stamp), _d(out))
    if rc < 0:
        raise PsbaError(rc, "psba_scal_block_take failed")
    return bool(rc), out.view(np.uint64)


def ring_plan(n_cams, n_pts, iidx, jidx):
    """The schedule of the S-assembly kernel's ring route for a sparsity pattern (host only, no
    device): dict of the arrays psba_ring_plan_copy documents, or None when the route does not
    apply to the problem.  Needs a library built with PSBA_BUILD_EXPERIMENTS=1."""
    if not HAS_EXPERIMENTS:
        raise PsbaError(-6, "the ring route is an experiment: build with PSBA_BUILD_EXPERIMENTS=1")
    iidx = _c(iidx, np.int32)
    jidx = _c(jidx, np.int32)
    p = lib.psba_ring_plan_create(int(n_cams), int(n_pts), int(iidx.size), _i(iidx), _i(jidx))
    if not p:
        raise PsbaError(-1, "psba_ring_plan_create failed")
    try:
        info = (C.c_longlong * 16)()
        lib.psba_ring_plan_info(p, info)
        (nR, nS, nwg, nsteps, nent, nops, njob, products, slots, lanes, pages, yslots, lat, nlb, nbl0, loaded) = (int(x) for x in info)
        if nwg == 0:
            return None
        wg = np.zeros((nwg, 13), dtype=np.int64)
        steps = np.zeros((nsteps, 4), dtype=np.int32)
        entries = np.zeros(nent, dtype=np.uint32)
        ops = np.zeros((nops, 2), dtype=np.int32)
        jobs = np.zeros((njob, 4), dtype=np.int32)
        lane_blk = np.zeros(nlb, dtype=np.int32)
        blk_lane0 = np.zeros(nbl0, dtype=np.int32)
        rb = np.zeros(nR + 1, dtype=np.int32)
        lib.psba_ring_plan_copy(p, wg.ctypes.data_as(C.POINTER(C.c_longlong)), _i(steps),
                                entries.ctypes.data_as(C.POINTER(C.c_uint)), _i(ops), _i(jobs), _i(lane_blk),
                                _i(blk_lane0), _i(rb))
    finally:
        lib.psba_ring_plan_destroy(p)
    return dict(nR=nR, nS=nS, wg=wg, steps=steps, entries=entries, ops=ops, jobs=jobs, lane_blk=lane_blk,
                blk_lane0=blk_lane0, rb=rb, products=products, lane_steps=slots, lanes=lanes, slots=pages,
                page=yslots, lat=lat, loaded_recs=loaded)


def shard_problem(prob, nranks, rank):
    """The sub-problem rank `rank` owns: a contiguous point range and its observations;
    cameras are replicated.  A problem with kc / cov keys (read_problem_ex) keeps kc and the cov rows of
    the observations it keeps; one with fixed_cams / fixed_pts keys (Psba.set_fixed) keeps fixed_cams and the
    fixed_pts entries of its points."""
    bounds = partition_points(prob["nP"], prob["iidx"], nranks)
    p0, p1 = int(bounds[rank]), int(bounds[rank + 1])
    iidx = np.asarray(prob["iidx"])
    sel = (iidx >= p0) & (iidx < p1)
    out = Problem(K=prob["K"], initrot=prob["initrot"], cams=prob["cams"], pts=prob["pts"][p0:p1],
                  impts=np.asarray(prob["impts"])[sel], iidx=(iidx[sel] - p0).astype(np.int32),
                  jidx=np.asarray(prob["jidx"])[sel].astype(np.int32), nC=prob["nC"], nP=p1 - p0,
                  nO=int(sel.sum()))
    if "kc" in prob:
        out["kc"] = prob["kc"]
    if "cov" in prob:
        out["cov"] = None if prob["cov"] is None else np.asarray(prob["cov"])[sel]
    if "fixed_cams" in prob:
        out["fixed_cams"] = prob["fixed_cams"]
    if "fixed_pts" in prob:
        out["fixed_pts"] = None if prob["fixed_pts"] is None else np.asarray(prob["fixed_pts"])[p0:p1]
    return out


class Psba:
    """One handle = one GPU.  Methods are the C entry points without the psba_ prefix."""

    def __init__(self, device=0):
        self._h = _h()
        rc = lib.psba_create(int(device), C.byref(self._h))
        if rc != 0:
            raise PsbaError(rc, lib.psba_last_error(None).decode())
        self.nC = self.nP = self.nO = 0

    def close(self):
        if self._h:
            lib.psba_destroy(self._h)
            self._h = _h()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise PsbaError(rc, lib.psba_last_error(self._h).decode())
        return rc

    # ---- setup ----
    def set_camera_model(self, model):
        """False / CAMERA_FIXED_K: blocks of 6; True / CAMERA_FREE_K: blocks of 11 (fu, u0, v0, ar, s | rotation |
        translation); CAMERA_FREE_KD: blocks of 16 (... s | k1..k5 | rotation | translation).  Before upload."""
        self._ck(lib.psba_set_camera_model(self._h, int(model)))

    def set_intrinsics_mask(self, free=None):
        """psba_set_intrinsics_mask: ten flags (fu, u0, v0, ar, s, k1..k5), non-zero = optimised; None = all free."""
        if free is None:
            return self._ck(lib.psba_set_intrinsics_mask(self._h, None))
        m = np.ascontiguousarray((np.asarray(free).reshape(-1) != 0).astype(np.uint8))
        if m.size != 10:
            raise PsbaError(-1, f"set_intrinsics_mask: {m.size} flags for 10 intrinsics")
        self._ck(lib.psba_set_intrinsics_mask(self._h, m.ctypes.data_as(C.POINTER(C.c_ubyte))))

    def intrinsics_mask(self):
        """psba_intrinsics_mask -> tuple of ten 0 / 1"""
        m = np.zeros(10, dtype=np.uint8)
        self._ck(lib.psba_intrinsics_mask(self._h, m.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return tuple(int(v) for v in m)

    def set_camera_masks(self, free=None):
        """psba_set_camera_masks: [nC, 10] flags, row j = camera j, order (fu, u0, v0, ar, s, k1..k5), non-zero =
        optimised (ANDed with the global mask); None, or a table without a zero, = no table.  CAMERA_FREE_KD only."""
        if free is None:
            return self._ck(lib.psba_set_camera_masks(self._h, None))
        m = np.ascontiguousarray((np.asarray(free).reshape(-1) != 0).astype(np.uint8))
        if self.nC and m.size != 10 * self.nC:  # (before an upload nC is 0: the library refuses, nothing is read)
            raise PsbaError(-1, f"set_camera_masks: {m.size} flags for {self.nC} cameras of 10 intrinsics")
        self._ck(lib.psba_set_camera_masks(self._h, m.ctypes.data_as(C.POINTER(C.c_ubyte))))

    def camera_masks(self):
        """psba_camera_masks -> [nC, 10] uint8, the table as set; all ones when there is none"""
        m = np.zeros((self.nC, 10), dtype=np.uint8)
        self._ck(lib.psba_camera_masks(self._h, m.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return m

    def set_intrinsics_groups(self, group_of_cam=None):
        """psba_set_intrinsics_groups: one label (any int) per camera, equal labels share their ten intrinsics;
        None = no sharing.  CAMERA_FREE_KD only; members must hold bit-identical intrinsics."""
        if group_of_cam is None:
            return self._ck(lib.psba_set_intrinsics_groups(self._h, None))
        g = np.ascontiguousarray(np.asarray(group_of_cam).reshape(-1), dtype=np.int32)
        if g.size != self.nC:
            raise PsbaError(-1, f"set_intrinsics_groups: {g.size} labels for {self.nC} cameras")
        self._ck(lib.psba_set_intrinsics_groups(self._h, g.ctypes.data_as(C.POINTER(C.c_int))))

    def set_sparse_intrinsics_groups(self, group_of_cam=None):
        """psba_set_sparse_intrinsics_groups: set_intrinsics_groups for a SOLVER_SPARSE handle on blocks of 16 -- the
        stored blocks stay unfolded and undamped, the solve folds.  None = no sharing."""
        if group_of_cam is None:
            return self._ck(lib.psba_set_sparse_intrinsics_groups(self._h, None))
        g = np.ascontiguousarray(np.asarray(group_of_cam).reshape(-1), dtype=np.int32)
        if g.size != self.nC:
            raise PsbaError(-1, f"set_sparse_intrinsics_groups: {g.size} labels for {self.nC} cameras")
        self._ck(lib.psba_set_sparse_intrinsics_groups(self._h, g.ctypes.data_as(C.POINTER(C.c_int))))

    def set_damping(self, kind=DAMPING_IDENTITY, dmin=0.0, dmax=0.0):
        """psba_set_damping: DAMPING_IDENTITY (N + mu I) or DAMPING_MARQUARDT (N + mu D, D = clamp(diag N, dmin, dmax));
        0 for a clamp = its default (1e-6, 1e32).  Free-intrinsics camera models only."""
        self._ck(lib.psba_set_damping(self._h, int(kind), float(dmin), float(dmax)))

    def damping(self):
        """psba_damping -> (kind, dmin, dmax)"""
        k, lo, hi = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        self._ck(lib.psba_damping(self._h, C.byref(k), C.byref(lo), C.byref(hi)))
        return k.value, lo.value, hi.value

    def get_damping_diag(self):
        """psba_get_damping_diag (test hook): D [nT] = [cnp per camera ; 3 per point] of the current linearization."""
        D = np.empty(getattr(self, "nT", 0) or 1)  # (before an upload the library refuses, nothing is written)
        self._ck(lib.psba_get_damping_diag(self._h, _d(D)))
        return D

    def intrinsics_groups(self):
        """psba_intrinsics_groups -> (representative of each camera [nC], number of groups)"""
        rep = np.zeros(self.nC, dtype=np.int32)
        n = C.c_int(0)
        self._ck(lib.psba_intrinsics_groups(self._h, rep.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n)))
        return rep, int(n.value)

    def set_distortion(self, kc):
        """psba_set_distortion: kc [nC, 5] = (k1, k2, k3, k4, k5) per camera, None = no distortion.  Under
        CAMERA_FREE_KD: the starting kc (columns 5..9 of the parameters), None = zeros."""
        k = None if kc is None else _c(kc).reshape(-1)
        if k is not None and k.size != 5 * self.nC:
            raise PsbaError(-1, f"set_distortion: {k.size} values for {self.nC} cameras (5 each)")
        self._ck(lib.psba_set_distortion(self._h, _d(k)))

    def set_obs_covariance(self, cov):
        """psba_set_obs_covariance: cov [nO, 2, 2] (or [nO, 4] row-major) in the uploaded observation order,
        None = none."""
        c = None if cov is None else _c(cov).reshape(-1)
        if c is not None and c.size != 4 * self.nO:
            raise PsbaError(-1, f"set_obs_covariance: {c.size} values for {self.nO} observations (4 each)")
        self._ck(lib.psba_set_obs_covariance(self._h, _d(c)))

    def lens_model(self):
        """psba_lens_model -> (has_distortion, has_covariance)"""
        d, c = C.c_int(), C.c_int()
        self._ck(lib.psba_lens_model(self._h, C.byref(d), C.byref(c)))
        return bool(d.value), bool(c.value)

    def set_robust_loss(self, kind, scale=1.0):
        """psba_set_robust_loss: kind LOSS_NONE / LOSS_HUBER / LOSS_CAUCHY / LOSS_SOFT_L1, scale c > 0 in whitened
        units (pixels when Sigma = I)."""
        self._ck(lib.psba_set_robust_loss(self._h, int(kind), float(scale)))

    def robust_loss(self):
        """psba_robust_loss -> (kind, scale)"""
        k, c = C.c_int(), C.c_double()
        self._ck(lib.psba_robust_loss(self._h, C.byref(k), C.byref(c)))
        return k.value, c.value

    def set_fixed(self, cams=None, pts=None):
        """psba_set_fixed: cams [nC], pts [nP] boolean or integer arrays, non-zero = the block is held constant;
        None = none of that kind, two Nones clear the mask."""
        def mask(a, n, what):
            if a is None:
                return None
            m = (np.asarray(a).reshape(-1) != 0).astype(np.uint8)
            if m.size != n:
                raise PsbaError(-1, f"set_fixed: {m.size} flags for {n} {what}")
            return np.ascontiguousarray(m)
        c, p = mask(cams, self.nC, "cameras"), mask(pts, self.nP, "points")
        ub = C.POINTER(C.c_ubyte)
        self._ck(lib.psba_set_fixed(self._h, None if c is None else c.ctypes.data_as(ub),
                                    None if p is None else p.ctypes.data_as(ub)))

    def fixed_counts(self):
        """psba_fixed_counts -> (fixed cameras, fixed points)"""
        c, p = C.c_int(), C.c_int()
        self._ck(lib.psba_fixed_counts(self._h, C.byref(c), C.byref(p)))
        return c.value, p.value

    def set_held(self, poses=None, pts=None):
        """psba_set_held (free-intrinsics models): poses [nC], pts [nP] boolean or integer arrays, non-zero = the
        camera's six pose coordinates / the point are held constant (the intrinsics stay under the mask and the
        groups); None = none of that kind, two Nones clear the masks."""
        def mask(a, n, what):
            if a is None:
                return None
            m = (np.asarray(a).reshape(-1) != 0).astype(np.uint8)
            if n and m.size != n:  # (before an upload n is 0: the library refuses, nothing is read)
                raise PsbaError(-1, f"set_held: {m.size} flags for {n} {what}")
            return np.ascontiguousarray(m)
        c, p = mask(poses, self.nC, "poses"), mask(pts, self.nP, "points")
        ub = C.POINTER(C.c_ubyte)
        self._ck(lib.psba_set_held(self._h, None if c is None else c.ctypes.data_as(ub),
                                   None if p is None else p.ctypes.data_as(ub)))

    def held_counts(self):
        """psba_held_counts -> (held poses, held points)"""
        c, p = C.c_int(), C.c_int()
        self._ck(lib.psba_held_counts(self._h, C.byref(c), C.byref(p)))
        return c.value, p.value

    def set_priors(self, cam_mean=None, cam_info=None, pt_mean=None, pt_info=None):
        """psba_set_priors (free-intrinsics models): Gaussian priors, cost += d^T info d with d = mean - parameters.
        cam_mean [nC, cnp], cam_info [nC, cnp, cnp]; pt_mean [nP, 3], pt_info [nP, 3, 3].  An info array of shape
        [n, k] is taken as diagonals (1 / sigma^2) and expanded here.  A block whose information is all zero has no
        prior; the mean and the information of a kind are both None or both given, four Nones clear the priors."""
        def kind(mean, info, n, k, what):
            if mean is None and info is None:
                return None, None
            if mean is None or info is None:   # (the library's refusal and its text)
                z = np.zeros(1)
                return (None, z) if mean is None else (z, None)
            m = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).reshape(-1))
            L = np.asarray(info, dtype=np.float64)
            if n and L.ndim == 2 and L.shape == (n, k):
                full = np.zeros((n, k, k))
                full[:, np.arange(k), np.arange(k)] = L
                L = full
            L = np.ascontiguousarray(L.reshape(-1))
            if n and (m.size != n * k or L.size != n * k * k):  # (before an upload n is 0: the library refuses)
                raise PsbaError(-1, f"set_priors: {m.size} means and {L.size} information entries for {n} {what} of {k}")
            return m, L
        cnp = self.camera_block()
        cm, ci = kind(cam_mean, cam_info, self.nC, cnp, "cameras")
        pm, pi = kind(pt_mean, pt_info, self.nP, 3, "points")
        ptr = lambda a: None if a is None else a.ctypes.data_as(_dp)  # noqa: E731
        self._ck(lib.psba_set_priors(self._h, ptr(cm), ptr(ci), ptr(pm), ptr(pi)))

    def prior_counts(self):
        """psba_prior_counts -> (cameras with a prior, points with a prior)"""
        c, p = C.c_int(), C.c_int()
        self._ck(lib.psba_prior_counts(self._h, C.byref(c), C.byref(p)))
        return c.value, p.value

    def prior_cost(self, which=PARAMS_CUR):
        """psba_prior_cost -> (camera priors' part, point priors' part) of the cost at PARAMS_CUR / PARAMS_NEW"""
        c, p = C.c_double(), C.c_double()
        self._ck(lib.psba_prior_cost(self._h, which, C.byref(c), C.byref(p)))
        return c.value, p.value

    def set_obs_weighting(self, kind, scale=1.0, sigma=None):
        """psba_set_obs_weighting (free-intrinsics models): a loss kind LOSS_NONE / LOSS_HUBER / LOSS_CAUCHY /
        LOSS_SOFT_L1 with scale c > 0, and sigma [nO] standard deviations per observation in the uploaded order (None:
        all 1).  (LOSS_NONE, any scale, None) clears the weighting."""
        s = None if sigma is None else np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(-1))
        if s is not None and self.nO and s.size != self.nO:  # (before an upload nO is 0: the library refuses)
            raise PsbaError(-1, f"set_obs_weighting: {s.size} sigmas for {self.nO} observations")
        self._ck(lib.psba_set_obs_weighting(self._h, int(kind), float(scale), None if s is None else _d(s)))

    def obs_weighting(self):
        """psba_obs_weighting -> (kind, scale, sigmas are set)"""
        k, c, s = C.c_int(), C.c_double(), C.c_int()
        self._ck(lib.psba_obs_weighting(self._h, C.byref(k), C.byref(c), C.byref(s)))
        return k.value, c.value, bool(s.value)

    def get_obs_weights(self, which=PARAMS_CUR):
        """psba_get_obs_weights -> (s [nO], w [nO]) at PARAMS_CUR / PARAMS_NEW: s_a = |e_a / sigma_a|^2 and
        w_a = omega_a / sigma_a, the factor the observation's blocks are multiplied by."""
        s, w = np.empty(self.nO), np.empty(self.nO)
        self._ck(lib.psba_get_obs_weights(self._h, which, _d(s), _d(w)))
        return s, w

    def obs_sq_residuals(self, which=PARAMS_CUR):
        """psba_obs_sq_residuals: s_a = ||L_a e_a||^2 per observation [nO] at PARAMS_CUR / PARAMS_NEW."""
        return self._out(lib.psba_obs_sq_residuals, self.nO, which)[1]

    def camera_block(self):
        n = C.c_int()
        self._ck(lib.psba_camera_block(self._h, C.byref(n)))
        return n.value

    def upload_problem(self, prob):
        self.nC, self.nP, self.nO = int(prob["nC"]), int(prob["nP"]), int(prob["nO"])
        self.cnp = self.camera_block()
        self.nA, self.nB = self.cnp * self.nC, 3 * self.nP
        self.nT = self.nA + self.nB
        a = [_c(prob[k]).reshape(-1) for k in ("K", "impts", "initrot", "cams", "pts")]
        ii, jj = _c(prob["iidx"], np.int32), _c(prob["jidx"], np.int32)
        self._ck(lib.psba_upload_problem(self._h, self.nC, self.nP, self.nO, _d(a[0]), _d(a[1]),
                                         _d(a[2]), _d(a[3]), _d(a[4]), _i(ii), _i(jj)))

    def set_params(self, cams, pts):
        c, p = _c(cams).reshape(-1), _c(pts).reshape(-1)
        self._ck(lib.psba_set_params(self._h, _d(c), _d(p)))

    def reset_params(self):
        self._ck(lib.psba_reset_params(self._h))

    def get_params(self, which=PARAMS_CUR):
        c, p = np.empty(self.nA), np.empty(self.nB)
        self._ck(lib.psba_get_params(self._h, which, _d(c), _d(p)))
        return c.reshape(self.nC, self.cnp), p.reshape(self.nP, 3)

    # ---- fused verbs ----
    def schur_path(self):
        """0: LDS-partition schedule, 1: owner route, 2: global-atomic assembly kernel, 3: ring route, 4: block-sparse,
        5: the free-intrinsics route (blocks of 11 and 16) (psba_schur_path)."""
        v = C.c_int()
        self._ck(lib.psba_schur_path(self._h, C.byref(v)))
        return v.value

    def lm_ran_lean(self):
        """True: the last levmar of this handle queued its look-ahead linearizations in the lean form (Jacobian factors
        to the Schur assembly, no W and no per-camera sums); False: in the standard form (psba_lm_ran_lean)."""
        v = C.c_int()
        self._ck(lib.psba_lm_ran_lean(self._h, C.byref(v)))
        return bool(v.value)

    def linearize_lean(self):
        """Test hook: the current parameters linearized once more in the lean form, behind linearize(); the next
        schur_assemble takes the lean route (psba_linearize_lean)."""
        self._ck(lib.psba_linearize_lean(self._h))

    def residual(self, which=PARAMS_CUR):
        v = C.c_double()
        self._ck(lib.psba_residual(self._h, which, C.byref(v)))
        return v.value

    def linearize(self, coeff=1.0, coeff_g=1.0):
        self._ck(lib.psba_linearize(self._h, coeff, coeff_g))

    def begin(self, coeff=1.0, coeff_g=1.0):
        """(cost, max diagonal) at the current parameters + their linearization, one sync."""
        c, m = C.c_double(), C.c_double()
        self._ck(lib.psba_begin(self._h, coeff, coeff_g, C.byref(c), C.byref(m)))
        return c.value, m.value

    def max_diag(self):
        v = C.c_double()
        self._ck(lib.psba_max_diag(self._h, C.byref(v)))
        return v.value

    def schur_assemble(self, mu):
        self._ck(lib.psba_schur_assemble(self._h, mu))

    def schur_reduce(self):
        self._ck(lib.psba_schur_reduce(self._h))

    def schur_solve(self):
        """PSBA_OK, or PSBA_PCG_MAXIT (4) when the iterative solve used up max_iter (the iterate is kept)."""
        return self._ck(lib.psba_schur_solve(self._h))

    def backsub(self, mu):
        s = TryScalars()
        self._ck(lib.psba_backsub(self._h, mu, C.byref(s)))
        return s

    def backsub_async(self, mu):
        self._ck(lib.psba_backsub_async(self._h, mu))

    def linearize_ahead(self):
        self._ck(lib.psba_linearize_ahead(self._h))

    def backsub_wait(self):
        s = TryScalars()
        self._ck(lib.psba_backsub_wait(self._h, C.byref(s)))
        return s

    def accept(self):
        self._ck(lib.psba_accept(self._h))

    def publish_stats(self):
        """(takes, torn) since the handle was created: scalar blocks backsub_wait accepted from a linearization queued
        ahead, and tries among them that met a torn reading first (psba_publish_stats)."""
        a, b = C.c_longlong(), C.c_longlong()
        self._ck(lib.psba_publish_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def test_publish(self, block=None, threads=128):
        """Test hook: the publishing prologue alone in one workgroup of `threads`; the 106 raw pinned words (block,
        stamp, check) as uint64.  block: 104 words (float64 or uint64) that stand in the device scalar block for the
        launch; None: the device's block as it is (psba_test_publish)."""
        b = None if block is None else np.ascontiguousarray(block).view(np.float64).reshape(SCAL_WORDS)
        raw = np.zeros(SCAL_RAW)
        self._ck(lib.psba_test_publish(self._h, _d(b), int(threads), _d(raw)))
        return raw.view(np.uint64)

    # ---- sba_func.h mirror ----
    def _out(self, fn, n, *pre):
        out = np.empty(n)
        rc = self._ck(fn(self._h, *pre, _d(out)))
        return rc, out

    def compute_exQT(self, which=PARAMS_CUR):
        return self._out(lib.psba_compute_exQT, 2 * self.nO, which)[1]

    def compute_jacobiQT(self):
        JA, JB = np.empty(12 * self.nO), np.empty(6 * self.nO)
        self._ck(lib.psba_compute_jacobiQT(self._h, _d(JA), _d(JB)))
        return JA, JB

    def compute_U(self, coeff=1.0):
        return self._out(lib.psba_compute_U, 36 * self.nC, coeff)[1]

    def compute_V(self, coeff=1.0):
        return self._out(lib.psba_compute_V, 9 * self.nP, coeff)[1]

    def maxElmOfUV(self):
        v = C.c_double()
        self._ck(lib.psba_maxElmOfUV(self._h, C.byref(v)))
        return v.value

    def update_UV(self, mu):
        U, V = np.empty(36 * self.nC), np.empty(9 * self.nP)
        self._ck(lib.psba_update_UV(self._h, mu, _d(U), _d(V)))
        return U, V

    def restore_UVdiag(self):
        self._ck(lib.psba_restore_UVdiag(self._h))

    def compute_Vinv(self):
        return self._out(lib.psba_compute_Vinv, 9 * self.nP)

    def compute_Wblks(self, coeff=1.0):
        return self._out(lib.psba_compute_Wblks, 18 * self.nO, coeff)[1]

    def compute_Yblks(self):
        return self._out(lib.psba_compute_Yblks, 18 * self.nO)[1]

    def compute_S(self):
        return self._out(lib.psba_compute_S, self.nA * self.nA)[1].reshape(self.nA, self.nA)

    def compute_g(self, coeff=1.0):
        return self._out(lib.psba_compute_g, self.nT, coeff)[1]

    def compute_ea(self):
        return self._out(lib.psba_compute_ea, self.nA)[1]

    def SPDinv_matVec(self):
        return self._out(lib.psba_SPDinv_matVec, self.nA)

    def compute_eb(self):
        return self._out(lib.psba_compute_eb, self.nB)[1]

    def compute_dpb(self):
        return self._out(lib.psba_compute_dpb, self.nT)[1]

    def compute_newp(self):
        return self._out(lib.psba_compute_newp, self.nT)[1]

    def update_p(self):
        return self._out(lib.psba_update_p, self.nT)[1]

    # ---- LM ----
    def levmar(self, max_iter=50, tr_handoff=False, verbose=False, log_cap=512, start_itno=0, init_mu=0.0,
               stop_cost=0.0):
        """stop_cost: end once the cost is at or below it; 0 = the default 1e-12, negative = no absolute stop."""
        opts = LmOptions(max_iter, int(tr_handoff), int(verbose), log_cap, start_itno, init_mu, stop_cost)
        res = LmResult()
        log = np.zeros((max(log_cap, 1), 5))
        self._ck(lib.psba_levmar(self._h, C.byref(opts), C.byref(res), _d(log)))
        return res, log[: res.n_log].copy()

    # ---- block-sparse S + PCG ----
    def set_solver(self, solver, tol=0.0, max_iter=0):
        """solver: 0 dense Cholesky, 1 block-sparse S + preconditioned CG (six-parameter blocks), SOLVER_SPARSE = 2 the
        block-sparse mode of whatever camera block the handle has (before upload_problem)."""
        self._ck(lib.psba_set_solver(self._h, int(solver), float(tol), int(max_iter)))

    def pcg_info(self):
        it, rr, nb, nd = C.c_int(), C.c_double(), C.c_longlong(), C.c_longlong()
        self._ck(lib.psba_pcg_info(self._h, C.byref(it), C.byref(rr), C.byref(nb), C.byref(nd)))
        return it.value, rr.value, nb.value, nd.value

    def get_sparse_S(self):
        nb = self.pcg_info()[2]
        jk = np.empty((nb, 2), dtype=np.int32)
        cnp = self.camera_block()
        val = np.empty((nb, cnp, cnp))
        ea = np.empty(cnp * self.nC)
        self._ck(lib.psba_get_sparse_S(self._h, _i(jk), _d(val), _d(ea)))
        return jk, val, ea

    def set_sparse_S(self, val, ea):
        val = np.ascontiguousarray(val, dtype=np.float64)
        ea = np.ascontiguousarray(ea, dtype=np.float64)
        self._ck(lib.psba_set_sparse_S(self._h, _d(val), _d(ea)))

    def sparse_S_times(self, x):
        """psba_sparse_S_times: y = S x [nA] on the stored blocks, by the solve's own product kernel."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        n = self.camera_block() * self.nC
        if x.size != n:
            raise PsbaError(-1, f"sparse_S_times: {x.size} entries for {n} unknowns")
        y = np.empty(n)
        self._ck(lib.psba_sparse_S_times(self._h, _d(x), _d(y)))
        return y

    def get_sparse_precond(self):
        """psba_get_sparse_precond (test hook): [nC, cnp, cnp], the inverses of the diagonal blocks the last schur_solve
        under SOLVER_SPARSE on blocks of 11 / 16 preconditioned with."""
        cnp = self.camera_block()
        M = np.empty((getattr(self, "nC", 0) or 1, cnp, cnp))  # (before an upload the library refuses, nothing is written)
        self._ck(lib.psba_get_sparse_precond(self._h, _d(M)))
        return M

    def sparse_S_times_many(self, X):
        """psba_sparse_S_times_many: Y = S X for panels X [n_panels, nA, 16], by the product kernel of
        sparse_camera_covariance."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        n = self._sizes()[1]
        if X.ndim != 3 or X.shape[1:] != (n, 16):
            raise PsbaError(-1, f"sparse_S_times_many: X is {X.shape}, not [panels, {n}, 16]")
        Y = np.empty_like(X)
        self._ck(lib.psba_sparse_S_times_many(self._h, X.shape[0], _d(X), _d(Y)))
        return Y

    def sparse_camera_covariance(self, sel, mu=0.0, scale=1.0, reassemble=True, want_cols=False):
        """psba_sparse_camera_covariance: (C, info) -- C [n cnp, n cnp] = scale (S(mu)^-1)[sel, sel], the joint covariance
        of the chosen cameras under SOLVER_SPARSE on blocks of 11 / 16; info = dict(status (PSBA_OK, PSBA_NOT_SPD or
        PSBA_PCG_MAXIT), iters [n cnp], relres [n cnp] and, with want_cols, cols [n cnp, nA]: the solved columns, not
        scaled).  Raises on errors."""
        sel = np.ascontiguousarray(np.asarray(sel).reshape(-1), dtype=np.int32)
        cnp, nA, _ = self._sizes()
        m = max(cnp * sel.size, 1)
        Cm = np.zeros((m, m))
        iters = np.zeros(m, dtype=np.int32)
        relres = np.zeros(m)
        cols = np.zeros((m, nA)) if want_cols else None
        rc = self._ck(lib.psba_sparse_camera_covariance(self._h, float(mu), float(scale), int(bool(reassemble)), int(sel.size),
                                                        _i(sel), _d(Cm), _d(cols), _i(iters), _d(relres)))
        info = dict(status=rc, iters=iters, relres=relres)
        if want_cols:
            info["cols"] = cols
        return Cm, info

    def sparse_point_covariance(self, sel, mu=0.0, scale=1.0, reassemble=True, want_cols=False):
        """psba_sparse_point_covariance: (C, info) -- C [3 n, 3 n], the joint covariance of the chosen points under
        SOLVER_SPARSE on blocks of 11 / 16: block (a, b) = scale (delta_ab V*_a^-1 + Y_a^T S(mu)^-1 Y_b); info =
        dict(status (PSBA_OK, PSBA_NOT_SPD, PSBA_SINGULAR_V or PSBA_PCG_MAXIT), iters [3 n], relres [3 n] and, with
        want_cols, cols [3 n, nA]: the solved columns S(mu)^-1 Y_b, not scaled).  Raises on errors."""
        sel = np.ascontiguousarray(np.asarray(sel).reshape(-1), dtype=np.int32)
        nA = self._sizes()[1]
        m = max(3 * sel.size, 1)
        Cm = np.zeros((m, m))
        iters = np.zeros(m, dtype=np.int32)
        relres = np.zeros(m)
        cols = np.zeros((m, nA)) if want_cols else None
        rc = self._ck(lib.psba_sparse_point_covariance(self._h, float(mu), float(scale), int(bool(reassemble)), int(sel.size),
                                                       _i(sel), _d(Cm), _d(cols), _i(iters), _d(relres)))
        info = dict(status=rc, iters=iters, relres=relres)
        if want_cols:
            info["cols"] = cols
        return Cm, info

    def set_sparse_pattern(self, flags):
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        self._ck(lib.psba_set_sparse_pattern(self._h, flags.ctypes.data_as(C.POINTER(C.c_ubyte)), flags.size))

    # ---- the sharded dense factorization, piece by piece ----
    def chol_dist_shape(self):
        n32, nb, sh = C.c_int(), C.c_int(), C.c_int()
        self._ck(lib.psba_chol_dist_shape(self._h, C.byref(n32), C.byref(nb), C.byref(sh)))
        return n32.value, nb.value, bool(sh.value)

    def chol_shape(self):
        """psba_chol_shape: the dense chain's route as a dict (n32, fused, fused2, blocked, NB, diag_only, lookahead,
        single)"""
        out = (C.c_int * 8)()
        self._ck(lib.psba_chol_shape(self._h, out))
        keys = ("n32", "fused", "fused2", "blocked", "NB", "diag_only", "lookahead", "single")
        return {k: (int(v) if k in ("n32", "NB") else bool(v)) for k, v in zip(keys, out)}

    def chol_dist_begin(self):
        self._ck(lib.psba_chol_dist_begin(self._h))

    def chol_dist_superpanel(self, J):
        self._ck(lib.psba_chol_dist_superpanel(self._h, int(J)))

    def chol_dist_get_block(self, B):
        n = C.c_longlong()
        self._ck(lib.psba_chol_dist_block(self._h, int(B), 0, None, C.byref(n)))
        buf = np.empty(n.value)
        self._ck(lib.psba_chol_dist_block(self._h, int(B), 0, _d(buf), C.byref(n)))
        return buf

    def chol_dist_set_block(self, B, buf):
        n = C.c_longlong()
        self._ck(lib.psba_chol_dist_block(self._h, int(B), 1, _d(_c(buf)), C.byref(n)))

    def chol_dist_finish(self):
        self._ck(lib.psba_chol_dist_finish(self._h))

    # ---- trust region ----
    def compute_Jmultiply(self, x):
        return self._out(lambda h, out: lib.psba_compute_Jmultiply(h, _d(_c(x)), out), 2 * self.nO)[1]

    def jmul_dots(self, x1, x2=None):
        out = np.empty(3)
        a1 = _c(x1)
        a2 = None if x2 is None else _c(x2)
        self._ck(lib.psba_jmul_dots(self._h, _d(a1), _d(a2), _d(out)))
        return out

    def get_gradient(self):
        return self._out(lib.psba_get_gradient, self.nT)[1]

    def get_dp(self):
        return self._out(lib.psba_get_dp, self.nT)[1]

    def set_step(self, dp):
        self._ck(lib.psba_set_step(self._h, _d(_c(dp))))

    def cholmod_lambda(self, reassemble=True):
        lam, info = C.c_double(), np.empty(3)
        self._ck(lib.psba_cholmod_lambda(self._h, int(reassemble), C.byref(lam), _d(info)))
        return lam.value, info

    def cholmod_factor(self):
        """psba_get_cholmod_factor (test hook): L [nA, nA] of the last dense-mode cholmod_lambda."""
        return self._out(lib.psba_get_cholmod_factor, self.nA * self.nA)[1].reshape(self.nA, self.nA)

    def free_obs_blocks(self):
        """psba_get_free_obs_blocks (test hook): W [nO, cnp, 3], B [nO, 2, 3], e [nO, 2] of the last psba_linearize
        with free intrinsics."""
        W, Be = np.empty(3 * self.cnp * self.nO), np.empty(8 * self.nO)
        self._ck(lib.psba_get_free_obs_blocks(self._h, _d(W), _d(Be)))
        Be = Be.reshape(self.nO, 8)
        return W.reshape(self.nO, self.cnp, 3), Be[:, :6].reshape(self.nO, 2, 3).copy(), Be[:, 6:].copy()

    # ---- covariance of the estimate (fixed-K dense route) ----
    def covariance(self, mu=0.0, scale=1.0, reassemble=True):
        """psba_covariance_compute: C = scale (J^T J + mu I)^-1 on the free blocks at the current parameters (mu = 0, the
        true covariance, needs the gauge fixed by set_fixed).  scale="reduced_chi2": residual(PARAMS_CUR) /
        (2 nO - number of free parameters).  Returns PSBA_OK, PSBA_NOT_SPD or PSBA_SINGULAR_V (the getters refuse
        then); raises on errors."""
        if isinstance(scale, str):
            if scale != "reduced_chi2":
                raise PsbaError(-1, f"covariance: unknown scale {scale!r}")
            fc, fp = self.fixed_counts()
            dof = 2 * self.nO - (self.nT - self.cnp * fc - 3 * fp)
            if dof <= 0:
                raise PsbaError(-1, f"covariance: reduced_chi2 needs more residuals than free parameters (dof = {dof})")
            scale = self.residual(PARAMS_CUR) / dof
        return self._ck(lib.psba_covariance_compute(self._h, float(mu), float(scale), int(bool(reassemble))))

    def camera_covariance(self, pairs=None):
        """psba_get_camera_covariance: [n, 6, 6] blocks C_jk of the pairs [(j, k), ...]; None: the nC diagonal blocks."""
        return self._camera_blocks(lib.psba_get_camera_covariance, 6, pairs)

    def _camera_blocks(self, getter, cnp, pairs):
        """the pair marshalling of both camera-covariance getters: [n, cnp, cnp]"""
        if pairs is None:
            out = np.empty((max(self.nC, 1), cnp, cnp))
            self._ck(getter(self._h, self.nC, None, _d(out)))
            return out[:self.nC]
        p = _c(pairs, np.int32).reshape(-1, 2)
        out = np.empty((p.shape[0], cnp, cnp))
        self._ck(getter(self._h, p.shape[0], _i(p), _d(out)))
        return out

    def covariance_matrix(self):
        """psba_get_covariance_matrix: C_aa [nA, nA], symmetric, zero rows and columns for fixed cameras."""
        return self._out(lib.psba_get_covariance_matrix, self.nA * self.nA)[1].reshape(self.nA, self.nA)

    def point_covariance(self):
        """psba_get_point_covariance: C_bb,i [nP, 3, 3] (not after covariance(reassemble=False))."""
        return self._out(lib.psba_get_point_covariance, 9 * self.nP)[1].reshape(self.nP, 3, 3)

    def covariance_times(self):
        """psba_covariance_times: HIP-event ms (factor, inverse, points) of the last covariance()."""
        return self._out(lib.psba_covariance_times, 3)[1]

    # ---- covariance of the estimate with free intrinsics (blocks of 11 and 16) ----
    def _sizes(self):
        """(cnp, nA, nT) of the uploaded problem; (6, 1, 1) before an upload (the library refuses, nothing is written)"""
        cnp = getattr(self, "cnp", 6)
        return cnp, max(cnp * self.nC, 1), max(cnp * self.nC + 3 * self.nP, 1)

    def free_covariance(self, mu=0.0, scale=1.0, reassemble=True):
        """psba_free_covariance_compute: C_aa = scale E S(mu)^-1 E^T on the live coordinates and the point blocks, at the
        current parameters (mu = 0, the covariance, needs a gauge: held poses or priors).  scale is a number.  Returns
        PSBA_OK, PSBA_NOT_SPD or PSBA_SINGULAR_V (the getters refuse then); raises on errors."""
        return self._ck(lib.psba_free_covariance_compute(self._h, float(mu), float(scale), int(bool(reassemble))))

    def free_camera_covariance(self, pairs=None):
        """psba_get_free_camera_covariance: [n, cnp, cnp] blocks C_jk of the pairs [(j, k), ...]; None: the nC diagonal
        blocks."""
        return self._camera_blocks(lib.psba_get_free_camera_covariance, self._sizes()[0], pairs)

    def free_covariance_matrix(self):
        """psba_get_free_covariance_matrix: C_aa [nA, nA], symmetric; zero rows and columns for masked and held
        coordinates, a folded-away coordinate's equal to its representative's."""
        nA = self._sizes()[1]
        return self._out(lib.psba_get_free_covariance_matrix, nA * nA)[1].reshape(nA, nA)

    def free_point_covariance(self):
        """psba_get_free_point_covariance: C_bb,i [nP, 3, 3] (not after free_covariance(reassemble=False))."""
        return self._out(lib.psba_get_free_point_covariance, max(9 * self.nP, 1))[1][:9 * self.nP].reshape(self.nP, 3, 3)

    def free_sigmas(self):
        """psba_get_free_sigmas: [nT] standard deviations = sqrt of the diagonals of C_aa and of the C_bb,i."""
        return self._out(lib.psba_get_free_sigmas, self._sizes()[2])[1]

    def free_point_blocks(self):
        """psba_get_free_point_blocks (test hook): V [nP, 3, 3] undamped, Y [nO, cnp, 3] of the last assemble."""
        cnp = self._sizes()[0]
        V, Y = np.empty(max(9 * self.nP, 1)), np.empty(max(3 * cnp * self.nO, 1))
        self._ck(lib.psba_get_free_point_blocks(self._h, _d(V), _d(Y)))
        return V[:9 * self.nP].reshape(self.nP, 3, 3), Y[:3 * cnp * self.nO].reshape(self.nO, cnp, 3)

    def free_covariance_times(self):
        """psba_free_covariance_times: HIP-event ms (factor, inverse, points) of the last free_covariance()."""
        return self._out(lib.psba_free_covariance_times, 3)[1]

    def trust_region(self, max_iter=50, start_itno=0, verbose=False, log_cap=512, init_lambda=0.0):
        opts = TrOptions(max_iter, start_itno, int(verbose), log_cap, init_lambda)
        res = TrResult()
        log = np.zeros((max(log_cap, 1), 6))
        self._ck(lib.psba_trust_region(self._h, C.byref(opts), C.byref(res), _d(log)))
        return res, log[: res.n_log].copy()

    def solve(self, max_iter=50, verbose=False):
        res = SolveResult()
        self._ck(lib.psba_solve(self._h, max_iter, int(verbose), C.byref(res)))
        return res

    # ---- multi-GPU ----
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        rc = lib.psba_comm_unique_id(buf)
        if rc != 0:
            raise PsbaError(rc, "psba_comm_unique_id failed")
        return buf.raw

    def comm_init(self, nranks, rank, uid):
        buf = C.create_string_buffer(uid, 128)
        self._ck(lib.psba_comm_init(self._h, nranks, rank, buf))

    def set_rank_layout(self, nranks, rank):
        self._ck(lib.psba_set_rank_layout(self._h, nranks, rank))

    def reduce_buffer_size(self):
        n = C.c_longlong()
        self._ck(lib.psba_reduce_buffer_size(self._h, C.byref(n)))
        return n.value

    def get_reduce_buffer(self):
        out = np.empty(self.reduce_buffer_size())
        self._ck(lib.psba_get_reduce_buffer(self._h, _d(out)))
        return out

    def set_reduce_buffer(self, buf):
        b = _c(buf).reshape(-1)
        assert b.size == self.reduce_buffer_size()
        self._ck(lib.psba_set_reduce_buffer(self._h, _d(b)))

    # ---- measurement ----
    def profile_enable(self, on=True):
        """True: every kernel class; False: off; int > 0: bit mask of 1 << K_*."""
        self._ck(lib.psba_profile_enable(self._h, -1 if on is True else int(on)))

    def profile_reset(self):
        self._ck(lib.psba_profile_reset(self._h))

    def profile_get(self, kernel):
        ms, n = C.c_double(), C.c_int()
        self._ck(lib.psba_profile_get(self._h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def algorithmic_bytes(self, kernel):
        b = C.c_double()
        self._ck(lib.psba_algorithmic_bytes(self._h, kernel, C.byref(b)))
        return b.value
