// covariance.cpp -- the covariance verbs of include/psba_hip.h (kernels_cov.hip): psba_covariance_compute
// and its getters for six-parameter camera blocks, psba_free_covariance_compute and its getters for blocks of 11 and 16.
// The two families are one body each behind a guard on the camera block: a handle has one camera model for its life, so
// one result (cov_A, cov_pts) and one pair of flags (cov_ok, cov_pts_ok) serve both, and each family refuses the other's
// handle with PSBA_E_STATE by cnp.  Messages open with the exported verb's name, which the wrappers pass down.
#include <cmath>
#include <string>
#include <vector>

#include "api_common.h"
#include "camera_model.h"

using namespace psba;

namespace {

struct CovEvents {  // the four stamps of one compute: before the factor, before the inverse, before the points, the end
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  ~CovEvents() {
    for (hipEvent_t v : e)
      if (v) (void)hipEventDestroy(v);
  }
};

enum Family { SIX, FREE };
const char *const COMPUTE_VERB[2] = {"psba_covariance_compute", "psba_free_covariance_compute"};

#define NEED_V(h, verb, cond, what)                                         \
  do {                                                                      \
    if (!(cond)) return fail((h), PSBA_E_STATE, "%s: %s", verb, what);      \
  } while (0)

// behind both compute verbs, which have checked the upload, the try in flight and the camera block
int covariance_compute(psba_ctx *h, const char *verb, double mu, double scale, int reassemble) {
  NEED_V(h, verb, !FREE_SPARSE(h), "the dense solver only: PSBA_SOLVER_SPARSE assembles no dense S to invert");
  NEED_V(h, verb, h->solver != PSBA_SOLVER_PCG, "the dense solver only: PSBA_SOLVER_PCG assembles no dense S to invert");
  NEED_V(h, verb, !h->comm && h->nranks == 1, "single rank only: not under a rank layout or a communicator");
  if (!(std::isfinite(mu) && mu >= 0.0)) return fail(h, PSBA_E_INVALID, "%s: mu must be finite and >= 0 (got %.17g)", verb, mu);
  if (!(std::isfinite(scale) && scale > 0.0))
    return fail(h, PSBA_E_INVALID, "%s: scale must be finite and > 0 (got %.17g)", verb, scale);
  if (!reassemble) {
    NEED_V(h, verb, h->assembled, "reassemble = 0 inverts what the reduce buffer holds (psba_schur_assemble first)");
    NEED_V(h, verb, !h->try_shortcut, "every camera is fixed: this try assembled no S to invert");
  }
  h->cov_ok = h->cov_pts_ok = false;
  if (reassemble) {
    if (!(h->linearized && h->coeff == 1.0 && h->coeff_g == 1.0)) TRY(psba_linearize(h, 1.0, 1.0));
    TRY(psba_schur_assemble(h, mu));
    TRY(psba_schur_reduce(h));
  }
  CovEvents ev;
  for (hipEvent_t &e : ev.e) PSBA_HIP(h, hipEventCreate(&e));
  if (!h->cov_status) TRY(h->cov_status.alloc(h, 2));
  PSBA_HIP(h, hipMemsetAsync(h->cov_status, 0, 2 * sizeof(int), h->stream));
  TRY(launch_cov_cameras(h, scale, ev.e));
  if (reassemble) TRY(launch_cov_points(h, mu, scale));
  PSBA_HIP(h, hipEventRecord(ev.e[3], h->stream));
  int st[2] = {0, 0};
  TRY(d2h(h, st, h->cov_status, sizeof st));
  for (int k = 0; k < 3; k++) {
    float ms = 0.f;
    PSBA_HIP(h, hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
    h->cov_ms[k] = ms;
  }
  if (st[0] || st[1]) {
    h->err = std::string(verb) + (st[0] ? ": S is not positive definite on its free coordinates (a pivot of its Cholesky factor is not positive and finite)"
                                        : ": some V_i + mu D_i is singular (D = I unless psba_set_damping chose Marquardt's rule)");
    return (st[0] ? PSBA_NOT_SPD : 0) | (st[1] ? PSBA_SINGULAR_V : 0);
  }
  h->cov_ok = true;
  h->cov_pts_ok = reassemble != 0;
  return PSBA_OK;
}

// what every getter opens with: a result of this family's compute verb exists (points: and its point part)
int need_cov(psba_ctx *h, const char *verb, Family f, bool points = false) {
  NEED_V(h, verb, h->uploaded, "no problem uploaded");
  NEED_V(h, verb, (h->cnp == 6) == (f == SIX),
         f == SIX ? "six-parameter camera blocks only (free intrinsics: the psba_get_free_* getters)"
                  : "free-intrinsics camera blocks only (six-parameter blocks: psba_get_camera_covariance and its kin)");
  NEED_V(h, verb, !FREE_SPARSE(h), "the dense solver only: PSBA_SOLVER_SPARSE assembles no dense S to invert");
  if (!h->cov_ok)
    return fail(h, PSBA_E_STATE, "%s: %s first (whatever moves the parameters or the model invalidates the covariance)", verb, COMPUTE_VERB[f]);
  if (points && !h->cov_pts_ok)
    return fail(h, PSBA_E_STATE, "%s: only the camera part exists after %s with reassemble = 0", verb, COMPUTE_VERB[f]);
  return PSBA_OK;
}

// the blocks C_jk [cnp][cnp] of a pair list (null: the nC diagonal blocks): validate, stage, gather, copy out
int camera_blocks(psba_ctx *h, const char *verb, Family f, int n_pairs, const int *pairs, double *out) {
  TRY(need_cov(h, verb, f));
  const int nC = h->d.nC;
  const size_t blk = (size_t)h->cnp * h->cnp;
  if (!out) return fail(h, PSBA_E_INVALID, "%s: null output", verb);
  if (n_pairs < 0 || (!pairs && n_pairs != nC))
    return fail(h, PSBA_E_INVALID, "%s: n_pairs = %d (without a pair list it must be the number of cameras, %d)", verb, n_pairs, nC);
  std::vector<int2> jk((size_t)n_pairs);
  for (int q = 0; q < n_pairs; q++) {
    jk[q] = pairs ? make_int2(pairs[2 * q], pairs[2 * q + 1]) : make_int2(q, q);
    if (jk[q].x < 0 || jk[q].x >= nC || jk[q].y < 0 || jk[q].y >= nC)
      return fail(h, PSBA_E_INVALID, "%s: pair %d = (%d, %d) names a camera out of range (%d cameras)", verb, q, jk[q].x, jk[q].y, nC);
  }
  if (n_pairs == 0) return PSBA_OK;
  DevBuf<int2> jk_dev;
  DevBuf<double> out_dev;
  TRY(jk_dev.alloc(h, jk.size()));
  TRY(out_dev.alloc(h, blk * jk.size()));
  PSBA_HIP(h, hipMemcpyAsync(jk_dev, jk.data(), sizeof(int2) * jk.size(), hipMemcpyHostToDevice, h->stream));
  int rc = launch_cov_gather(h, jk_dev, n_pairs, out_dev);
  if (rc == PSBA_OK) rc = d2h(h, out, out_dev, sizeof(double) * blk * jk.size());
  (void)hipStreamSynchronize(h->stream);  // (before the two buffers go)
  return rc;
}

int covariance_matrix(psba_ctx *h, const char *verb, Family f, double *Caa) {
  TRY(need_cov(h, verb, f));
  if (!Caa) return fail(h, PSBA_E_INVALID, "%s: null output", verb);
  PSBA_HIP(h, hipMemcpy2DAsync(Caa, sizeof(double) * h->d.nA, h->cov_A, sizeof(double) * h->n32, sizeof(double) * h->d.nA,
                               h->d.nA, hipMemcpyDeviceToHost, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  return PSBA_OK;
}

int point_covariance(psba_ctx *h, const char *verb, Family f, double *out) {
  TRY(need_cov(h, verb, f, true));
  if (!out) return fail(h, PSBA_E_INVALID, "%s: null output", verb);
  return d2h(h, out, h->cov_pts, sizeof(double) * 9 * (size_t)h->d.nP);
}

int covariance_times(psba_ctx *h, const char *verb, Family f, double ms3[3]) {
  TRY(need_cov(h, verb, f));
  if (!ms3) return fail(h, PSBA_E_INVALID, "%s: null output", verb);
  for (int k = 0; k < 3; k++) ms3[k] = h->cov_ms[k];
  return PSBA_OK;
}

}  // namespace

// ---- six-parameter camera blocks ----

int psba_covariance_compute(psba_handle h, double mu, double scale, int reassemble) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  NEED(h, !h->backsub_pending, "a damping try is in flight (psba_backsub_wait first)");
  if (h->cnp != 6)
    return fail(h, PSBA_E_STATE, "%s: six-parameter camera blocks only (not %s)", __func__,
                h->cnp == KD_CNP ? "PSBA_CAMERA_FREE_KD" : "PSBA_CAMERA_FREE_K");
  return covariance_compute(h, __func__, mu, scale, reassemble);
}

int psba_get_camera_covariance(psba_handle h, int n_pairs, const int *pairs, double *out) {
  CHECK_H(h);
  return camera_blocks(h, __func__, SIX, n_pairs, pairs, out);
}

int psba_get_covariance_matrix(psba_handle h, double *Caa) {
  CHECK_H(h);
  return covariance_matrix(h, __func__, SIX, Caa);
}

int psba_get_point_covariance(psba_handle h, double *out) {
  CHECK_H(h);
  return point_covariance(h, __func__, SIX, out);
}

int psba_covariance_times(psba_handle h, double ms3[3]) {
  CHECK_H(h);
  return covariance_times(h, __func__, SIX, ms3);
}

// ---- free intrinsics, blocks of 11 and 16 ----

int psba_free_covariance_compute(psba_handle h, double mu, double scale, int reassemble) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  NEED(h, !h->backsub_pending, "a damping try is in flight (psba_backsub_wait first)");
  NEED(h, h->cnp != 6, "free-intrinsics camera blocks only (PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD); six-parameter blocks: psba_covariance_compute");
  return covariance_compute(h, __func__, mu, scale, reassemble);
}

int psba_get_free_camera_covariance(psba_handle h, int n_pairs, const int *pairs, double *out) {
  CHECK_H(h);
  return camera_blocks(h, __func__, FREE, n_pairs, pairs, out);
}

int psba_get_free_covariance_matrix(psba_handle h, double *Caa) {
  CHECK_H(h);
  return covariance_matrix(h, __func__, FREE, Caa);
}

int psba_get_free_point_covariance(psba_handle h, double *out) {
  CHECK_H(h);
  return point_covariance(h, __func__, FREE, out);
}

int psba_free_covariance_times(psba_handle h, double ms3[3]) {
  CHECK_H(h);
  return covariance_times(h, __func__, FREE, ms3);
}

int psba_get_free_sigmas(psba_handle h, double *sigma) {
  CHECK_H(h);
  TRY(need_cov(h, __func__, FREE, true));
  if (!sigma) return fail(h, PSBA_E_INVALID, "%s: null output", __func__);
  DevBuf<double> sig_dev;
  TRY(sig_dev.alloc(h, (size_t)h->d.nT));
  int rc = launch_fcov_sigmas(h, sig_dev);
  if (rc == PSBA_OK) rc = d2h(h, sigma, sig_dev, sizeof(double) * (size_t)h->d.nT);
  (void)hipStreamSynchronize(h->stream);  // (before the buffer goes)
  return rc;
}

// ---- chosen cameras under PSBA_SOLVER_SPARSE (kernels_free_pcg_many.hip) ----

// what both verbs of the sparse route open with: an uploaded problem, no try in flight, a FREE_SPARSE handle
static int need_free_sparse(psba_ctx *h, const char *verb) {
  NEED_V(h, verb, h->uploaded, "no problem uploaded");
  NEED_V(h, verb, !h->backsub_pending, "a damping try is in flight (psba_backsub_wait first)");
  NEED_V(h, verb, h->cnp != 6,
         "PSBA_SOLVER_SPARSE on free-intrinsics camera blocks only (six-parameter blocks: psba_covariance_compute)");
  NEED_V(h, verb, FREE_SPARSE(h),
         "PSBA_SOLVER_SPARSE only (psba_set_solver before the upload); the dense solver: psba_free_covariance_compute");
  NEED_V(h, verb, h->kd_rep_h.empty(),
         "not with shared intrinsics (psba_set_sparse_intrinsics_groups): the stored blocks are unfolded and undamped, and "
         "covariance under groups is not supported on this route");
  return PSBA_OK;
}

int psba_sparse_camera_covariance(psba_handle h, double mu, double scale, int reassemble, int n_sel, const int *sel, double *C,
                                  double *cols, int *iters, double *relres) {
  CHECK_H(h);
  TRY(need_free_sparse(h, __func__));
  if (!(std::isfinite(mu) && mu >= 0.0)) return fail(h, PSBA_E_INVALID, "%s: mu must be finite and >= 0 (got %.17g)", __func__, mu);
  if (!(std::isfinite(scale) && scale > 0.0))
    return fail(h, PSBA_E_INVALID, "%s: scale must be finite and > 0 (got %.17g)", __func__, scale);
  if (n_sel < 1 || !sel) return fail(h, PSBA_E_INVALID, "%s: n_sel = %d (at least one chosen camera, and its list)", __func__, n_sel);
  if (!C) return fail(h, PSBA_E_INVALID, "%s: C is a null pointer", __func__);
  {
    std::vector<int> at((size_t)h->d.nC, -1);
    for (int a = 0; a < n_sel; a++) {
      if (sel[a] < 0 || sel[a] >= h->d.nC)
        return fail(h, PSBA_E_INVALID, "%s: sel[%d] = %d names a camera out of range (%d cameras)", __func__, a, sel[a], h->d.nC);
      if (at[(size_t)sel[a]] >= 0)
        return fail(h, PSBA_E_INVALID, "%s: camera %d is listed twice (sel[%d] and sel[%d])", __func__, sel[a], at[(size_t)sel[a]], a);
      at[(size_t)sel[a]] = a;
    }
  }
  if (!reassemble) NEED(h, h->assembled, "reassemble = 0 works on the blocks as they stand (psba_schur_assemble first)");
  if (reassemble) {
    if (!(h->linearized && h->coeff == 1.0 && h->coeff_g == 1.0)) TRY(psba_linearize(h, 1.0, 1.0));
    TRY(psba_schur_assemble(h, mu));
  }
  h->precond_ok = false;  // (the block inverses go into the solve's buffer)
  const int rc = launch_fcovm_compute(h, scale, n_sel, sel, C, cols, iters, relres);
  if (rc == PSBA_NOT_SPD)
    h->err = std::string(__func__) + ": S is not positive definite on a chosen column (a pivot of a diagonal block, p.Sp <= 0, or a residual that is not finite)";
  else if (rc == PSBA_PCG_MAXIT)
    h->err = std::string(__func__) + ": a column used up max_iter (iters and relres say which)";
  return rc;
}

int psba_sparse_S_times_many(psba_handle h, int n_panels, const double *X, double *Y) {
  CHECK_H(h);
  TRY(need_free_sparse(h, __func__));
  NEED(h, h->assembled, "psba_schur_assemble first (the state of psba_get_sparse_S)");
  if (n_panels < 1 || !X || !Y) return fail(h, PSBA_E_INVALID, "%s: n_panels = %d, or a null pointer", __func__, n_panels);
  return launch_fbsr_times_many(h, n_panels, X, Y);
}

// ---- chosen points under PSBA_SOLVER_SPARSE (kernels_free_pcg_points.hip) ----

int psba_sparse_point_covariance(psba_handle h, double mu, double scale, int reassemble, int n_sel, const int *sel_pts, double *C,
                                 double *cols, int *iters, double *relres) {
  CHECK_H(h);
  TRY(need_free_sparse(h, __func__));
  if (!(std::isfinite(mu) && mu >= 0.0)) return fail(h, PSBA_E_INVALID, "%s: mu must be finite and >= 0 (got %.17g)", __func__, mu);
  if (!(std::isfinite(scale) && scale > 0.0))
    return fail(h, PSBA_E_INVALID, "%s: scale must be finite and > 0 (got %.17g)", __func__, scale);
  if (n_sel < 1 || !sel_pts) return fail(h, PSBA_E_INVALID, "%s: n_sel = %d (at least one chosen point, and its list)", __func__, n_sel);
  if (!C) return fail(h, PSBA_E_INVALID, "%s: C is a null pointer", __func__);
  {
    std::vector<int> at((size_t)h->d.nP, -1);
    for (int a = 0; a < n_sel; a++) {
      if (sel_pts[a] < 0 || sel_pts[a] >= h->d.nP)
        return fail(h, PSBA_E_INVALID, "%s: sel_pts[%d] = %d names a point out of range (%d points)", __func__, a, sel_pts[a], h->d.nP);
      if (at[(size_t)sel_pts[a]] >= 0)
        return fail(h, PSBA_E_INVALID, "%s: point %d is listed twice (sel_pts[%d] and sel_pts[%d])", __func__, sel_pts[a],
                    at[(size_t)sel_pts[a]], a);
      at[(size_t)sel_pts[a]] = a;
    }
  }
  if (!reassemble) NEED(h, h->assembled, "reassemble = 0 works on the blocks, V and Y as they stand (psba_schur_assemble first)");
  if (reassemble) {
    if (!(h->linearized && h->coeff == 1.0 && h->coeff_g == 1.0)) TRY(psba_linearize(h, 1.0, 1.0));
    TRY(psba_schur_assemble(h, mu));
  }
  h->precond_ok = false;  // (the block inverses go into the solve's buffer)
  const int rc = launch_fcovp_compute(h, mu, scale, n_sel, sel_pts, C, cols, iters, relres);
  if (rc == PSBA_NOT_SPD)
    h->err = std::string(__func__) + ": S is not positive definite on a chosen column (a pivot of a diagonal block, p.Sp <= 0, or a residual that is not finite)";
  else if (rc == PSBA_SINGULAR_V)
    h->err = std::string(__func__) + ": some chosen V_i + mu D_i is singular (D = I unless psba_set_damping chose Marquardt's rule)";
  else if (rc == PSBA_PCG_MAXIT)
    h->err = std::string(__func__) + ": a column used up max_iter (iters and relres say which)";
  return rc;
}

// test hook (psba_hip.h): V_i as the linearization stored it (undamped) and Y as k_free_Y stored it for the last assemble
int psba_get_free_point_blocks(psba_handle h, double *V, double *Y) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  NEED(h, h->cnp != 6, "free-intrinsics camera blocks only (six-parameter blocks: psba_compute_V, psba_compute_Yblks)");
  NEED(h, h->assembled, "an assembled try (psba_schur_assemble or psba_free_covariance_compute first; psba_schur_solve ends it)");
  if (V) {
    std::vector<double> pv((size_t)9 * h->d.nP);
    TRY(d2h(h, pv.data(), h->PV, sizeof(double) * pv.size()));
    for (int i = 0; i < h->d.nP; i++) {
      const double *p = pv.data() + (size_t)9 * i;  // sym6 packing (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) | g_b,i
      double *o = V + (size_t)9 * i;
      o[0] = p[0], o[1] = o[3] = p[1], o[2] = o[6] = p[2], o[4] = p[3], o[5] = o[7] = p[4], o[8] = p[5];
    }
  }
  if (Y) TRY(d2h(h, Y, h->free_Y, sizeof(double) * 3 * (size_t)h->cnp * h->d.nO));
  return PSBA_OK;
}
