// problem_options.cpp -- the settings of an uploaded problem (include/psba_hip.h): camera model, lens model,
// robust loss, fixed blocks, the mask, the per-camera masks and the groups of the intrinsics, held poses and points, priors, the observation weighting, the damping rule,
// and their getters.  Every setter is built from the same three pieces: settable() says whether it may run now,
// stage() puts new device tables in place all or nothing, model_changed() / params_changed() drop what was derived.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "api_common.h"
#include "camera_model.h"

using namespace psba;

namespace psba {

// A new derived-state flag is cleared here, and nowhere else.
void model_changed(psba_ctx *h) {
  h->ahead = false;
  h->lin_is_ahead = false;
  h->linearized = h->assembled = h->solved = false;
  h->free_obs = false;
  h->damp_ok = false;
  h->cov_ok = h->cov_pts_ok = false;
  h->precond_ok = false;
  h->lean_cur = h->lean_alt = false;  // (the linearizations they describe are gone)
}

void params_changed(psba_ctx *h) {
  model_changed(h);
  h->backsubbed = false;
}

int groups_split(psba_ctx *h, const char *who, const std::vector<int> &rep, const double *v, int stride, int ncols, int col0) {
  for (int j = 0; j < (int)rep.size(); j++)
    for (int k = 0; rep[j] != j && k < ncols; k++)
      if (memcmp(v + (size_t)stride * j + k, v + (size_t)stride * rep[j] + k, sizeof(double)) != 0)
        return fail(h, PSBA_E_INVALID, "%s: camera %d differs from camera %d, the representative of its group, in column %d "
                    "(%.17g against %.17g): members of a group hold bit-identical intrinsics",
                    who, j, rep[j], col0 + k, v[(size_t)stride * j + k], v[(size_t)stride * rep[j] + k]);
  return PSBA_OK;
}

}  // namespace psba

namespace {

enum Models { SIX_PARAM, FREE_MODELS, FREE_KD };  // the camera models a verb exists for
enum When { NO_TRY_IN_FLIGHT, ANY_TIME };         // setters / getters

// May the verb fn run now?  A problem is uploaded, its camera model is one of `allowed` (hint: where the other models
// find the same thing) and, for a setter, no damping try is in flight.
int settable(psba_ctx *h, const char *fn, Models allowed, const char *hint = "", When when = NO_TRY_IN_FLIGHT) {
  if (!h->uploaded) return fail(h, PSBA_E_STATE, "%s: no problem uploaded", fn);
  const char *only = nullptr;
  if (allowed == SIX_PARAM && h->cnp != 6) only = "the fixed-intrinsics camera block only (not PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD)";
  if (allowed == FREE_MODELS && h->cnp == 6) only = "free-intrinsics models only (PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD)";
  if (allowed == FREE_KD && h->cnp != KD_CNP) only = "PSBA_CAMERA_FREE_KD only";
  if (only) return fail(h, PSBA_E_STATE, "%s: %s%s", fn, only, hint);
  if (when == NO_TRY_IN_FLIGHT && h->backsub_pending)
    return fail(h, PSBA_E_STATE, "%s: a damping try is in flight (psba_backsub_wait first)", fn);
  return PSBA_OK;
}

// One device table of a setter on its way in: the member it replaces and the host data (empty: the member is released).
template <typename T>
struct Staged {
  Staged(DevBuf<T> &m, const std::vector<T> &v) : member(m), host(v) {}
  int alloc(psba_ctx *h) { return host.empty() ? PSBA_OK : buf.alloc(h, host.size()); }
  int copy(psba_ctx *h) {
    if (!host.empty()) PSBA_HIP(h, hipMemcpyAsync(buf, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice, h->stream));
    return PSBA_OK;
  }
  DevBuf<T> &member;
  const std::vector<T> &host;
  DevBuf<T> buf;
};

// All or nothing: every table is allocated in a buffer of its own, every copy queued, the stream waited for once
// (whatever failed: a staged buffer and the host data outlive the copies, and nothing queued still reads the old tables)
// and only then, if all went well, the buffers are swapped into the handle.  A call that fails leaves the handle as it was.
template <typename... S>
int stage(psba_ctx *h, S &&...s) {
  int rc = PSBA_OK;
  ((rc = rc != PSBA_OK ? rc : s.alloc(h)), ...);
  ((rc = rc != PSBA_OK ? rc : s.copy(h)), ...);
  const hipError_t e = hipStreamSynchronize(h->stream);
  if (rc != PSBA_OK) return rc;
  PSBA_HIP(h, e);
  ((s.member = std::move(s.buf)), ...);
  return PSBA_OK;
}

// a byte mask as 0 / 1 (NULL: all zero) and the number of its ones
std::vector<unsigned char> flags01(const unsigned char *f, int n, int *ones) {
  std::vector<unsigned char> v((size_t)n, 0);
  for (int j = 0; f && j < n; j++) v[j] = f[j] ? 1 : 0;
  *ones = (int)std::count(v.begin(), v.end(), 1);
  return v;
}

}  // namespace

extern "C" {

int psba_set_camera_model(psba_handle h, int model) {
  CHECK_H(h);
  if (model != PSBA_CAMERA_FIXED_K && model != PSBA_CAMERA_FREE_K && model != PSBA_CAMERA_FREE_KD)
    return fail(h, PSBA_E_INVALID, "unknown camera model %d", model);
  NEED(h, !h->uploaded, "psba_set_camera_model before psba_upload_problem (every buffer depends on the camera block)");
  h->cnp = model == PSBA_CAMERA_FREE_KD ? KD_CNP : model == PSBA_CAMERA_FREE_K ? FK_CNP : 6;
  return PSBA_OK;
}

// ---- lens model (camera_model.h) -------------------------------------------------------------
// PSBA_CAMERA_FREE_KD: kc is part of the camera block -- the starting values go into columns 5..9 of the current
// parameters and of the copy psba_reset_params restores
static int set_start_distortion(psba_ctx *h, const double *kc) {
  const int nC = h->d.nC;
  for (int t = 0; kc && t < 5 * nC; t++)
    if (!std::isfinite(kc[t])) return fail(h, PSBA_E_INVALID, "psba_set_distortion: kc[%d] of camera %d is not finite", t % 5, t / 5);
  if (kc && !h->kd_rep_h.empty()) TRY(groups_split(h, "psba_set_distortion", h->kd_rep_h, kc, 5, 5, 5));
  std::vector<double> c((size_t)h->d.nA);
  double *dst[2] = {h->cams[h->cur], h->params0};
  for (int k = 0; k < 2; k++) {
    PSBA_HIP(h, hipMemcpyAsync(c.data(), dst[k], sizeof(double) * c.size(), hipMemcpyDeviceToHost, h->stream));
    PSBA_HIP(h, hipStreamSynchronize(h->stream));
    for (int j = 0; j < nC; j++)
      for (int q = 0; q < 5; q++) c[(size_t)KD_CNP * j + 5 + q] = kc ? kc[5 * j + q] : 0.0;
    PSBA_HIP(h, hipMemcpyAsync(dst[k], c.data(), sizeof(double) * c.size(), hipMemcpyHostToDevice, h->stream));
    PSBA_HIP(h, hipStreamSynchronize(h->stream));
  }
  params_changed(h);
  return PSBA_OK;
}

int psba_set_distortion(psba_handle h, const double *kc) {
  CHECK_H(h);
  TRY(settable(h, __func__, h->cnp == KD_CNP ? FREE_KD : SIX_PARAM));
  if (h->cnp == KD_CNP) return set_start_distortion(h, kc);
  if (!kc) {
    h->lens_kc.reset();
    h->lens &= ~LENS_DIST;
  } else {
    for (int t = 0; t < 5 * h->d.nC; t++)
      if (!std::isfinite(kc[t])) return fail(h, PSBA_E_INVALID, "%s: kc[%d] of camera %d is not finite", __func__, t % 5, t / 5);
    if (!h->lens_kc) TRY(h->lens_kc.alloc(h, (size_t)5 * h->d.nC));
    PSBA_HIP(h, hipMemcpyAsync(h->lens_kc, kc, sizeof(double) * 5 * (size_t)h->d.nC, hipMemcpyHostToDevice, h->stream));
    PSBA_HIP(h, hipStreamSynchronize(h->stream));
    h->lens |= LENS_DIST;
  }
  model_changed(h);
  return PSBA_OK;
}

int psba_set_obs_covariance(psba_handle h, const double *cov) {
  CHECK_H(h);
  TRY(settable(h, __func__, SIX_PARAM));
  if (!cov) {
    h->lens_w.reset();
    h->lens &= ~LENS_COV;
    model_changed(h);
    return PSBA_OK;
  }
  // Sigma = [p q; q r] -> Sigma^-1 = [r -q; -q p] / det = L^T L, L = [l00 l01; 0 l11]
  std::vector<double> w((size_t)LENS_WSTRIDE * h->d.nO, 0.0);
  for (int a = 0; a < h->d.nO; a++) {
    const double *c = cov + 4 * (size_t)a;
    const double p = c[0], r = c[3];
    const double big = std::fmax(std::fmax(std::fabs(c[0]), std::fabs(c[1])), std::fmax(std::fabs(c[2]), std::fabs(c[3])));
    if (!(std::isfinite(p) && std::isfinite(c[1]) && std::isfinite(c[2]) && std::isfinite(r)))
      return fail(h, PSBA_E_INVALID, "%s: covariance of observation %d is not finite", __func__, a);
    if (std::fabs(c[1] - c[2]) > 1e-12 * big)
      return fail(h, PSBA_E_INVALID, "%s: covariance of observation %d is not symmetric (%.17g vs %.17g)", __func__, a, c[1], c[2]);
    const double q = 0.5 * (c[1] + c[2]);
    const double det = p * r - q * q;
    if (!(p > 0.0) || !(det > 0.0))
      return fail(h, PSBA_E_INVALID, "%s: covariance of observation %d is not positive definite", __func__, a);
    const double i00 = r / det, i01 = -q / det, i11 = p / det;
    const double l00 = std::sqrt(i00), l01 = i01 / l00;
    const double t = i11 - l01 * l01;
    if (!(t > 0.0)) return fail(h, PSBA_E_INVALID, "%s: covariance of observation %d is not positive definite", __func__, a);
    w[(size_t)LENS_WSTRIDE * a] = l00;
    w[(size_t)LENS_WSTRIDE * a + 1] = l01;
    w[(size_t)LENS_WSTRIDE * a + 2] = std::sqrt(t);
  }
  if (!h->lens_w) TRY(h->lens_w.alloc(h, w.size()));
  PSBA_HIP(h, hipMemcpyAsync(h->lens_w, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  h->lens |= LENS_COV;
  model_changed(h);
  return PSBA_OK;
}

int psba_lens_model(psba_handle h, int *has_distortion, int *has_covariance) {
  CHECK_H(h);
  if (has_distortion) *has_distortion = ((h->lens & LENS_DIST) || h->cnp == KD_CNP) ? 1 : 0;
  if (has_covariance) *has_covariance = (h->lens & LENS_COV) ? 1 : 0;
  return PSBA_OK;
}

// ---- robust loss (camera_model.h RobustLoss) ----
static_assert(PSBA_LOSS_NONE == LOSS_NONE && PSBA_LOSS_HUBER == LOSS_HUBER && PSBA_LOSS_CAUCHY == LOSS_CAUCHY &&
                  PSBA_LOSS_SOFT_L1 == LOSS_SOFT_L1,
              "loss kinds of the C ABI and the kernels");

int psba_set_robust_loss(psba_handle h, int kind, double scale) {
  CHECK_H(h);
  TRY(settable(h, __func__, SIX_PARAM));
  if (kind < PSBA_LOSS_NONE || kind > PSBA_LOSS_SOFT_L1) return fail(h, PSBA_E_INVALID, "%s: unknown loss kind %d", __func__, kind);
  if (!(std::isfinite(scale) && scale > 0.0))
    return fail(h, PSBA_E_INVALID, "%s: the scale must be finite and > 0 (got %.17g)", __func__, scale);
  h->loss_kind = kind;
  h->loss_c = scale;
  if (kind == PSBA_LOSS_NONE)
    h->lens &= ~LENS_ROBUST;  // the plain instantiations: bit for bit what a handle that never set a loss computes
  else
    h->lens |= LENS_ROBUST;
  model_changed(h);
  return PSBA_OK;
}

int psba_robust_loss(psba_handle h, int *kind, double *scale) {
  CHECK_H(h);
  if (kind) *kind = h->loss_kind;
  if (scale) *scale = h->loss_c;
  return PSBA_OK;
}

// ---- fixed parameter blocks (camera_model.h FixedMask) ----
int psba_set_fixed(psba_handle h, const unsigned char *fixed_cams, const unsigned char *fixed_pts) {
  CHECK_H(h);
  TRY(settable(h, __func__, SIX_PARAM));
  const int nC = h->d.nC, nP = h->d.nP;
  int nfc = 0, nfp = 0;
  std::vector<unsigned char> fc = flags01(fixed_cams, nC, &nfc), fp = flags01(fixed_pts, nP, &nfp);
  // (under a rank layout this rank sees only its own points: the other ranks' may be free)
  if (h->nranks == 1 && nfc == nC && nfp == nP)
    return fail(h, PSBA_E_INVALID, "%s: every camera and every point is fixed: no free parameter is left", __func__);
  // a mask without a non-zero entry is no mask: only the kinds that have one get a buffer
  if (!nfc) fc.clear();
  if (!nfp) fp.clear();
  TRY(stage(h, Staged(h->fix_cams, fc), Staged(h->fix_pts, fp)));
  h->n_fix_cams = nfc;
  h->n_fix_pts = nfp;
  h->has_fixed = nfc > 0 || nfp > 0;  // none: the plain kernel instantiations, as on a handle that never set a mask
  h->struct_only = nfc == nC;
  h->try_shortcut = false;
  model_changed(h);
  return PSBA_OK;
}

int psba_fixed_counts(psba_handle h, int *n_fixed_cams, int *n_fixed_pts) {
  CHECK_H(h);
  if (n_fixed_cams) *n_fixed_cams = h->n_fix_cams;
  if (n_fixed_pts) *n_fixed_pts = h->n_fix_pts;
  return PSBA_OK;
}

// ---- per-parameter mask of the ten intrinsics (PSBA_CAMERA_FREE_KD) ----
int psba_set_intrinsics_mask(psba_handle h, const unsigned char *free10) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_KD));
  unsigned m = 0;
  for (int k = 0; k < 10; k++) m |= (!free10 || free10[k]) ? 1u << k : 0u;
  h->kd_mask = m;
  model_changed(h);
  return PSBA_OK;
}

int psba_intrinsics_mask(psba_handle h, unsigned char *out10) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_KD, "", ANY_TIME));
  for (int k = 0; out10 && k < 10; k++) out10[k] = (h->kd_mask >> k) & 1u;
  return PSBA_OK;
}

// ---- per-camera masks of the ten intrinsics (PSBA_CAMERA_FREE_KD) ----
// the members of a group carry equal rows: whichever of the two setters comes second checks it on the host tables
static int masks_split(psba_ctx *h, const char *who, const std::vector<int> &rep, const std::vector<unsigned short> &cm) {
  static const char *names[10] = {"fu", "u0", "v0", "ar", "s", "k1", "k2", "k3", "k4", "k5"};
  for (int j = 0; j < (int)rep.size() && !cm.empty(); j++) {
    const unsigned diff = (unsigned)(cm[j] ^ cm[rep[j]]);
    if (!diff) continue;
    int k = 0;
    while (!((diff >> k) & 1u)) k++;
    return fail(h, PSBA_E_INVALID, "%s: camera %d and camera %d, the representative of its group, differ in coordinate %d "
                "(%s) of their rows of psba_set_camera_masks: the members of a group carry equal rows",
                who, j, rep[j], k, names[k]);
  }
  return PSBA_OK;
}

int psba_set_camera_masks(psba_handle h, const unsigned char *free10_per_cam) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_KD, "; blocks of 11 (PSBA_CAMERA_FREE_K) have no mask"));
  const int nC = h->d.nC;
  std::vector<unsigned short> cm;
  bool any_zero = false;
  if (free10_per_cam) {
    cm.assign((size_t)nC, 0);
    for (int j = 0; j < nC; j++)
      for (int k = 0; k < 10; k++) {
        if (free10_per_cam[10 * (size_t)j + k])
          cm[j] |= (unsigned short)(1u << k);
        else
          any_zero = true;
      }
  }
  if (!any_zero) cm.clear();  // a table without a zero entry is no table: no buffer, the kernels read the global mask alone
  if (!h->kd_rep_h.empty()) TRY(masks_split(h, __func__, h->kd_rep_h, cm));
  TRY(stage(h, Staged(h->kd_cmask, cm)));
  h->kd_cmask_h = std::move(cm);
  model_changed(h);
  return PSBA_OK;
}

int psba_camera_masks(psba_handle h, unsigned char *out10_per_cam) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_KD, "; blocks of 11 (PSBA_CAMERA_FREE_K) have no mask", ANY_TIME));
  for (int j = 0; out10_per_cam && j < h->d.nC; j++)
    for (int k = 0; k < 10; k++) out10_per_cam[10 * (size_t)j + k] = h->kd_cmask_h.empty() ? 1 : (h->kd_cmask_h[j] >> k) & 1u;
  return PSBA_OK;
}

// ---- intrinsics shared between cameras (PSBA_CAMERA_FREE_KD) ----
// the body of both setters: labels -> rep / gidx / gptr / gmem, the checks of the masks and of the members' intrinsics,
// the tables staged all or nothing.  sparse: also the buffers of the folded diagonal blocks (kernels_free_pcg.hip)
static int set_groups(psba_ctx *h, const char *fn, const int *group_of_cam, bool sparse) {
  const int nC = h->d.nC;
  // the representative of a label is the first camera that carries it
  std::vector<int> rep((size_t)nC), order((size_t)nC);
  for (int j = 0; j < nC; j++) order[j] = j;
  if (group_of_cam)
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return group_of_cam[a] < group_of_cam[b]; });
  int ngroups = 0;
  for (int t = 0; t < nC; t++) {
    const bool first = !group_of_cam || t == 0 || group_of_cam[order[t]] != group_of_cam[order[t - 1]];
    rep[order[t]] = first ? order[t] : rep[order[t - 1]];
    ngroups += first ? 1 : 0;
  }
  std::vector<int> gidx, gptr, gmem;
  if (ngroups < nC) {
    TRY(masks_split(h, fn, rep, h->kd_cmask_h));  // (host tables: before anything is read from the device)
    std::vector<double> c((size_t)h->d.nA);
    const double *src[2] = {h->cams[h->cur], h->params0};
    const std::string who[2] = {std::string(fn) + " (current parameters)", std::string(fn) + " (the psba_reset_params copy)"};
    for (int k = 0; k < 2; k++) {
      TRY(d2h(h, c.data(), src[k], sizeof(double) * c.size()));
      TRY(groups_split(h, who[k].c_str(), rep, c.data(), KD_CNP, 10, 0));
    }
    std::vector<int> count((size_t)nC, 0);
    for (int j = 0; j < nC; j++) count[rep[j]]++;
    gidx.assign((size_t)nC, -1);
    gptr.assign(1, 0);
    for (int j = 0; j < nC; j++)  // groups in the order of their representatives, members ascending
      if (rep[j] == j && count[j] > 1) {
        for (int m = j; m < nC; m++)
          if (rep[m] == j) {
            gidx[m] = (int)gptr.size() - 1;
            gmem.push_back(m);
          }
        gptr.push_back((int)gmem.size());
      }
  } else {
    rep.clear();  // (every camera alone is no grouping: no tables, the ungrouped launches)
  }
  const int nmg = rep.empty() ? 0 : (int)gptr.size() - 1;
  DevBuf<double> part, blk;
  if (sparse && nmg) {
    TRY(part.alloc(h, (size_t)10 * KD_CNP * gmem.size()));
    TRY(blk.alloc(h, (size_t)KD_CNP * KD_CNP * nmg));
  }
  TRY(stage(h, Staged(h->kd_rep, rep), Staged(h->kd_gidx, gidx), Staged(h->kd_gptr, gptr), Staged(h->kd_gmem, gmem)));
  h->fg_part = std::move(part);
  h->fg_blk = std::move(blk);
  h->kd_ngroups = rep.empty() ? 0 : ngroups;
  h->kd_nmg = nmg;
  h->kd_nmem = (int)gmem.size();
  h->kd_rep_h = std::move(rep);
  model_changed(h);
  return PSBA_OK;
}

int psba_set_intrinsics_groups(psba_handle h, const int *group_of_cam) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_KD));
  NEED(h, !FREE_SPARSE(h), "not under PSBA_SOLVER_SPARSE: the fold sums rows and columns of a dense S "
                           "(psba_set_sparse_intrinsics_groups folds inside the solve)");
  return set_groups(h, __func__, group_of_cam, false);
}

// ... on a PSBA_SOLVER_SPARSE handle: the same tables; the list stays unfolded and the solve folds
int psba_set_sparse_intrinsics_groups(psba_handle h, const int *group_of_cam) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_KD, "; the other camera blocks have no groups (as under psba_set_intrinsics_groups)"));
  NEED(h, FREE_SPARSE(h), "PSBA_SOLVER_SPARSE only (psba_set_solver before the upload); the dense solver: psba_set_intrinsics_groups");
  return set_groups(h, __func__, group_of_cam, true);
}

int psba_intrinsics_groups(psba_handle h, int *rep_of_cam, int *n_groups) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_KD, "", ANY_TIME));
  for (int j = 0; rep_of_cam && j < h->d.nC; j++) rep_of_cam[j] = h->kd_rep_h.empty() ? j : h->kd_rep_h[j];
  if (n_groups) *n_groups = h->kd_rep_h.empty() ? h->d.nC : h->kd_ngroups;
  return PSBA_OK;
}

// ---- held poses and points of the free-intrinsics route ----
int psba_set_held(psba_handle h, const unsigned char *held_poses, const unsigned char *held_pts) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_MODELS, "; six-parameter blocks are held as a whole by psba_set_fixed"));
  const int nC = h->d.nC, nP = h->d.nP;
  int nhc = 0, nhp = 0;
  std::vector<unsigned char> hc = flags01(held_poses, nC, &nhc), hp = flags01(held_pts, nP, &nhp);
  if (nhc == nC && nhp == nP)
    return fail(h, PSBA_E_INVALID, "%s: every pose and every point is held (a resection of the intrinsics alone is not supported)",
                __func__);
  // a mask without a non-zero entry is no mask; with one in either, both masks go to the device (the kernels test no pointer)
  if (!nhc && !nhp) {
    hc.clear();
    hp.clear();
  }
  TRY(stage(h, Staged(h->held_poses, hc), Staged(h->held_pts, hp)));
  h->n_held_poses = nhc;
  h->n_held_pts = nhp;
  h->has_held = nhc > 0 || nhp > 0;
  model_changed(h);
  return PSBA_OK;
}

int psba_held_counts(psba_handle h, int *n_held_poses, int *n_held_pts) {
  CHECK_H(h);
  if (n_held_poses) *n_held_poses = h->n_held_poses;
  if (n_held_pts) *n_held_pts = h->n_held_pts;
  return PSBA_OK;
}

// ---- Gaussian priors on cameras and points of the free-intrinsics route ----
// one kind: n blocks of m parameters; checks every block and compacts those whose information is not all zero into
// idx [n] (-1: none), list and rec [mean (m) | information (m x m), symmetrised]
static int priors_pack(psba_ctx *h, const char *what, int n, int m, const double *mean, const double *info,
                       std::vector<int> &idx, std::vector<int> &list, std::vector<double> &rec) {
  idx.assign((size_t)n, -1);
  for (int b = 0; mean && b < n; b++) {
    const double *mu = mean + (size_t)m * b, *L = info + (size_t)m * m * b;
    double big = 0.0;
    for (int r = 0; r < m; r++)
      if (!std::isfinite(mu[r])) return fail(h, PSBA_E_INVALID, "psba_set_priors: mean[%d] of %s %d is not finite", r, what, b);
    for (int t = 0; t < m * m; t++) {
      if (!std::isfinite(L[t]))
        return fail(h, PSBA_E_INVALID, "psba_set_priors: information[%d][%d] of %s %d is not finite", t / m, t % m, what, b);
      big = std::fmax(big, std::fabs(L[t]));
    }
    for (int r = 0; r < m; r++)
      if (L[m * r + r] < 0.0)
        return fail(h, PSBA_E_INVALID, "psba_set_priors: information[%d][%d] of %s %d is negative (%.17g)", r, r, what, b,
                    L[m * r + r]);
    for (int r = 0; r < m; r++)
      for (int c = r + 1; c < m; c++)
        if (std::fabs(L[m * r + c] - L[m * c + r]) > 1e-12 * big)
          return fail(h, PSBA_E_INVALID, "psba_set_priors: information of %s %d is not symmetric at [%d][%d] (%.17g vs %.17g)",
                      what, b, r, c, L[m * r + c], L[m * c + r]);
    if (big == 0.0) continue;  // all zero: no prior
    idx[b] = (int)list.size();
    list.push_back(b);
    rec.insert(rec.end(), mu, mu + m);
    for (int r = 0; r < m; r++)
      for (int c = 0; c < m; c++) rec.push_back(0.5 * (L[m * r + c] + L[m * c + r]));
  }
  return PSBA_OK;
}

int psba_set_priors(psba_handle h, const double *cam_mean, const double *cam_info, const double *pt_mean,
                    const double *pt_info) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_MODELS, "; six-parameter blocks carry no priors"));
  if ((cam_mean == nullptr) != (cam_info == nullptr))
    return fail(h, PSBA_E_INVALID, "psba_set_priors: cam_mean and cam_info are both NULL or both given");
  if ((pt_mean == nullptr) != (pt_info == nullptr))
    return fail(h, PSBA_E_INVALID, "psba_set_priors: pt_mean and pt_info are both NULL or both given");
  const int nC = h->d.nC, nP = h->d.nP, cnp = h->cnp;
  std::vector<int> cidx, pidx, clist, plist;
  std::vector<double> crec, prec;
  TRY(priors_pack(h, "camera", nC, cnp, cam_mean, cam_info, cidx, clist, crec));
  TRY(priors_pack(h, "point", nP, 3, pt_mean, pt_info, pidx, plist, prec));
  const int ncp = (int)clist.size(), npp = (int)plist.size();
  // no block with a prior is no priors.  With one, every table goes to the device (the kernels test no pointer): a kind
  // without priors keeps one unused element
  if (ncp || npp) {
    if (clist.empty()) clist.push_back(0);
    if (plist.empty()) plist.push_back(0);
    if (crec.empty()) crec.assign((size_t)cnp + cnp * cnp, 0.0);
    if (prec.empty()) prec.assign(12, 0.0);
  } else {
    cidx.clear();
    pidx.clear();
  }
  TRY(stage(h, Staged(h->prior_cidx, cidx), Staged(h->prior_pidx, pidx), Staged(h->prior_clist, clist),
            Staged(h->prior_plist, plist), Staged(h->prior_crec, crec), Staged(h->prior_prec, prec)));
  h->n_cam_priors = ncp;
  h->n_pt_priors = npp;
  h->has_prior = ncp > 0 || npp > 0;
  model_changed(h);
  return PSBA_OK;
}

int psba_prior_counts(psba_handle h, int *n_cam_priors, int *n_pt_priors) {
  CHECK_H(h);
  if (n_cam_priors) *n_cam_priors = h->n_cam_priors;
  if (n_pt_priors) *n_pt_priors = h->n_pt_priors;
  return PSBA_OK;
}

int psba_prior_cost(psba_handle h, int which, double *cams_part, double *pts_part) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_MODELS));  // (it launches a kernel: not while a try is in flight)
  if (which != PSBA_PARAMS_CUR && which != PSBA_PARAMS_NEW) return fail(h, PSBA_E_INVALID, "%s: which = %d", __func__, which);
  double out[2] = {0.0, 0.0};
  if (h->has_prior) {
    if (!h->prior_out) TRY(h->prior_out.alloc(h, 2));
    TRY(launch_prior_cost_free(h, which, h->prior_out));
    TRY(d2h(h, out, h->prior_out, sizeof(out)));
  } else {
    PSBA_HIP(h, hipStreamSynchronize(h->stream));
  }
  if (cams_part) *cams_part = out[0];
  if (pts_part) *pts_part = out[1];
  return PSBA_OK;
}

// ---- observation weighting of the free-intrinsics route ----
int psba_set_obs_weighting(psba_handle h, int loss_kind, double loss_scale, const double *sigma) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_MODELS, "; six-parameter blocks: psba_set_robust_loss / psba_set_obs_covariance"));
  if (loss_kind < PSBA_LOSS_NONE || loss_kind > PSBA_LOSS_SOFT_L1)
    return fail(h, PSBA_E_INVALID, "%s: unknown loss kind %d", __func__, loss_kind);
  if (!(std::isfinite(loss_scale) && loss_scale > 0.0))
    return fail(h, PSBA_E_INVALID, "%s: the scale must be finite and > 0 (got %.17g)", __func__, loss_scale);
  const int nO = h->d.nO;
  for (int a = 0; sigma && a < nO; a++)
    if (!(std::isfinite(sigma[a]) && sigma[a] > 0.0 && std::isfinite(1.0 / sigma[a])))  // (the reciprocal is what is stored)
      return fail(h, PSBA_E_INVALID, "%s: sigma of observation %d must be finite and > 0 (got %.17g)", __func__, a, sigma[a]);
  // (none, any scale, no sigmas) is no weighting: no table, the plain instantiations.  With a loss alone the table holds
  // ones (the kernels test no pointer)
  const bool on = loss_kind != PSBA_LOSS_NONE || sigma;
  std::vector<double> isig;
  if (on) isig.assign((size_t)nO, 1.0);
  for (int a = 0; sigma && a < nO; a++) isig[a] = 1.0 / sigma[a];
  TRY(stage(h, Staged(h->obs_isig, isig)));
  h->wgt_kind = loss_kind;
  h->wgt_c = loss_scale;
  h->wgt_sigma = sigma != nullptr;
  h->has_weighting = on;
  model_changed(h);
  return PSBA_OK;
}

int psba_obs_weighting(psba_handle h, int *loss_kind, double *loss_scale, int *has_sigma) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_MODELS, "", ANY_TIME));
  if (loss_kind) *loss_kind = h->wgt_kind;
  if (loss_scale) *loss_scale = h->wgt_c;
  if (has_sigma) *has_sigma = h->wgt_sigma ? 1 : 0;
  return PSBA_OK;
}

// ---- the damping rule of the free-intrinsics route ----
int psba_set_damping(psba_handle h, int kind, double dmin, double dmax) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_MODELS, "; six-parameter blocks keep the reference's N + mu I"));
  if (kind != PSBA_DAMPING_IDENTITY && kind != PSBA_DAMPING_MARQUARDT)
    return fail(h, PSBA_E_INVALID, "psba_set_damping: unknown kind %d", kind);
  if (dmin == 0.0) dmin = 1e-6;
  if (dmax == 0.0) dmax = 1e32;
  if (!(std::isfinite(dmin) && std::isfinite(dmax) && dmin > 0.0 && dmin <= dmax))
    return fail(h, PSBA_E_INVALID, "psba_set_damping: clamps (%g, %g): 0 < dmin <= dmax, both finite (0 = the default)", dmin,
                dmax);
  if (kind == PSBA_DAMPING_MARQUARDT && !h->damp_D) {  // both sets or none: a refused call changes nothing
    DevBuf<double> D, D_alt;
    TRY(D.alloc(h, (size_t)h->d.nT));
    TRY(D_alt.alloc(h, (size_t)h->d.nT));
    h->damp_D = std::move(D);
    h->damp_D_alt = std::move(D_alt);
  }
  h->damp_kind = kind;
  h->damp_dmin = dmin;
  h->damp_dmax = dmax;
  model_changed(h);  // (a linearization queued ahead carries no D, or one of other clamps)
  return PSBA_OK;
}

int psba_damping(psba_handle h, int *kind, double *dmin, double *dmax) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_MODELS, "", ANY_TIME));
  if (kind) *kind = h->damp_kind;
  if (dmin) *dmin = h->damp_dmin;
  if (dmax) *dmax = h->damp_dmax;
  return PSBA_OK;
}

// test hook (psba_hip.h): D as k_free_damp_diag stored it for the current linearization
int psba_get_damping_diag(psba_handle h, double *D) {
  CHECK_H(h);
  TRY(settable(h, __func__, FREE_MODELS, "", ANY_TIME));
  NEED(h, h->damp_kind == PSBA_DAMPING_MARQUARDT, "psba_set_damping(PSBA_DAMPING_MARQUARDT) first");
  NEED(h, h->damp_ok, "psba_linearize first (every verb that moves the parameters or the model invalidates the diagonal)");
  return d2h(h, D, h->damp_D, sizeof(double) * (size_t)h->d.nT);
}

}  // extern "C"
