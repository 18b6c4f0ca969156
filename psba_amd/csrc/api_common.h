// api_common.h -- what the files of the C-ABI host layer share (psba_api.cpp, problem_options.cpp, covariance.cpp):
// the macros every entry point opens with and the few helpers that cross the files.
#pragma once
#include <vector>

#include "psba_internal.h"

// every entry point makes the handle's device current: a host may keep handles on several GPUs
// in one process, or call from a thread whose current device is another one
// With a communicator the try's scalar all-reduce and its copy to the host run on a side stream
// (psba_backsub_async), beside the linearization that is queued ahead; whatever else is queued on
// the main stream before psba_backsub_wait has returned must come after them.
#define CHECK_H_NOJOIN(h)                 \
  do {                                    \
    if (!(h)) return PSBA_E_INVALID;      \
    (void)hipSetDevice((h)->device);      \
  } while (0)
#define CHECK_H(h)                                                         \
  do {                                                                     \
    CHECK_H_NOJOIN(h);                                                     \
    if ((h)->scal_side) {                                                  \
      (void)hipStreamWaitEvent((h)->stream, (h)->scal_event, 0);           \
      (h)->scal_side = false;                                              \
    }                                                                      \
  } while (0)
#define NEED(h, cond, what)                                             \
  do {                                                                  \
    if (!(cond)) return fail((h), PSBA_E_STATE, "%s: %s", __func__, what); \
  } while (0)
// the verbs that exist for the six-parameter camera block only
#define SIX_ONLY "six-parameter camera blocks only (PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD: the fused verbs and psba_levmar)"
#define NEED_SIX(h) NEED(h, (h)->cnp == 6, SIX_ONLY)
// the verbs that read or write the dense reduce buffer or the Cholesky chain's factor: under PSBA_SOLVER_PCG neither
// exists (one double each is allocated), so they refuse on the host before any copy or launch.  FREE_SPARSE: the handle
// runs PSBA_SOLVER_SPARSE on camera blocks of 11 / 16 (kernels_free_pcg.hip), where the text names that solver
#define FREE_SPARSE(h) ((h)->cnp != 6 && (h)->solver == PSBA_SOLVER_PCG && (h)->sparse_any_block)
#define NEED_DENSE(h)                                                                                                   \
  do {                                                                                                                  \
    NEED(h, !FREE_SPARSE(h), "no dense S and no Cholesky chain with PSBA_SOLVER_SPARSE (psba_schur_solve, psba_get_sparse_S)"); \
    NEED(h, (h)->solver != PSBA_SOLVER_PCG, "no dense S and no Cholesky chain with PSBA_SOLVER_PCG (psba_schur_solve, psba_get_sparse_S)"); \
  } while (0)
#define RCCL(h, call)                                                                   \
  do {                                                                                  \
    ncclResult_t r__ = (call);                                                          \
    if (r__ != ncclSuccess)                                                             \
      return fail((h), PSBA_E_RCCL, "%s failed: %s", #call, ncclGetErrorString(r__));   \
  } while (0)
#define TRY(expr)                 \
  do {                            \
    int rc__ = (expr);            \
    if (rc__ < 0) return rc__;    \
  } while (0)

namespace psba {

// bytes from the device into dst (NULL: nothing) on the handle's stream, waited for (psba_api.cpp)
int d2h(psba_ctx *h, void *dst, const void *src, size_t bytes);

// members of a group hold bit-identical intrinsics: v[stride j + k], k < ncols, against the representative's; the
// message counts columns from col0 (the camera block's numbering) (problem_options.cpp)
int groups_split(psba_ctx *h, const char *who, const std::vector<int> &rep, const double *v, int stride, int ncols, int col0);

// The two invalidations (problem_options.cpp).  model_changed: a setting of the problem changed, so whatever was derived
// from the model is stale -- the linearization (current, queued ahead or kept for the next psba_linearize), the try's
// system and solution, the per-observation blocks, the damping diagonal and the covariance.  The try's result stays:
// psba_accept may still take the proposal.  params_changed: the current parameters moved, so the proposal goes too.
void model_changed(psba_ctx *h);
void params_changed(psba_ctx *h);

}  // namespace psba
