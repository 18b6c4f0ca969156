// psba_api.cpp -- the thin C-ABI HIP host layer (include/psba_hip.h).
// Takes the place of PSBA/cl_psba.cpp (runtime, buffers, uploads), PSBA/sba_func.cpp (one
// host wrapper per kernel), PSBA/cl_spdinv.cpp + PSBA/cl_linearalg.cpp (dense solve) and
// PSBA/misc.cpp:178-217 (index generation) of the reference.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <new>
#include <vector>

#include "api_common.h"
#include "camera_model.h"

using namespace psba;

static thread_local std::string g_create_err;

namespace psba {

int fail(psba_ctx *h, int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h)
    h->err = buf;
  else
    g_create_err = buf;
  return code;
}

int mirror_refused(psba_ctx *h) {
  return fail(h, PSBA_E_STATE, "the sba_func.h mirror is six-parameter only (not PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD)");
}

ProfScope::ProfScope(psba_ctx *hh, int kind) : h(hh) {
  if (kind < 0 || !(h->prof & (1u << kind))) return;
  if (h->spans_used == h->spans.size()) {
    psba_ctx::Span s;
    s.kind = kind;
    if (hipEventCreateWithFlags(&s.a, hipEventDisableSystemFence) != hipSuccess ||
        hipEventCreateWithFlags(&s.b, hipEventDisableSystemFence) != hipSuccess)
      return;
    h->spans.push_back(s);
  }
  idx = (int)h->spans_used++;
  h->spans[idx].kind = kind;
  (void)hipEventRecord(h->spans[idx].a, h->stream);
}
ProfScope::~ProfScope() {
  if (idx >= 0) (void)hipEventRecord(h->spans[idx].b, h->stream);
}

int alloc_bytes(psba_ctx *h, void **p, size_t bytes, bool pinned) {
  *p = nullptr;
  if (pinned) {
    if (hipHostMalloc(p, bytes) != hipSuccess) return fail(h, PSBA_E_NOMEM, "no pinned memory (%zu bytes)", bytes);
    return PSBA_OK;
  }
  PSBA_HIP(h, hipMalloc(p, bytes));
  static const bool poison = getenv("PSBA_DEBUG_POISON") != nullptr;
  if (poison) {
    PSBA_HIP(h, hipMemsetAsync(*p, 0xFF, bytes, h->stream));
    PSBA_HIP(h, hipStreamSynchronize(h->stream));
  }
  return PSBA_OK;
}

int d2h(psba_ctx *h, void *dst, const void *src, size_t bytes) {
  if (!dst) return PSBA_OK;
  PSBA_HIP(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  return PSBA_OK;
}

}  // namespace psba

// v on the device, in a buffer of its own (the blocking copy goes through the null stream: psba_upload_problem ends
// with a device-wide synchronisation)
template <typename T>
static int upload(psba_ctx *h, DevBuf<T> &dst, const std::vector<T> &v) {
  TRY(dst.alloc(h, v.size()));
  if (!v.empty()) PSBA_HIP(h, hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  return PSBA_OK;
}

// the uploaded problem and everything that was set or computed on it goes: buffers, schedules, settings, try state
static void drop_problem(psba_ctx *h) { static_cast<ProblemState &>(*h) = ProblemState{}; }

extern "C" {

const char *psba_version(void) { return "psba_hip 0.1 (gfx950, fp64)"; }

const char *psba_last_error(psba_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

// the handle's stream at the HIGHEST priority: the library's only concurrent work is the far updates of the blocked
// Cholesky chain (lowest priority, kernels_chol_graph.hip), and the main stream's small dependent launches must win a
// freed CU against them (PSBA_STREAM_PRIO_DEFAULT=1: default priority)
static hipError_t create_main_stream(hipStream_t *s) {
  int least = 0, greatest = 0;
  if (getenv("PSBA_STREAM_PRIO_DEFAULT") || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess)
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  return hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest);
}

int psba_create(int device, psba_handle *out) {
  if (!out) return PSBA_E_INVALID;
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(nullptr, PSBA_E_HIP, "no HIP device available (%s); this library has no CPU path",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device < 0 || device >= ndev)
    return fail(nullptr, PSBA_E_INVALID, "device %d out of range (%d devices)", device, ndev);
  psba_ctx *h = new psba_ctx();
  h->device = device;
  if ((e = hipSetDevice(device)) != hipSuccess ||
      (e = create_main_stream(&h->stream)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->scal_event, hipEventDisableTiming)) != hipSuccess) {
    int rc = fail(nullptr, PSBA_E_HIP, "psba_create: %s", hipGetErrorString(e));
    psba_destroy(h);
    return rc;
  }
  if (h->scal.alloc(h, NSCAL) != PSBA_OK || h->h_scal.alloc(h, NSCAL + 8) != PSBA_OK) {  // (+ the publish stamp and check word)
    int rc = fail(nullptr, PSBA_E_HIP, "psba_create: %s", h->err.c_str());
    psba_destroy(h);
    return rc;
  }
  if (hipHostGetDevicePointer((void **)&h->h_scal_dev, h->h_scal, 0) != hipSuccess) h->h_scal_dev = nullptr;
  // the status stamps live in the tail of the scalar block so that one copy fetches both
  h->status = reinterpret_cast<int *>(h->scal + 8);
  h->h_status = reinterpret_cast<int *>(h->h_scal + 8);
  // (on the handle's stream and waited for: hipMemset on the null stream is asynchronous to the host for device
  // memory and a non-blocking stream does not wait for the null stream -- a late memset would wipe the status
  // stamps and the partial sums of a try already running)
  (void)hipMemsetAsync(h->scal, 0, sizeof(double) * NSCAL, h->stream);
  (void)hipStreamSynchronize(h->stream);
  // the publish stamp, the check word and the spare words behind them (psba_backsub_wait): the first stamp waited for
  // is 1.0, and zeros are not the check of any block that carries it
  for (int k = NSCAL; k < NSCAL + 8; k++) h->h_scal[k] = 0.0;
  *out = h;
  return PSBA_OK;
}

int psba_destroy(psba_handle h) {
  CHECK_H(h);
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->stream2) (void)hipStreamSynchronize(h->stream2);
  if (h->comm) ncclCommDestroy(h->comm);
  if (h->k3_event) (void)hipEventDestroy(h->k3_event);
  for (hipEvent_t e : h->chol_events) (void)hipEventDestroy(e);
  if (h->chol_side) {
    (void)hipStreamSynchronize(h->chol_side);
    (void)hipStreamDestroy(h->chol_side);
  }
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  if (h->scal_event) (void)hipEventDestroy(h->scal_event);
  for (auto &s : h->spans) {
    (void)hipEventDestroy(s.a);
    (void)hipEventDestroy(s.b);
  }
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;  // (the problem's buffers, the scalar blocks and the captured graphs go with their owners)
  return PSBA_OK;
}

int psba_schur_path(psba_handle h, int *path) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  if (path) *path = FREE_SPARSE(h) ? 6 : h->cnp != 6 ? 5 : h->solver == PSBA_SOLVER_PCG ? 4 : getenv("PSBA_SCHUR_ATOMIC") ? 2 : h->ring_nWg > 0 ? 3 : h->nGroups > 0 ? 0 : 1;
  return PSBA_OK;
}

int psba_obs_sq_residuals(psba_handle h, int which, double *s) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  NEED(h, h->cnp == 6, "six-parameter camera blocks only (not PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD)");
  if (which != PSBA_PARAMS_CUR && which != PSBA_PARAMS_NEW) return fail(h, PSBA_E_INVALID, "%s: which = %d", __func__, which);
  if (!h->obs_s) TRY(h->obs_s.alloc(h, (size_t)h->d.nO));
  TRY(launch_residual(h, which, nullptr, h->obs_s));
  return d2h(h, s, h->obs_s, sizeof(double) * (size_t)h->d.nO);
}

int psba_camera_block(psba_handle h, int *cnp) {
  CHECK_H(h);
  if (cnp) *cnp = h->cnp;
  return PSBA_OK;
}

int psba_get_dims(psba_handle h, int *nCams, int *n3Dpts, int *n2Dprojs) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  if (nCams) *nCams = h->d.nC;
  if (n3Dpts) *n3Dpts = h->d.nP;
  if (n2Dprojs) *n2Dprojs = h->d.nO;
  return PSBA_OK;
}

// ---- psba_upload_problem, step by step ----------------------------------------------------
namespace {
struct Upload {  // the caller's arrays and what the steps derive from them on the host
  int nC, nP, nO;
  const double *Kparas, *impts, *initrot, *camsEx, *pts3D;
  const int *iidx, *jidx;
  std::vector<int> ptr;       // point CSR over the observations
  std::vector<int> tile_pt;   // first point of each tile of the contiguous partition
  std::vector<int> long_pts;  // points seen by more than TILE_OBS cameras
  int maxTrack = 0;
};
}  // namespace

// arguments and ordering, and the point CSR (replaces generate_idxs).  Nothing of the handle is touched here: a
// rejected upload leaves the old problem usable
static int build_point_csr(psba_ctx *h, Upload &u) {
  if (u.nC <= 0 || u.nP <= 0 || u.nO <= 0 || !u.Kparas || !u.impts || !u.initrot || !u.camsEx || !u.pts3D || !u.iidx ||
      !u.jidx)
    return fail(h, PSBA_E_INVALID, "psba_upload_problem: null pointer or non-positive size");
  // (PSBA_SOLVER_PCG is the mode of the six-parameter blocks; PSBA_SOLVER_SPARSE is stored as it with the flag set)
  const bool pcg6 = h->solver == PSBA_SOLVER_PCG && !h->sparse_any_block;
  if (h->cnp == KD_CNP && (pcg6 || h->nranks > 1 || h->comm))
    return fail(h, PSBA_E_STATE, "PSBA_CAMERA_FREE_KD: dense solver or PSBA_SOLVER_SPARSE, single rank only");
  if (h->cnp != 6 && (pcg6 || h->nranks > 1 || h->comm))
    return fail(h, PSBA_E_INVALID, "free intrinsics: dense solver or PSBA_SOLVER_SPARSE, single rank only");
  u.ptr.assign((size_t)u.nP + 1, 0);
  for (int a = 0; a < u.nO; a++) {
    const int i = u.iidx[a], j = u.jidx[a];
    if (i < 0 || i >= u.nP || j < 0 || j >= u.nC)
      return fail(h, PSBA_E_INVALID, "observation %d: point %d / camera %d out of range", a, i, j);
    if (a > 0 && (i < u.iidx[a - 1] || (i == u.iidx[a - 1] && j <= u.jidx[a - 1])))
      return fail(h, PSBA_E_INVALID,
                  "observations must be sorted point-major with ascending, distinct cameras "
                  "inside a point (violated at observation %d)", a);
    u.ptr[(size_t)i + 1]++;
  }
  for (int i = 0; i < u.nP; i++) {
    if (u.ptr[(size_t)i + 1] > u.maxTrack) u.maxTrack = u.ptr[(size_t)i + 1];
    u.ptr[(size_t)i + 1] += u.ptr[i];
  }
  return PSBA_OK;
}

// point-aligned tiles of at most TILE_OBS observations / TILE_PTS points.  A point seen by more
// cameras than a tile holds (the reference has no such limit: CL_files/compute_V.cl:6-38 loops
// over all cameras) is a tile of its own that the tile kernels skip; one workgroup per such point
// walks its observations in the *_long kernels instead.
static void cut_tiles(Upload &u) {
  const std::vector<int> &ptr = u.ptr;
  u.tile_pt.push_back(0);
  for (int p0 = 0; p0 < u.nP;) {
    int p1 = p0;
    if (ptr[(size_t)p0 + 1] - ptr[p0] > TILE_OBS) {
      u.long_pts.push_back(p0);
      p1 = p0 + 1;
    } else {
      while (p1 < u.nP && (ptr[(size_t)p1 + 1] - ptr[p0]) <= TILE_OBS && (p1 - p0) < TILE_PTS) p1++;
    }
    u.tile_pt.push_back(p1);
    p0 = p1;
  }
}

// the sizes everything else is cut to, and which form K1's camera sums take
static void set_dims(psba_ctx *h, const Upload &u) {
  const int cnp = h->cnp;  // 6, 11 with free intrinsics or 16 with distortion too (both kernels_free.hip)
  Dims d;
  d.nC = u.nC;
  d.nP = u.nP;
  d.nO = u.nO;
  d.nA = cnp * u.nC;
  d.nB = 3 * u.nP;
  d.nT = d.nA + d.nB;
  d.nTilesAll = (int)u.tile_pt.size() - 1;
  d.nTiles = d.nTilesAll - (int)u.long_pts.size();  // the tile kernels never see a long point's tile
  if (d.nTiles < 1) d.nTiles = 1;                   // (only long points: one empty tile keeps the grids non-empty)
  d.maxTrack = u.maxTrack;
  h->d = d;
  h->nLong = (int)u.long_pts.size();
  // K1's 27 sums per camera: LDS accumulators per workgroup while they leave room for three
  // workgroups per CU (up to ~220 cameras: 31 ... 36 us for K1 at 218 k observations), the
  // camera-major pass beyond (~40 us flat; the LDS form takes 55 us at 257 cameras and 64 at 455,
  // where it ends: PSBA_LIN_LDS_ACC=1 keeps it up to there)
  const size_t cam_lds_max = getenv("PSBA_LIN_LDS_ACC") ? 96 * 1024 : 48 * 1024;
  h->cam_global = cnp == 6 && ((size_t)CAM_ACC * u.nC * sizeof(double) > cam_lds_max || getenv("PSBA_LIN_GLOBAL_ACC"));
  h->nPart = d.nTiles < 768 ? d.nTiles : 768;  // persistent workgroups: three per CU fit since W is staged in halves
  if (const char *e = getenv("PSBA_LIN_GRID")) h->nPart = atoi(e) > 0 && atoi(e) < d.nTiles ? atoi(e) : d.nTiles;
  h->n32 = (d.nA + 31) / 32 * 32;
}

// everything the kernels write: parameters, both sets of linearization outputs, camera sums, S and its factor
static int alloc_work_buffers(psba_ctx *h) {
  const Dims &d = h->d;
  const int cnp = h->cnp;
  TRY(h->cams[0].alloc(h, (size_t)d.nA));
  TRY(h->cams[1].alloc(h, (size_t)d.nA));
  TRY(h->pts[0].alloc(h, (size_t)d.nB));
  TRY(h->pts[1].alloc(h, (size_t)d.nB));
  TRY(h->params0.alloc(h, (size_t)d.nT));
  TRY(h->impts.alloc(h, (size_t)2 * d.nO));
  TRY(h->iidx.alloc(h, (size_t)d.nO));
  TRY(h->jidx.alloc(h, (size_t)d.nO));
  TRY(h->W.alloc(h, (size_t)3 * cnp * d.nO));
  TRY(h->W_alt.alloc(h, (size_t)3 * cnp * d.nO));
  TRY(h->PV.alloc(h, (size_t)9 * d.nP));
  TRY(h->PV_alt.alloc(h, (size_t)9 * d.nP));
  // (a point without observations is never written by K1, whose stores come from the last lane of a point's run
  // of observations: its V_i and g_b,i are the zeros put here)
  PSBA_HIP(h, hipMemsetAsync(h->PV, 0, sizeof(double) * 9 * (size_t)d.nP, h->stream));
  PSBA_HIP(h, hipMemsetAsync(h->PV_alt, 0, sizeof(double) * 9 * (size_t)d.nP, h->stream));
  TRY(h->U.alloc(h, (size_t)cnp * cnp * d.nC));
  TRY(h->U_alt.alloc(h, (size_t)cnp * cnp * d.nC));
  TRY(h->ga.alloc(h, (size_t)d.nA));
  TRY(h->ga_alt.alloc(h, (size_t)d.nA));
  TRY(h->campart.alloc(h, (h->cam_global || cnp != 6) ? 1 : (size_t)(h->nPart + 1) * d.nC * CAM_ACC));  // (+1: the long points' slab)
  if (cnp != 6) {  // kernels_free.hip (the per-unit buffers: upload_camera_index)
    TRY(h->free_Be.alloc(h, (size_t)8 * d.nO));
    TRY(h->free_Y.alloc(h, (size_t)3 * cnp * d.nO));
    TRY(h->free_red.alloc(h, (size_t)KD_RED));
  }
  if (h->cam_global) TRY(h->camacc.alloc(h, (size_t)d.nC * CAM_ACC));
  // rows [0, n32 + 16) are the reduce buffer proper; n32 more rows below it are the working
  // space of the identity rows the panel chain carries along (kernels_chol_graph.hip)
  // (PSBA_SOLVER_PCG: no dense S, no factor -- only the blocks that exist, plan_schur_sparse)
  const size_t dense = h->solver == PSBA_SOLVER_PCG ? 1 : (size_t)(2 * h->n32 + 16) * h->n32;
  TRY(h->red.alloc(h, dense));
  PSBA_HIP(h, hipMemsetAsync(h->red, 0, sizeof(double) * dense, h->stream));
  TRY(h->dp.alloc(h, (size_t)(d.nT > 36 * d.nC ? d.nT : 36 * d.nC)));
  PSBA_HIP(h, hipMemsetAsync(h->dp, 0, sizeof(double) * d.nT, h->stream));
  TRY(h->chol_ws.alloc(h, (size_t)((d.nA + 31) / 32) * 1024));
  TRY(h->chol_L.alloc(h, dense));
  PSBA_HIP(h, hipMemsetAsync(h->chol_L, 0, sizeof(double) * dense, h->stream));
  if (getenv("PSBA_CHOL_TIMING")) TRY(h->chol_tim.alloc(h, 32));  // [0..15] diag kernel + pivot wave, [16..31] inverse wave
  return PSBA_OK;
}

// camera-major index of the observations, cut into segments of at most 256 (K1's camera sums with many cameras) or
// KD_UNIT (free intrinsics: one observation per lane of a wave, and the units of each camera by free_cuptr)
static int upload_camera_index(psba_ctx *h, const Upload &u) {
  const int cnp = h->cnp;
  const bool kd = cnp != 6;
  std::vector<int> cptr((size_t)u.nC + 1, 0), cobs((size_t)u.nO);
  for (int a = 0; a < u.nO; a++) cptr[(size_t)u.jidx[a] + 1]++;
  for (int j = 0; j < u.nC; j++) cptr[(size_t)j + 1] += cptr[j];
  {
    std::vector<int> at(cptr.begin(), cptr.end() - 1);
    for (int a = 0; a < u.nO; a++) cobs[(size_t)at[u.jidx[a]]++] = a;
  }
  std::vector<int4> units;
  const int LSEG = kd ? KD_UNIT : 256;
  std::vector<int> cuptr((size_t)u.nC + 1, 0);
  for (int j = 0; j < u.nC; j++) {
    for (int f = cptr[j]; f < cptr[(size_t)j + 1]; f += LSEG)
      units.push_back(make_int4(j, f, std::min(f + LSEG, cptr[(size_t)j + 1]), 0));
    cuptr[(size_t)j + 1] = (int)units.size();
  }
  h->nCamUnits = (int)units.size();
  if (kd) {
    TRY(upload(h, h->free_cuptr, cuptr));
    TRY(h->free_upart.alloc(h, (size_t)(cnp * cnp + cnp) * units.size()));
    TRY(h->free_eapart.alloc(h, (size_t)cnp * units.size()));
  }
  TRY(upload(h, h->cam_obs, cobs));
  return upload(h, h->cam_units, units);
}

// ---- K2's static schedule: one of the routes below per problem (psba_schur_path) ----

// the owner route's product lists (many cameras; with PSBA_SOLVER_PCG they also give the blocks that exist)
static int upload_owner_plan(psba_ctx *h, const OwnerPlanHost &op) {
  TRY(upload(h, h->own_prod, op.prod));
  TRY(upload(h, h->own_waves, op.waves));
  TRY(upload(h, h->own_units, op.units));
  h->own_nwaves = (int)op.waves.size();
  h->own_products = op.products;
  return PSBA_OK;
}

// sharded points: every rank must hold the same block list, the union of what the ranks' points
// produce -- one byte per block of the lower triangle, combined with a max all-reduce over the
// communicator, or handed in by a host that has its own transport (psba_set_sparse_pattern).
// pat stays empty where this rank's own blocks are the list
static int shared_block_pattern(psba_ctx *h, const Upload &u, std::vector<unsigned char> &pat) {
  // (PSBA_SPARSE_PATTERN_FORCE=1: test hook -- a one-rank communicator exchanges its pattern too)
  if (!(h->nranks > 1 || (h->comm && getenv("PSBA_SPARSE_PATTERN_FORCE")))) return PSBA_OK;
  const size_t nBlk = (size_t)u.nC * (u.nC + 1) / 2;
  if (!h->comm) {
    if (h->bs_pattern.size() != nBlk)
      return fail(h, PSBA_E_STATE, "PSBA_SOLVER_PCG with a rank layout and no communicator: psba_set_sparse_pattern "
                                   "(the union of psba_sparse_pattern over the ranks) before psba_upload_problem");
    pat = h->bs_pattern;
    return PSBA_OK;
  }
  pat.resize(nBlk);
  TRY(sparse_pattern(u.nC, u.nO, u.iidx, u.jidx, u.ptr.data(), pat.data()));
  DevBuf<unsigned char> dev;
  TRY(dev.alloc(h, nBlk));
  PSBA_HIP(h, hipMemcpyAsync(dev, pat.data(), nBlk, hipMemcpyHostToDevice, h->stream));
  RCCL(h, ncclAllReduce(dev, dev, nBlk, ncclUint8, ncclMax, h->comm, h->stream));
  PSBA_HIP(h, hipMemcpyAsync(pat.data(), dev, nBlk, hipMemcpyDeviceToHost, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  return PSBA_OK;
}

// the symmetric pattern by block row (kernels_pcg.hip, k_pcg_spmv)
static int upload_bsr_rows(psba_ctx *h, const OwnerPlanHost &op) {
  const int nC = h->d.nC;
  std::vector<int> rp((size_t)nC + 1, 0);
  for (const int2 &b : op.blocks) {
    rp[(size_t)b.x + 1]++;
    if (b.x != b.y) rp[(size_t)b.y + 1]++;
  }
  for (int j = 0; j < nC; j++) rp[(size_t)j + 1] += rp[(size_t)j];
  std::vector<int2> ent((size_t)rp[(size_t)nC]);
  std::vector<int> at(rp.begin(), rp.end() - 1);
  for (size_t sl = 0; sl < op.blocks.size(); sl++) {
    const int2 b = op.blocks[sl];
    if (b.x == b.y) {
      ent[(size_t)at[(size_t)b.x]++] = make_int2((int)sl, b.x | (2 << 28));
    } else {
      ent[(size_t)at[(size_t)b.x]++] = make_int2((int)sl, b.y);
      ent[(size_t)at[(size_t)b.y]++] = make_int2((int)sl, b.x | (1 << 28));
    }
  }
  TRY(upload(h, h->bs_rowptr, rp));
  return upload(h, h->bs_rowent, ent);
}

// block-sparse S (PSBA_SOLVER_PCG): the owner route's product lists give the blocks that exist
static int plan_schur_sparse(psba_ctx *h, const Upload &u) {
  const Dims &d = h->d;
  std::vector<unsigned char> pat;
  TRY(shared_block_pattern(h, u, pat));
  OwnerPlanHost op;
  TRY(build_owner_plan(u.nC, u.nO, u.iidx, u.jidx, u.ptr.data(), op, pat.empty() ? nullptr : pat.data()));
  h->packedN = 36 * (size_t)u.nC * (u.nC + 1) / 2;
  TRY(upload_owner_plan(h, op));
  h->bs_nblk = (long long)op.blocks.size();
  TRY(h->bs_val.alloc(h, (size_t)36 * op.blocks.size() + (size_t)d.nA));
  h->bs_ea = h->bs_val + (size_t)36 * op.blocks.size();
  TRY(upload(h, h->bs_jk, op.blocks));
  TRY(upload(h, h->bs_diag, op.diag_slot));
  TRY(upload_bsr_rows(h, op));
  TRY(h->pcg_vec.alloc(h, (size_t)5 * d.nA));  // r, z, p, q, and r's second buffer
  TRY(h->pcg_minv.alloc(h, (size_t)36 * d.nC));
  TRY(h->pcg_scal.alloc(h, (size_t)(16 + 4 * 64)));  // scalars + the partial sums of p.Sp (kernels_pcg.hip)
  if (!h->pcg_host) TRY(h->pcg_host.alloc(h, 16));
  if (getenv("PSBA_SCHUR_PLAN_INFO"))
    fprintf(stderr, "[psba] block-sparse S: %lld of %lld blocks of the lower block triangle (%.1f %%), %lld products\n",
            h->bs_nblk, (long long)u.nC * (u.nC + 1) / 2, 100.0 * (double)h->bs_nblk / ((double)u.nC * (u.nC + 1) / 2),
            op.products);
  return PSBA_OK;
}

#ifdef PSBA_BUILD_EXPERIMENTS
// the ring route (few cameras): taken where build_ring_plan finds it worth it (ring_nWg > 0 afterwards)
static int plan_schur_ring(psba_ctx *h, const Upload &u) {
  RingPlanHost rp;
  TRY(build_ring_plan(u.nC, u.nP, u.nO, u.iidx, u.jidx, u.ptr.data(), rp));
  if (rp.nWg <= 0) return PSBA_OK;
  h->packedN = 36 * (size_t)u.nC * (u.nC + 1) / 2;
  h->ring_nWg = rp.nWg;
  h->ring_nS = rp.nS;
  h->ring_products = rp.products;
  h->ring_slots = rp.slots;
  h->ring_loaded_recs = (size_t)rp.loaded_recs;
  std::vector<int> canon;
  for (int j = 0; j < u.nC; j++)
    for (int k = 0; k <= j; k++) canon.push_back((j << 16) | k);
  TRY(upload(h, h->ring_wg, rp.wgs));
  TRY(upload(h, h->ring_steps, rp.steps));
  TRY(upload(h, h->ring_entries, rp.entries));
  TRY(upload(h, h->ring_ops, rp.ops));
  TRY(upload(h, h->ring_jobs, rp.jobs));
  TRY(upload(h, h->ring_bl0, rp.blk_lane0));
  TRY(upload(h, h->ring_canon, canon));
  TRY(h->ring_slab.alloc(h, (size_t)rp.nS * h->packedN));
  TRY(h->ring_pvi.alloc(h, (size_t)9 * u.nP + 2));
  h->packed_doubles = h->packedN;
  TRY(h->redp.alloc(h, h->packed_doubles));
  if (getenv("PSBA_SCHUR_PLAN_INFO")) {
    long long steps_max = 0;
    for (const auto &w : rp.wgs) steps_max = w.nsteps > steps_max ? w.nsteps : steps_max;
    fprintf(stderr, "[psba] K2 ring route: %d block ranges x %d stretches, %lld products in %lld lane-steps (fill %.3f), "
                    "%lld record loads (%.2f per observation), %zu jobs, steps <= %lld, lists %.1f MB, copies %.1f MB\n",
            rp.nR, rp.nS, rp.products, rp.slots, rp.slots ? (double)rp.products / (double)rp.slots : 1.0,
            rp.loaded_recs, (double)rp.loaded_recs / u.nO, rp.jobs.size(), steps_max,
            1e-6 * (4.0 * rp.entries.size() + 4.0 * rp.ops.size() + 16.0 * rp.jobs.size() + 16.0 * rp.steps.size()),
            8e-6 * (double)rp.nS * (double)h->packedN);
  }
  return PSBA_OK;
}
#endif

// the LDS route (groups of blocks, workgroups, conflict-free item rows), or, where build_schur_plan finds no
// partition of S that fits (nGroups = 0: many cameras), the owner route
static int plan_schur_lds(psba_ctx *h, const Upload &u) {
  SchurPlanHost plan;
  TRY(build_schur_plan(h, u.nC, u.nP, u.nO, u.iidx, u.jidx, u.ptr.data(), plan));
  if (!h->nGroups) {
    // many cameras: the owner route (one thread per block segment, sums in registers)
    OwnerPlanHost op;
    TRY(build_owner_plan(u.nC, u.nO, u.iidx, u.jidx, u.ptr.data(), op));
    TRY(upload_owner_plan(h, op));
    if (getenv("PSBA_SCHUR_PLAN_INFO"))
      // no silent cliff: say which route K2 takes (psba_schur_path returns the same)
      fprintf(stderr, "[psba] K2 owner route (%d cameras): %lld products in %zu ELL slots (fill %.3f), %d waves\n",
              u.nC, op.products, op.prod.size(), (double)op.products / (double)op.prod.size(), h->own_nwaves);
    return PSBA_OK;
  }
  h->schur_runs = plan.runs;
  h->schur_pairs = plan.pair_items > 0;
  TRY(upload(h, h->items, plan.items));
  TRY(upload(h, h->wg, plan.wgs));
  TRY(upload(h, h->posblock, plan.posblock));
  TRY(h->slab.alloc(h, plan.slab_doubles));
  for (int j = 0, b = 0; j < 6; j++)
    for (int k = 0; k <= j; k++, b++) {
      h->h_diagpos[b] = j < u.nC ? plan.blockpos[(size_t)b] : 0;
      int g = -1;
      if (j < u.nC)
        for (g = 0; b >= h->gblk0[g + 1];) g++;
      h->h_diaggrp[b] = g;
    }
  std::vector<ReduceGroup> tab;
  long long pos0 = 0;
  for (int g = 0; g < h->nGroups; g++) {
    tab.insert(tab.end(), (size_t)h->gnblk[g] / 16, ReduceGroup{h->gnwg[g], h->gnblk[g], pos0, h->gslab[g], 0});
    pos0 += h->gnblk[g];
  }
  TRY(upload(h, h->gtab, tab));
  h->packed_doubles = h->packedN;  // 36 doubles per block of the lower block triangle, canonical order
  TRY(h->redp.alloc(h, h->packed_doubles));
  TRY(h->diag0.alloc(h, (size_t)21 * 36));
  PSBA_HIP(h, hipMemsetAsync(h->diag0, 0, sizeof(double) * 21 * 36, h->stream));
  if (getenv("PSBA_SCHUR_PLAN_INFO"))
    fprintf(stderr, "[psba] K2 plan%s: %d groups, %d workgroups, %lld products in %zu item slots (fill %.3f), slabs %.1f MB\n",
            plan.runs ? " (runs layout)" : "", h->nGroups, h->nWg, plan.real_items, plan.items.size(),
            plan.items.size() ? (double)plan.real_items / (double)plan.items.size() : 1.0,
            8e-6 * (double)plan.slab_doubles);
  return PSBA_OK;
}

// free intrinsics: products sorted by block, cut into segments (blockprod_plan.cpp); PSBA_FKD_SEG=n sets the
// segment length for tests and sweeps
static int plan_schur_blockprod(psba_ctx *h, const Upload &u) {
  int seg = KD_SEG_DEFAULT;
  if (const char *e = getenv("PSBA_FKD_SEG"))
    if (atoi(e) > 0) seg = atoi(e);
  BlockProdPlanHost plan;
  if (build_blockprod_plan(u.nC, u.nO, u.iidx, u.jidx, u.ptr.data(), seg, plan) != PSBA_OK)
    return fail(h, PSBA_E_INVALID, "%s: more than 2^31 products Y_a W_b^T", h->cnp == KD_CNP ? "PSBA_CAMERA_FREE_KD" : "PSBA_CAMERA_FREE_K");
  TRY(upload(h, h->free_blocks, plan.blocks));
  TRY(upload(h, h->free_segs, plan.segs));
  TRY(upload(h, h->free_prods, plan.prods));
  if (!plan.multi.empty()) TRY(upload(h, h->free_multi, plan.multi));
  TRY(h->free_tiles.alloc(h, (size_t)h->cnp * h->cnp * (plan.ntiles ? plan.ntiles : 1)));
  h->free_nsegs = (int)plan.segs.size();
  h->free_nmulti = (int)plan.multi.size();
  return PSBA_OK;
}

// PSBA_SOLVER_SPARSE on these blocks: the same plan, with the tables of the two assembly kernels carrying the slot of the
// stored block in place of (j, k); the stored list, its row walk and the buffers of the conjugate gradients
// (kernels_free_pcg.hip).  Nothing here is of size nA^2
static int plan_schur_blockprod_sparse(psba_ctx *h, const Upload &u) {
  const Dims &d = h->d;
  const size_t c2 = (size_t)h->cnp * h->cnp;
  int seg = KD_SEG_DEFAULT;
  if (const char *e = getenv("PSBA_FKD_SEG"))
    if (atoi(e) > 0) seg = atoi(e);
  BlockProdPlanHost plan;
  if (build_blockprod_plan(u.nC, u.nO, u.iidx, u.jidx, u.ptr.data(), seg, plan) != PSBA_OK)
    return fail(h, PSBA_E_INVALID, "%s: more than 2^31 products Y_a W_b^T", h->cnp == KD_CNP ? "PSBA_CAMERA_FREE_KD" : "PSBA_CAMERA_FREE_K");
  BlockRowsHost rows;
  build_block_rows(u.nC, plan, rows);
  std::vector<int2> slots(plan.blocks.size());
  for (size_t b = 0; b < plan.blocks.size(); b++) slots[b] = make_int2(rows.slot_of[b], 0);
  std::vector<int4> multi(plan.multi);
  {
    size_t b = 0;  // (multi follows the order of blocks)
    for (int4 &m : multi) {
      while (plan.blocks[b].x != m.x || plan.blocks[b].y != m.y) b++;
      m.x = rows.slot_of[b];
      m.y = 0;
    }
  }
  TRY(upload(h, h->free_blocks, slots));
  TRY(upload(h, h->free_segs, plan.segs));
  TRY(upload(h, h->free_prods, plan.prods));
  if (!multi.empty()) TRY(upload(h, h->free_multi, multi));
  TRY(h->free_tiles.alloc(h, c2 * (plan.ntiles ? plan.ntiles : 1)));
  h->free_nsegs = (int)plan.segs.size();
  h->free_nmulti = (int)multi.size();
  h->bs_nblk = (long long)rows.jk.size();
  TRY(h->bs_val.alloc(h, c2 * rows.jk.size() + (size_t)d.nA));
  h->bs_ea = h->bs_val + c2 * rows.jk.size();
  TRY(upload(h, h->bs_jk, rows.jk));
  std::vector<int> diag(rows.diag_slot);
  for (int j = 0; j < u.nC; j++)
    if (rows.added[(size_t)j]) diag[(size_t)j] |= FBSR_ADDED;
  TRY(upload(h, h->bs_diag, diag));
  TRY(upload(h, h->bs_rowptr, rows.rowptr));
  TRY(upload(h, h->bs_rowent, rows.rowent));
  TRY(h->pcg_vec.alloc(h, (size_t)5 * d.nA));  // r, z, p, q, and r's second buffer
  TRY(h->pcg_minv.alloc(h, c2 * d.nC));
  TRY(h->pcg_scal.alloc(h, (size_t)(16 + 13 * FPCG_CAP)));  // scalars + the partial sums (kernels_free_pcg.hip)
  if (!h->pcg_host) TRY(h->pcg_host.alloc(h, 16));
  if (getenv("PSBA_SCHUR_PLAN_INFO"))
    fprintf(stderr, "[psba] block-sparse S, blocks of %d: %lld of %lld blocks of the lower block triangle, %lld diagonal blocks added\n",
            h->cnp, h->bs_nblk, (long long)u.nC * (u.nC + 1) / 2, rows.nadded);
  return PSBA_OK;
}

static int plan_schur(psba_ctx *h, const Upload &u) {
  if (h->solver == PSBA_SOLVER_PCG) return h->cnp != 6 ? plan_schur_blockprod_sparse(h, u) : plan_schur_sparse(h, u);
#ifdef PSBA_BUILD_EXPERIMENTS
  TRY(plan_schur_ring(h, u));
  if (h->ring_nWg) return PSBA_OK;
#endif
  if (h->cnp != 6) return plan_schur_blockprod(h, u);
  return plan_schur_lds(h, u);
}

// the caller's arrays and the index tables derived from them, to the device
static int copy_inputs(psba_ctx *h, const Upload &u) {
  const Dims &d = h->d;
  std::vector<double> cc((size_t)u.nC * 9);
  for (int j = 0; j < u.nC; j++) {
    for (int k = 0; k < 5; k++) cc[(size_t)9 * j + k] = u.Kparas[5 * j + k];
    for (int k = 0; k < 4; k++) cc[(size_t)9 * j + 5 + k] = u.initrot[4 * j + k];
  }
  TRY(upload(h, h->camconst, cc));
  TRY(upload(h, h->ptr, u.ptr));
  TRY(upload(h, h->tile_pt, u.tile_pt));
  if (h->nLong) TRY(upload(h, h->long_pts, u.long_pts));
  std::vector<int4> tile_desc;
  for (int t = 0; t < d.nTilesAll; t++)
    if (u.ptr[u.tile_pt[t + 1]] - u.ptr[u.tile_pt[t]] <= TILE_OBS)
      tile_desc.push_back(make_int4(u.tile_pt[t], u.tile_pt[t + 1], u.ptr[u.tile_pt[t]], u.ptr[u.tile_pt[t + 1]]));
  if (tile_desc.empty()) tile_desc.push_back(make_int4(0, 0, 0, 0));  // (only long points: an empty tile keeps the grids non-empty)
  TRY(upload(h, h->tile_desc, tile_desc));
  const double *cams = u.camsEx;
  std::vector<double> cam11;  // free intrinsics: the camera block is (K | [kc = 0: psba_set_distortion] | local rotation | translation)
  if (h->cnp != 6) {
    cam11.assign((size_t)d.nA, 0.0);
    for (int j = 0; j < u.nC; j++) {
      for (int k = 0; k < 5; k++) cam11[(size_t)h->cnp * j + k] = u.Kparas[5 * j + k];
      for (int k = 0; k < 6; k++) cam11[(size_t)h->cnp * j + h->cnp - 6 + k] = u.camsEx[6 * j + k];
    }
    cams = cam11.data();
  }
  auto H2D = [&](void *dst, const void *src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream);
  };
  PSBA_HIP(h, H2D(h->cams[0], cams, sizeof(double) * d.nA));
  PSBA_HIP(h, H2D(h->pts[0], u.pts3D, sizeof(double) * d.nB));
  PSBA_HIP(h, H2D(h->params0, cams, sizeof(double) * d.nA));
  PSBA_HIP(h, H2D(h->params0 + d.nA, u.pts3D, sizeof(double) * d.nB));
  PSBA_HIP(h, H2D(h->impts, u.impts, sizeof(double) * 2 * (size_t)d.nO));
  PSBA_HIP(h, H2D(h->iidx, u.iidx, sizeof(int) * (size_t)d.nO));
  PSBA_HIP(h, H2D(h->jidx, u.jidx, sizeof(int) * (size_t)d.nO));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));  // host vectors go out of scope
  return PSBA_OK;
}

int psba_upload_problem(psba_handle h, int nCams, int n3Dpts, int n2Dprojs, const double *Kparas,
                        const double *impts, const double *initrot, const double *camsEx,
                        const double *pts3D, const int *iidx, const int *jidx) {
  CHECK_H(h);
  Upload u{nCams, n3Dpts, n2Dprojs, Kparas, impts, initrot, camsEx, pts3D, iidx, jidx};
  TRY(build_point_csr(h, u));
  cut_tiles(u);
  PSBA_HIP(h, hipSetDevice(h->device));
  drop_problem(h);  // from here on the handle holds no problem until this upload has succeeded
  set_dims(h, u);
  TRY(alloc_work_buffers(h));
  if (h->cam_global || h->cnp != 6) TRY(upload_camera_index(h, u));
  TRY(plan_schur(h, u));
  // the lean form of psba_levmar's look-ahead linearizations: what the problem's shape and the switch
  // PSBA_LEAN_LIN=0 decide is decided here; lean_eligible() adds what can change after the upload, and the record
  // buffers come with the first psba_levmar that can use them (lean_prepare)
  h->lean_ok = h->cnp == 6 && h->solver != PSBA_SOLVER_PCG && h->nGroups > 0 && h->ring_nWg == 0 && !h->schur_runs &&
               !h->schur_pairs && !h->cam_global && h->nLong == 0;
  if (const char *e = getenv("PSBA_LEAN_LIN")) h->lean_ok = h->lean_ok && atoi(e) != 0;
  TRY(copy_inputs(h, u));
  // the blocking copies went through the null stream, which this handle's non-blocking stream does not wait for:
  // everything on the device is done before the first kernel can be queued
  PSBA_HIP(h, hipDeviceSynchronize());
  h->uploaded = true;
  return PSBA_OK;
}

// psba_set_params and psba_reset_params may run while a try is in flight, where the setters refuse: they replace the
// parameters the try was made for, so the try is given up as a whole and nothing waits for its scalars any more
static void abandon_try(psba_ctx *h) { h->backsub_pending = h->publish_deferred = h->publish_in_k1 = false; }

int psba_set_params(psba_handle h, const double *camsEx, const double *pts3D) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  if (!h->kd_rep_h.empty()) TRY(groups_split(h, "psba_set_params", h->kd_rep_h, camsEx, KD_CNP, 10, 0));
  PSBA_HIP(h, hipMemcpyAsync(h->cams[h->cur], camsEx, sizeof(double) * h->d.nA,
                             hipMemcpyHostToDevice, h->stream));
  PSBA_HIP(h, hipMemcpyAsync(h->pts[h->cur], pts3D, sizeof(double) * h->d.nB,
                             hipMemcpyHostToDevice, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  params_changed(h);
  abandon_try(h);
  return PSBA_OK;
}

int psba_reset_params(psba_handle h) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  PSBA_HIP(h, hipMemcpyAsync(h->cams[h->cur], h->params0, sizeof(double) * h->d.nA, hipMemcpyDeviceToDevice,
                             h->stream));
  PSBA_HIP(h, hipMemcpyAsync(h->pts[h->cur], h->params0 + h->d.nA, sizeof(double) * h->d.nB,
                             hipMemcpyDeviceToDevice, h->stream));
  params_changed(h);
  abandon_try(h);
  return PSBA_OK;
}

int psba_get_params(psba_handle h, int which, double *camsEx, double *pts3D) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  const int set = which == PSBA_PARAMS_NEW ? 1 - h->cur : h->cur;
  if (camsEx)
    PSBA_HIP(h, hipMemcpyAsync(camsEx, h->cams[set], sizeof(double) * h->d.nA,
                               hipMemcpyDeviceToHost, h->stream));
  if (pts3D)
    PSBA_HIP(h, hipMemcpyAsync(pts3D, h->pts[set], sizeof(double) * h->d.nB,
                               hipMemcpyDeviceToHost, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  return PSBA_OK;
}

// ---- fused verbs ------------------------------------------------------------------------

static int fetch_scalars(psba_ctx *h) {
  PSBA_HIP(h, hipMemcpyAsync(h->h_scal, h->scal, sizeof(double) * NSCAL, hipMemcpyDeviceToHost,
                             h->stream));  // scalars and the status stamps (tail of the block)
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  return PSBA_OK;
}

static int enqueue_residual(psba_ctx *h, int which) {
  TRY(launch_residual(h, which, nullptr));
  if (h->comm)
    RCCL(h, ncclAllReduce(h->scal + SC_COST, h->scal + SC_COST, 1, ncclDouble, ncclSum, h->comm,
                          h->stream));
  return PSBA_OK;
}

int psba_residual(psba_handle h, int which, double *cost) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  TRY(enqueue_residual(h, which));
  TRY(fetch_scalars(h));
  if (cost) *cost = h->h_scal[SC_COST];
  return PSBA_OK;
}

int psba_linearize(psba_handle h, double coeff, double coeff_g) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  // nothing to do when psba_linearize_ahead already produced exactly this linearization
  if (!(h->lin_is_ahead && coeff == h->coeff && coeff_g == h->coeff_g)) {
    h->coeff = coeff;
    h->coeff_g = coeff_g;
    TRY(launch_linearize(h, false));
    h->free_obs = h->cnp != 6;
    h->damp_ok = h->damp_kind == PSBA_DAMPING_MARQUARDT;
  }
  h->lin_is_ahead = false;
  h->ahead = false;
  h->linearized = true;
  h->assembled = h->solved = h->backsubbed = false;
  return PSBA_OK;
}

static int enqueue_max_diag(psba_ctx *h) {
  if (h->comm) {
    // diag(U) is a sum over all points: reduce the per-rank U first (scratch copy in dp)
    double *tmp = h->dp;  // dp is free between linearize and the first solve
    PSBA_HIP(h, hipMemcpyAsync(tmp, h->U, sizeof(double) * 36 * h->d.nC, hipMemcpyDeviceToDevice,
                               h->stream));
    RCCL(h, ncclAllReduce(tmp, tmp, (size_t)36 * h->d.nC, ncclDouble, ncclSum, h->comm, h->stream));
    std::swap(h->U, h->dp);  // (the launcher reads h->U)
    int rc = launch_max_diag(h);
    std::swap(h->U, h->dp);
    TRY(rc);
    RCCL(h, ncclAllReduce(h->scal + SC_MAXDIAG, h->scal + SC_MAXDIAG, 1, ncclDouble, ncclMax,
                          h->comm, h->stream));
  } else {
    TRY(launch_max_diag(h));
  }
  return PSBA_OK;
}

int psba_begin(psba_handle h, double coeff, double coeff_g, double *cost, double *max_diag) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  TRY(enqueue_residual(h, PSBA_PARAMS_CUR));
  h->coeff = coeff;
  h->coeff_g = coeff_g;
  TRY(launch_linearize(h, false));
  h->free_obs = h->cnp != 6;
  h->damp_ok = h->damp_kind == PSBA_DAMPING_MARQUARDT;
  h->linearized = true;
  h->assembled = h->solved = h->backsubbed = false;
  h->ahead = false;
  TRY(enqueue_max_diag(h));
  TRY(fetch_scalars(h));
  if (cost) *cost = h->h_scal[SC_COST];
  if (max_diag) *max_diag = h->h_scal[SC_MAXDIAG];
  h->lin_is_ahead = true;  // the next psba_linearize with these coefficients has nothing left to do
  return PSBA_OK;
}

int psba_max_diag(psba_handle h, double *out) {
  CHECK_H(h);
  NEED(h, h->linearized, "psba_linearize first");
  TRY(enqueue_max_diag(h));
  TRY(fetch_scalars(h));
  if (out) *out = h->h_scal[SC_MAXDIAG];
  return PSBA_OK;
}

int psba_schur_assemble(psba_handle h, double mu) {
  CHECK_H(h);
  NEED(h, h->linearized, "psba_linearize first");
  h->mu = mu;
  // every camera fixed: no coupled system.  dpa = 0 and K3's point part is the whole solve, so K2, the S-reduce and the
  // factorization are not queued at all (PSBA_FIXED_NO_SHORTCUT=1: the general route, for the test that compares them)
  h->try_shortcut = h->struct_only && h->cnp == 6 && !getenv("PSBA_FIXED_NO_SHORTCUT");
  h->cholmod_factor = false;  // the S-reduce kernel may factor the first diagonal block into chol_L
  if (h->try_shortcut)
    TRY(launch_struct_only_try(h, mu));
  else
    TRY(launch_schur(h, mu, false));
  h->assembled = true;
  h->solved = h->backsubbed = false;
  h->precond_ok = false;
  return PSBA_OK;
}

// the per-try collective: [tril(S) || e_a] in slab order when the LDS schedule produced it
// (about half the bytes of the padded square), then scattered into the padded buffer; the whole
// padded square for the global-atomic fallback kernel
static int allreduce_schur(psba_ctx *h) {
  if (h->solver == PSBA_SOLVER_PCG) {  // the blocks that exist and e_a behind them: one collective
    if (h->comm)
      RCCL(h, ncclAllReduce(h->bs_val, h->bs_val, (size_t)36 * h->bs_nblk + h->d.nA, ncclDouble, ncclSum, h->comm, h->stream));
    return PSBA_OK;
  }
  if (h->packed_pending) {
    if (h->comm)
      RCCL(h, ncclAllReduce(h->redp, h->redp, h->packed_doubles, ncclDouble, ncclSum, h->comm, h->stream));
    TRY(launch_schur_expand(h));
    h->packed_pending = false;
  } else if (h->comm) {
    const size_t n = (size_t)(h->n32 + 1) * h->n32;  // S rows, padding rows and the ea row
    RCCL(h, ncclAllReduce(h->red, h->red, n, ncclDouble, ncclSum, h->comm, h->stream));
  }
  return PSBA_OK;
}

int psba_schur_reduce(psba_handle h) {
  CHECK_H(h);
  NEED(h, h->assembled, "psba_schur_assemble first");
  if (!h->comm || h->try_shortcut) return PSBA_OK;
  ProfScope ps(h, PSBA_K_ALLREDUCE);
  TRY(allreduce_schur(h));
  return PSBA_OK;
}

int psba_schur_solve(psba_handle h) {
  CHECK_H(h);
  NEED(h, h->assembled, "psba_schur_assemble first");
  if (h->try_shortcut) {  // structure-only: dpa is zero already, the try is stamped, psba_backsub does the rest
    h->assembled = false;
    h->solved = true;
    return PSBA_OK;
  }
  if (h->packed_pending) TRY(allreduce_schur(h));  // psba_schur_reduce was skipped
  h->cholmod_factor = false;
  if (h->solver == PSBA_SOLVER_PCG) {
    TRY(h->cnp != 6 ? launch_fpcg_solve(h) : launch_pcg_solve(h));
    h->assembled = false;
    h->solved = true;
    h->precond_ok = h->cnp != 6;
    return h->pcg_exhausted ? PSBA_PCG_MAXIT : PSBA_OK;
  }
  TRY(launch_chol_solve(h));
  if (h->chol_tim) {
    long long t[32];
    PSBA_HIP(h, hipMemcpyAsync(t, h->chol_tim, sizeof t, hipMemcpyDeviceToHost, h->stream));
    PSBA_HIP(h, hipStreamSynchronize(h->stream));
    fprintf(stderr, "chol stamps (cycles since the first):");
    for (int k = 1; k < 32; k++) fprintf(stderr, " %lld", t[k] ? t[k] - t[0] : 0);
    fprintf(stderr, "\n");
  }
  h->assembled = false;  // S is overwritten by its factor
  h->solved = true;
  return PSBA_OK;
}

// the try's scalar block to the host behind everything queued on s, and the event the host waits for
static int publish_scalars(psba_ctx *h, hipStream_t s) {
  if (h->h_scal_dev && !getenv("PSBA_SCAL_MEMCPY"))
    TRY(launch_publish_scal(h, s));
  else
    PSBA_HIP(h, hipMemcpyAsync(h->h_scal, h->scal, sizeof(double) * NSCAL, hipMemcpyDeviceToHost, s));
  PSBA_HIP(h, hipEventRecord(h->scal_event, s));
  return PSBA_OK;
}

int psba_backsub_async(psba_handle h, double mu) {
  CHECK_H(h);
  NEED(h, h->solved, "psba_schur_solve first");
  TRY(launch_backsub(h, mu, false));
  hipStream_t s = h->stream;
  if (h->comm) {
    // four sums (as partial sets) + two status flags in one collective -- on the side stream, so
    // that the linearization the loop queues next (psba_linearize_ahead) runs beside the collective
    // and the copy instead of behind them (a small all-reduce is ~20-30 us of latency, K1 33 us)
    // (one rank: the collective is a 5 us copy and the two event hops cost more than they hide --
    // 0.221 against 0.213 ms per LM iteration; PSBA_COMM_SIDE_STREAM=1 forces the side stream there,
    // which is how the tests cover it; N > 1 has not been measured
    // and without a communicator a side stream for the scalar copy alone cost 18 us per iteration
    // (0.203 against 0.185 ms: the second stream slows the graph launches of the main one), so the
    // side stream is opt-in until an N > 1 run says otherwise)
    if (h->stream2 && getenv("PSBA_COMM_SIDE_STREAM")) {
      PSBA_HIP(h, hipEventRecord(h->k3_event, h->stream));
      PSBA_HIP(h, hipStreamWaitEvent(h->stream2, h->k3_event, 0));
      s = h->stream2;
      h->scal_side = true;
    }
    RCCL(h, ncclAllReduce(h->scal + SC_PART, h->scal + SC_PART, 4 * SC_NPART + 2, ncclDouble, ncclSum, h->comm, s));
  }
  h->publish_in_k1 = false;
  // single rank: the scalars are not sent yet -- if psba_linearize_ahead comes next, its kernel carries
  // them (no kernel of their own between K3 and the linearization); psba_backsub_wait sends them
  // itself otherwise
  h->publish_deferred = !h->comm && h->h_scal_dev && !getenv("PSBA_SCAL_MEMCPY") && !getenv("PSBA_SCAL_KERNEL");
  if (!h->publish_deferred) TRY(publish_scalars(h, s));
  h->solved = false;  // the try's accumulators are consumed; a new try starts at psba_schur_assemble
  h->backsub_pending = true;
  h->ahead = false;
  return PSBA_OK;
}

extern "C++" {
namespace psba {

// May psba_levmar queue its look-ahead linearizations in the lean form?  Everything the lean kernels leave out: a lens
// model, covariance weights or a robust loss (h->lens), fixed blocks, priors, more than one rank or a communicator,
// the packed reduce, any K2 route but the LDS partitions in the rows layout (lean_ok, PSBA_SCHUR_ATOMIC), K3 reading W,
// the development forms of K1 and K2.  Anything else takes the standard form, silently.
bool lean_eligible(psba_ctx *h) {
  return h->lean_ok && h->uploaded && h->solver == PSBA_SOLVER_DENSE && h->lens == 0 && !h->has_fixed && !h->has_prior &&
         !h->comm && h->nranks == 1 && !getenv("PSBA_SCHUR_ATOMIC") && !getenv("PSBA_BACK_READ_W") && !getenv("PSBA_LIN_V1") &&
         !getenv("PSBA_LIN_MODE") && !getenv("PSBA_SCHUR_MODE");
}

// lean_eligible, and the record buffers exist: they are allocated by the first call that can use them, so a handle that
// never runs psba_levmar lean does not hold them, and a handle that cannot have them (no memory) takes the standard
// form from then on like any other ineligible one
bool lean_prepare(psba_ctx *h) {
  if (!lean_eligible(h)) return false;
  if (h->R.get() && h->R_alt.get()) return true;
  const size_t n = (size_t)LEAN_REC * h->d.nO;
  if (h->R.alloc(h, n) < 0 || h->R_alt.alloc(h, n) < 0) {
    h->R.reset();
    h->R_alt.reset();
    (void)hipGetLastError();  // (the failed hipMalloc is not this call's error)
    h->err.clear();
    h->lean_ok = false;
    return false;
  }
  return true;
}

int linearize_ahead(psba_ctx *h, bool lean) {
  CHECK_H_NOJOIN(h);  // K1 reads and writes nothing the scalar collective touches
  NEED(h, h->backsub_pending || h->backsubbed, "psba_backsub_async / psba_backsub first");
  const bool carry = h->backsub_pending && h->publish_deferred;
  if (carry) h->pub_seq += 1.0;
  h->free_obs = false;  // (free_Be is about to hold the blocks at the proposal, W those at the current parameters)
  TRY(launch_linearize(h, false, true, carry, lean));
  if (carry) {
    h->publish_deferred = false;
    h->publish_in_k1 = true;
  }
  h->ahead = true;
  return PSBA_OK;
}

// Before psba_levmar returns: a lean linearization that a later verb could still reach -- the current set while it
// counts as linearized or spares the next psba_linearize, the set queued ahead while psba_accept may still take it --
// is replaced by a standard one at the same parameters and coefficients, so that W, U and g_a are what every other
// verb expects.  (One K1 where the call ends on an accepted step with its look-ahead queued, two -- the set queued
// ahead and the current one -- where it ends after a rejected try or on an error, none where it ends on an accepted
// step without a look-ahead, as through max_iter; PV is rewritten with the same values.)
// Because no lean set outlives psba_levmar, and psba_levmar linearizes with (1, 1) throughout, the coefficients
// launch_schur_lds takes from the handle when it assembles are the ones the set's K1 was launched with (PV carries
// them); the test hook below keeps to that by taking them over from the psba_linearize in front of it.
int lean_restore(psba_ctx *h) {
  if (h->cnp != 6) return PSBA_OK;
  if (h->lean_alt && h->ahead) TRY(launch_linearize(h, false, true, false, false));
  if (h->lean_cur && (h->linearized || h->lin_is_ahead)) TRY(launch_linearize(h, false, false, false, false));
  h->lean_cur = h->lean_alt = false;
  return PSBA_OK;
}

}  // namespace psba
}  // extern "C++"

int psba_linearize_ahead(psba_handle h) { return linearize_ahead(h, false); }

int psba_linearize_lean(psba_handle h) {
  CHECK_H(h);
  NEED(h, h->linearized, "psba_linearize first");
  NEED(h, !h->backsub_pending, "a damping try is in flight (psba_backsub_wait first)");
  NEED(h, lean_prepare(h), "this handle takes the standard form only (psba_lm_ran_lean in include/psba_hip.h lists what the lean form needs)");
  TRY(launch_linearize(h, false, false, false, true));
  h->assembled = h->solved = h->backsubbed = false;
  return PSBA_OK;
}

int psba_lm_ran_lean(psba_handle h, int *lean) {
  CHECK_H(h);
  if (lean) *lean = h->lm_lean ? 1 : 0;
  return PSBA_OK;
}

int psba_backsub_wait(psba_handle h, psba_try_scalars *out) {
  CHECK_H_NOJOIN(h);
  NEED(h, h->backsub_pending, "psba_backsub_async first");
  if (h->publish_deferred) {  // no linearization was queued ahead: send the scalars now
    TRY(publish_scalars(h, h->stream));
    h->publish_deferred = false;
  }
  // the host's own copy of the block: everything below is formed from it, never from pinned memory in place
  union {
    unsigned long long w[PUB_RAW];
    double d[PUB_RAW];
  } blk;
  if (h->publish_in_k1) {
    // workgroup 0 of the linearization queued ahead writes the block, the stamp and the check word
    // (scal_publish.h): poll the stamp in pinned memory (a try is ~180 us of GPU work) and take the block
    // behind it.  The wanted stamp over a block that fails its check is a torn reading -- the stamp reached
    // host memory ahead of words written before it: read again.  Should no block be accepted, the
    // stream's end tells why; every word has arrived by then
    const volatile unsigned long long *raw = reinterpret_cast<const volatile unsigned long long *>(h->h_scal.get());
    const unsigned long long want = pub_bits(h->pub_seq);
    bool ok = false, torn = false, stamped = false;
    long long spin = 0;
    for (;;) {
      if (raw[PUB_STAMP] == want) {
        if ((ok = pub_take(raw, want, blk.w, &stamped))) break;
        torn = torn || stamped;
      }
      if (++spin >= 200000000LL) break;
      if ((spin & 0xfffff) == 0 && hipStreamQuery(h->stream) != hipErrorNotReady) break;
    }
    if (!ok) {
      PSBA_HIP(h, hipStreamSynchronize(h->stream));
      ok = pub_take(raw, want, blk.w);
    }
    if (torn) h->pub_torn++;
    if (!ok) return fail(h, PSBA_E_HIP, "the try's scalars did not reach the host");
    h->pub_takes++;
    h->publish_in_k1 = false;
  } else {
    // poll the event for a while before handing the thread to the runtime's wait (0.9 us per LM
    // iteration on the venice-shaped problem)
    for (int spin = 0; spin < 20000 && hipEventQuery(h->scal_event) == hipErrorNotReady; spin++) {
    }
    PSBA_HIP(h, hipEventSynchronize(h->scal_event));
    memcpy(blk.d, h->h_scal.get(), sizeof(double) * NSCAL);
  }
  h->scal_side = false;  // the host has seen the side stream's work complete
  h->backsub_pending = false;
  // the four sums arrive as SC_NPART partial sets: add them up in a fixed order
  double sum[4];
  for (int q = 0; q < 4; q++) {
    double v = 0.0;
    for (int s = 0; s < SC_NPART; s++) v += blk.d[SC_PART + 4 * s + q];
    sum[q] = v;
  }
  // K3 publishes the status as flags (summed over ranks): > 0 <=> flagged on some rank
  const int st0 = blk.d[SC_STATUS_V] > 0.0 ? h->try_id : 0;
  const int st1 = blk.d[SC_STATUS_SPD] > 0.0 ? h->try_id : 0;
  h->backsubbed = true;
  if (out) {
    out->status = (st1 == h->try_id ? PSBA_NOT_SPD : 0) | (st0 == h->try_id ? PSBA_SINGULAR_V : 0);
    out->dp_l2 = sum[0];
    out->gain_den = sum[1];
    out->new_cost = sum[2];
    out->newp_l2 = sum[3];
  }
  return PSBA_OK;
}

// ---- the handshake's test hooks (scal_publish.h) ----
int psba_scal_block_check(const double *block, double stamp, double *check) {
  if (!block || !check) return PSBA_E_INVALID;
  unsigned long long w[PUB_WORDS];
  memcpy(w, block, sizeof w);
  const unsigned long long c = pub_check(w, pub_bits(stamp));
  memcpy(check, &c, sizeof c);
  return PSBA_OK;
}

int psba_scal_block_take(const double *words, double want_stamp, double *out) {
  if (!words || !out) return PSBA_E_INVALID;
  unsigned long long copy[PUB_RAW];
  const bool ok = pub_take(reinterpret_cast<const volatile unsigned long long *>(words), pub_bits(want_stamp), copy);
  memcpy(out, copy, sizeof(double) * PUB_WORDS);
  return ok ? 1 : 0;
}

int psba_publish_stats(psba_handle h, long long *takes, long long *torn) {
  CHECK_H_NOJOIN(h);
  if (takes) *takes = h->pub_takes;
  if (torn) *torn = h->pub_torn;
  return PSBA_OK;
}

int psba_test_publish(psba_handle h, const double *block, int threads, double *raw) {
  CHECK_H(h);
  if (!raw || (threads != 64 && threads != 128 && threads != 256))
    return fail(h, PSBA_E_INVALID, "psba_test_publish: raw[%d] and 64, 128 or 256 threads", PUB_RAW);
  NEED(h, !h->backsub_pending, "a damping try is in flight (psba_backsub_wait first)");
  NEED(h, h->h_scal_dev, "no device address of the pinned block");
  h->backsubbed = false;  // the try's result goes: psba_accept needs a new try
  // a given block stands in the device scalar block for the launch only: the block also holds the status stamps, the
  // cost and the largest diagonal entry, which the next verbs read
  double saved[NSCAL];
  if (block) {
    TRY(d2h(h, saved, h->scal, sizeof saved));
    PSBA_HIP(h, hipMemcpyAsync(h->scal, block, sizeof saved, hipMemcpyHostToDevice, h->stream));
  }
  TRY(launch_test_publish(h, threads));
  if (block) PSBA_HIP(h, hipMemcpyAsync(h->scal, saved, sizeof saved, hipMemcpyHostToDevice, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  memcpy(raw, h->h_scal.get(), sizeof(double) * PUB_RAW);
  return PSBA_OK;
}

int psba_backsub(psba_handle h, double mu, psba_try_scalars *out) {
  TRY(psba_backsub_async(h, mu));
  return psba_backsub_wait(h, out);
}

int psba_accept(psba_handle h) {
  CHECK_H(h);
  NEED(h, h->backsubbed, "psba_backsub first");
  const bool ahead = h->ahead, lean = h->ahead && h->lean_alt;
  h->cur = 1 - h->cur;
  params_changed(h);  // what was derived belonged to the parameters that were current: both covariances among it
  h->ahead = ahead;  // (what the linearization queued ahead keeps alive is set again below)
  h->free_obs = h->ahead && h->cnp != 6;  // W_alt and free_Be of the linearization queued ahead become the current pair
  if (h->ahead) {  // the linearization at the (now current) proposed parameters exists already
    std::swap(h->W, h->W_alt);
    std::swap(h->PV, h->PV_alt);
    std::swap(h->U, h->U_alt);
    std::swap(h->ga, h->ga_alt);
    std::swap(h->damp_D, h->damp_D_alt);
    std::swap(h->R, h->R_alt);
    h->lean_cur = lean;  // (the set that held the old parameters is dead until K1 writes it again)
  }
  h->damp_ok = h->ahead && h->damp_kind == PSBA_DAMPING_MARQUARDT;
  // only a linearization that was computed ahead for THIS proposal spares the next psba_linearize
  // (an earlier accept's flag must not survive: psba_set_step -> psba_accept -> psba_linearize)
  h->lin_is_ahead = h->ahead;
  h->ahead = false;
  return PSBA_OK;
}

// ---- operators of the trust-region caller ---------------------------------

// ---- the sharded dense factorization, piece by piece (kernels_chol_graph.hip: chol_dist_*) ----
int psba_chol_dist_shape(psba_handle h, int *n32, int *NB, int *sharded) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  int nb = 0, bl = 0;
  TRY(chol_dist_shape(h, &nb, &bl));
  if (n32) *n32 = h->n32;
  if (NB) *NB = nb;
  if (sharded) *sharded = bl;
  return PSBA_OK;
}
int psba_chol_shape(psba_handle h, int *out8) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  if (!out8) return fail(h, PSBA_E_INVALID, "psba_chol_shape: null pointer");
  return chol_shape(h, out8);
}
int psba_chol_dist_exchange_plan(int n32, int NB, int nranks, int JE, long long *out4, int cap) {
  if (!out4 || cap <= 0) return PSBA_E_INVALID;
  return psba::chol_dist_exchange_plan(n32, NB, nranks, JE, reinterpret_cast<long long(*)[4]>(out4), cap);
}
int psba_chol_dist_begin(psba_handle h) {
  CHECK_H(h);
  NEED_DENSE(h);
  NEED(h, h->assembled, "psba_schur_assemble (and the reduction over ranks) first");
  if (h->packed_pending) {
    TRY(launch_schur_expand(h));
    h->packed_pending = false;
  }
  h->cholmod_factor = false;
  return chol_dist_begin(h);
}
int psba_chol_dist_superpanel(psba_handle h, int J) {
  CHECK_H(h);
  NEED_DENSE(h);
  NEED(h, h->assembled, "psba_schur_assemble first");
  if (J < 0 || J >= h->n32) return fail(h, PSBA_E_INVALID, "super-panel column %d out of range", J);
  h->cholmod_factor = false;
  return chol_dist_superpanel(h, J);
}
int psba_chol_dist_block(psba_handle h, int B, int set, double *buf, long long *n_doubles) {
  CHECK_H(h);
  NEED_DENSE(h);
  NEED(h, h->assembled, "psba_schur_assemble first");
  if (B < 0 || 64 * B >= h->n32) return fail(h, PSBA_E_INVALID, "column block %d out of range", B);
  const int ncols = h->n32 - 64 * B < 64 ? h->n32 - 64 * B : 64;
  const long long n = (long long)(h->n32 + 1 - 64 * B) * ncols;
  if (n_doubles) *n_doubles = n;
  if (!buf) return PSBA_OK;
  if (!h->dist_buf) TRY(h->dist_buf.alloc(h, (size_t)(h->n32 + 1) * 64 * 8));
  if (set) {
    h->cholmod_factor = false;
    PSBA_HIP(h, hipMemcpyAsync(h->dist_buf, buf, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    return chol_dist_block(h, B, h->dist_buf, 1);
  }
  TRY(chol_dist_block(h, B, h->dist_buf, 0));
  return d2h(h, buf, h->dist_buf, sizeof(double) * (size_t)n);
}
int psba_chol_dist_finish(psba_handle h) {
  CHECK_H(h);
  NEED_DENSE(h);
  NEED(h, h->assembled, "psba_schur_assemble first");
  h->cholmod_factor = false;
  TRY(chol_dist_finish(h));
  h->assembled = false;
  h->solved = true;
  return PSBA_OK;
}

static int ensure_trv(psba_ctx *h) {
  for (int k = 0; k < 2; k++)
    if (!h->trv[k]) TRY(h->trv[k].alloc(h, (size_t)h->d.nT));
  return PSBA_OK;
}

int psba_jmul_dots(psba_handle h, const double *x1, const double *x2, double dots[3]) {
  CHECK_H(h);
  NEED_SIX(h);
  NEED(h, h->uploaded, "no problem uploaded");
  if (!x1 || !dots) return fail(h, PSBA_E_INVALID, "psba_jmul_dots: null pointer");
  TRY(ensure_trv(h));
  const size_t bytes = sizeof(double) * (size_t)h->d.nT;
  PSBA_HIP(h, hipMemcpyAsync(h->trv[0], x1, bytes, hipMemcpyHostToDevice, h->stream));
  if (x2 && x2 != x1) PSBA_HIP(h, hipMemcpyAsync(h->trv[1], x2, bytes, hipMemcpyHostToDevice, h->stream));
  TRY(launch_jmul(h, h->trv[0], (x2 && x2 != x1) ? h->trv[1] : h->trv[0], nullptr, h->scal + SC_TR_DOTS));
  // the dot products run over observations: with points sharded over ranks, the sum of the ranks'
  // (a rank layout without a communicator returns this rank's part)
  if (h->comm)
    RCCL(h, ncclAllReduce(h->scal + SC_TR_DOTS, h->scal + SC_TR_DOTS, 3, ncclDouble, ncclSum, h->comm, h->stream));
  TRY(fetch_scalars(h));
  for (int k = 0; k < 3; k++) dots[k] = h->h_scal[SC_TR_DOTS + k];
  return PSBA_OK;
}

int psba_set_solver(psba_handle h, int solver, double tol, int max_iter) {
  CHECK_H(h);
  if (solver != PSBA_SOLVER_DENSE && solver != PSBA_SOLVER_PCG && solver != PSBA_SOLVER_SPARSE)
    return fail(h, PSBA_E_INVALID, "unknown solver %d", solver);
  // PSBA_SOLVER_SPARSE is PSBA_SOLVER_PCG with the flag: with six-parameter blocks nothing else reads the flag, on
  // blocks of 11 / 16 the upload and the dispatch do
  const bool any_block = solver == PSBA_SOLVER_SPARSE;
  if (any_block) solver = PSBA_SOLVER_PCG;
  NEED(h, !h->uploaded || (solver == h->solver && (h->cnp == 6 || any_block == h->sparse_any_block)),
       "psba_set_solver before psba_upload_problem (the buffers depend on it)");
  h->solver = solver;
  if (!h->uploaded) h->sparse_any_block = any_block;
  if (tol > 0) h->pcg_tol = tol;
  if (max_iter > 0) h->pcg_maxit = max_iter;
  return PSBA_OK;
}

int psba_pcg_info(psba_handle h, int *iters, double *relres, long long *blocks, long long *dense_blocks) {
  CHECK_H(h);
  NEED(h, h->uploaded && h->solver == PSBA_SOLVER_PCG, "PSBA_SOLVER_PCG and an uploaded problem");
  if (iters) *iters = h->pcg_iters;
  if (relres) *relres = h->pcg_relres;
  if (blocks) *blocks = h->bs_nblk;
  if (dense_blocks) *dense_blocks = (long long)h->d.nC * (h->d.nC + 1) / 2;
  return PSBA_OK;
}

// the block-sparse S as assembled (after psba_schur_assemble / psba_schur_reduce): jk[2 blocks], val[36 blocks], ea[nA]
int psba_get_sparse_S(psba_handle h, int *jk, double *val, double *ea) {
  CHECK_H(h);
  NEED(h, h->assembled && h->solver == PSBA_SOLVER_PCG, "psba_schur_assemble with PSBA_SOLVER_PCG first");
  NEED(h, !h->try_shortcut, "every camera is fixed: this try assembled no S (PSBA_FIXED_NO_SHORTCUT=1 keeps the general route)");
  if (jk) TRY(d2h(h, jk, h->bs_jk, sizeof(int2) * (size_t)h->bs_nblk));
  if (val) TRY(d2h(h, val, h->bs_val, sizeof(double) * (size_t)(h->cnp * h->cnp) * (size_t)h->bs_nblk));
  if (ea) TRY(d2h(h, ea, h->bs_ea, sizeof(double) * (size_t)h->d.nA));
  return PSBA_OK;
}

// the counterpart for a host that sums the ranks' blocks itself (between psba_schur_assemble and psba_schur_solve)
int psba_set_sparse_S(psba_handle h, const double *val, const double *ea) {
  CHECK_H(h);
  NEED(h, h->assembled && h->solver == PSBA_SOLVER_PCG, "psba_schur_assemble with PSBA_SOLVER_PCG first");
  NEED(h, !h->try_shortcut, "every camera is fixed: this try assembled no S (PSBA_FIXED_NO_SHORTCUT=1 keeps the general route)");
  if (val) PSBA_HIP(h, hipMemcpyAsync(h->bs_val, val, sizeof(double) * (size_t)(h->cnp * h->cnp) * (size_t)h->bs_nblk, hipMemcpyHostToDevice, h->stream));
  std::vector<double> kept;
  if (ea && h->cnp == KD_CNP && !h->kd_rep_h.empty()) {  // shared intrinsics: e_a is 0 at a folded-away coordinate
    kept.assign(ea, ea + h->d.nA);
    for (int j = 0; j < h->d.nC; j++)
      for (int k = 0; k < 10 && h->kd_rep_h[j] != j; k++) {
        const unsigned bits = h->kd_cmask_h.empty() ? h->kd_mask : h->kd_mask & h->kd_cmask_h[j];
        if ((bits >> k) & 1u) kept[(size_t)KD_CNP * j + k] = 0.0;
      }
    ea = kept.data();
  }
  if (ea) PSBA_HIP(h, hipMemcpyAsync(h->bs_ea, ea, sizeof(double) * (size_t)h->d.nA, hipMemcpyHostToDevice, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  h->solved = h->backsubbed = false;
  h->precond_ok = false;
  return PSBA_OK;
}

// test hook (psba_hip.h): the inverses of the diagonal blocks the last solve of this route preconditioned with
int psba_get_sparse_precond(psba_handle h, double *M) {
  CHECK_H(h);
  NEED(h, h->uploaded && FREE_SPARSE(h), "PSBA_SOLVER_SPARSE on camera blocks of 11 / 16 and an uploaded problem");
  NEED(h, h->precond_ok, "psba_schur_solve first (a new assembly, psba_set_sparse_S, a covariance verb and every setter of the model end it)");
  if (!M) return fail(h, PSBA_E_INVALID, "%s: null pointer", __func__);
  return d2h(h, M, h->pcg_minv, sizeof(double) * (size_t)(h->cnp * h->cnp) * (size_t)h->d.nC);
}

// y = S x on the stored blocks, with the kernel the solve uses for its products (a mirror verb: how that kernel is judged
// on its own)
int psba_sparse_S_times(psba_handle h, const double *x, double *y) {
  CHECK_H(h);
  NEED(h, h->assembled && h->solver == PSBA_SOLVER_PCG, "psba_schur_assemble with PSBA_SOLVER_PCG first");
  NEED(h, !h->try_shortcut, "every camera is fixed: this try assembled no S (PSBA_FIXED_NO_SHORTCUT=1 keeps the general route)");
  if (!x || !y) return fail(h, PSBA_E_INVALID, "%s: null pointer", __func__);
  return h->cnp != 6 ? launch_fbsr_times(h, x, y) : launch_bsr_times(h, x, y);
}

// host only: which blocks of the lower block triangle a (shard of a) problem produces
int psba_sparse_pattern(int nCams, int n3Dpts, int n2Dprojs, const int *iidx, const int *jidx, unsigned char *flags) {
  if (nCams <= 0 || n3Dpts <= 0 || n2Dprojs <= 0 || !iidx || !jidx || !flags) return PSBA_E_INVALID;
  std::vector<int> ptr((size_t)n3Dpts + 1, 0);
  for (int a = 0; a < n2Dprojs; a++) {
    if (iidx[a] < 0 || iidx[a] >= n3Dpts || jidx[a] < 0 || jidx[a] >= nCams) return PSBA_E_INVALID;
    // point-major with cameras ascending inside a point, as psba_upload_problem requires (sparse_pattern's
    // b <= a loop relies on it: unordered cameras would flag the wrong blocks silently)
    if (a && (iidx[a] < iidx[a - 1] || (iidx[a] == iidx[a - 1] && jidx[a] <= jidx[a - 1]))) return PSBA_E_INVALID;
    ptr[(size_t)iidx[a] + 1]++;
  }
  for (int i = 0; i < n3Dpts; i++) ptr[(size_t)i + 1] += ptr[(size_t)i];
  return psba::sparse_pattern(nCams, n2Dprojs, iidx, jidx, ptr.data(), flags);
}

int psba_set_sparse_pattern(psba_handle h, const unsigned char *flags, long long n) {
  CHECK_H(h);
  if (!flags || n <= 0) return fail(h, PSBA_E_INVALID, "psba_set_sparse_pattern: null pattern");
  NEED(h, !h->uploaded, "psba_set_sparse_pattern before psba_upload_problem (the block list depends on it)");
  h->bs_pattern.assign(flags, flags + n);
  return PSBA_OK;
}

int psba_allreduce_scalars(psba_handle h, double *v, int n) {
  CHECK_H(h);
  if (!v || n < 0 || n > 8) return fail(h, PSBA_E_INVALID, "psba_allreduce_scalars: at most 8 values");
  if (!h->comm || n == 0) return PSBA_OK;  // one rank (or the caller sums): nothing to add
  double *tmp = h->scal + SC_SUMS;
  PSBA_HIP(h, hipMemcpyAsync(tmp, v, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  RCCL(h, ncclAllReduce(tmp, tmp, (size_t)n, ncclDouble, ncclSum, h->comm, h->stream));
  return d2h(h, v, tmp, sizeof(double) * (size_t)n);
}

int psba_compute_Jmultiply(psba_handle h, const double *x, double *Jmul) {
  CHECK_H(h);
  NEED_SIX(h);
  NEED(h, h->uploaded, "no problem uploaded");
  if (!x) return fail(h, PSBA_E_INVALID, "psba_compute_Jmultiply: null pointer");
  TRY(ensure_trv(h));
  if (!h->jmul_out) TRY(h->jmul_out.alloc(h, (size_t)2 * h->d.nO));
  PSBA_HIP(h, hipMemcpyAsync(h->trv[0], x, sizeof(double) * (size_t)h->d.nT, hipMemcpyHostToDevice, h->stream));
  TRY(launch_jmul(h, h->trv[0], h->trv[0], h->jmul_out, h->scal + SC_TR_DOTS));
  return d2h(h, Jmul, h->jmul_out, sizeof(double) * 2 * (size_t)h->d.nO);
}

int psba_get_gradient(psba_handle h, double *g) {
  CHECK_H(h);
  if (h->cnp == KD_CNP) {  // a copy: g_a as stored, g_b,i from the tail of each point's record
    NEED(h, h->linearized, "psba_linearize first");
    if (!g) return PSBA_E_INVALID;
    TRY(d2h(h, g, h->ga, sizeof(double) * (size_t)h->d.nA));
    std::vector<double> pv((size_t)9 * h->d.nP);
    TRY(d2h(h, pv.data(), h->PV, sizeof(double) * pv.size()));
    for (int i = 0; i < h->d.nP; i++)
      for (int k = 0; k < 3; k++) g[h->d.nA + 3 * (size_t)i + k] = pv[(size_t)9 * i + 6 + k];
    return PSBA_OK;
  }
  NEED_SIX(h);
  NEED(h, h->linearized, "psba_linearize first");
  if (!g) return PSBA_E_INVALID;
  TRY(ensure_trv(h));
  TRY(launch_pack_g(h, h->trv[0]));
  // g_a is a sum over observations: every rank holds its points' part (g_b is rank-local by nature)
  if (h->comm) RCCL(h, ncclAllReduce(h->trv[0], h->trv[0], (size_t)h->d.nA, ncclDouble, ncclSum, h->comm, h->stream));
  return d2h(h, g, h->trv[0], sizeof(double) * (size_t)h->d.nT);
}

int psba_get_dp(psba_handle h, double *dp) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  return d2h(h, dp, h->dp, sizeof(double) * (size_t)h->d.nT);
}

int psba_set_step(psba_handle h, const double *dp) {
  CHECK_H(h);
  NEED_SIX(h);
  NEED(h, h->uploaded, "no problem uploaded");
  if (!dp) return PSBA_E_INVALID;
  PSBA_HIP(h, hipMemcpyAsync(h->dp, dp, sizeof(double) * (size_t)h->d.nT, hipMemcpyHostToDevice, h->stream));
  TRY(launch_newp(h, h->dp));
  h->ahead = false;  // a linearization computed ahead belongs to another proposal
  h->backsubbed = true;  // a proposal exists: psba_accept may take it
  return PSBA_OK;
}

int psba_cholmod_lambda(psba_handle h, int reassemble, double *lambda, double *info3) {
  CHECK_H(h);
  NEED_SIX(h);
  NEED(h, h->uploaded, "no problem uploaded");
  if (h->nranks > 1 && !h->comm)
    return fail(h, PSBA_E_INVALID, "psba_cholmod_lambda on a rank layout needs the communicator (S must be complete)");
  // a structure-only try (every camera fixed) has assembled nothing, and forming S here at lambda = 0 would put the
  // try's solve on the general route with the wrong damping: finish the try first (the loops never get here: such a
  // try cannot fail its factorization)
  NEED(h, !(h->try_shortcut && h->assembled), "a structure-only try is open (psba_schur_solve / psba_backsub first)");
  if (h->try_shortcut) {  // the last try assembled nothing: whatever the caller says, S has to be formed here
    reassemble = 1;
    h->try_shortcut = false;
  }
  h->cholmod_factor = false;
  if (h->solver == PSBA_SOLVER_PCG) {
    // block-sparse mode: no dense S to factor -- the damping estimate is the Gershgorin shift of the stored blocks
    // (kernels_pcg.hip; no reference counterpart: the reference has no sparse mode)
    NEED(h, h->linearized, "psba_linearize first");
    if (reassemble || !h->assembled) {
      TRY(launch_schur(h, 0.0, false));
      TRY(allreduce_schur(h));  // every rank then looks at the same complete blocks
    }
    double lam = 0.0;
    TRY(launch_bsr_gershgorin(h, &lam, info3));
    if (lambda) *lambda = lam;
    h->assembled = h->solved = false;
    return PSBA_OK;
  }
  if (reassemble) {
    // S at lambda = 0 again (the failed factorization worked in place), then the modified
    // Cholesky on a copy of it (trust_region.cpp:341-363)
    NEED(h, h->linearized, "psba_linearize first");
    TRY(launch_schur(h, 0.0, false));
    // with a communicator (even of one rank) the sums sit in the packed buffer until the all-reduce
    // and k_schur_expand have run: the modified Cholesky must not factor a stale square
    if (h->packed_pending || h->comm) TRY(allreduce_schur(h));  // every rank then factors the same complete S
  }
  h->diag_done = false;  // the first diagonal block's factor in chol_L is about to be overwritten
  TRY(launch_cholmod(h, h->scal + SC_CHOLMOD));
  TRY(fetch_scalars(h));
  if (lambda) *lambda = h->h_scal[SC_CHOLMOD];
  if (info3)
    for (int k = 0; k < 3; k++) info3[k] = h->h_scal[SC_CHOLMOD + 1 + k];
  h->assembled = h->solved = false;
  h->cholmod_factor = true;
  return PSBA_OK;
}

// test hook (psba_hip.h): the factor the modified Cholesky left in chol_L
int psba_get_cholmod_factor(psba_handle h, double *L) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  NEED(h, !FREE_SPARSE(h), "no Cholesky chain and no modified Cholesky factor with PSBA_SOLVER_SPARSE");
  NEED(h, h->solver != PSBA_SOLVER_PCG, "no modified Cholesky factor with PSBA_SOLVER_PCG (the estimate is a Gershgorin shift)");
  NEED(h, h->cholmod_factor, "psba_cholmod_lambda first (every verb that factors or assembles S overwrites the factor)");
  if (!L) return fail(h, PSBA_E_INVALID, "psba_get_cholmod_factor: null pointer");
  const size_t n = (size_t)h->d.nA;
  PSBA_HIP(h, hipMemcpy2DAsync(L, sizeof(double) * n, h->chol_L, sizeof(double) * (size_t)h->n32, sizeof(double) * n, n,
                               hipMemcpyDeviceToHost, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  return PSBA_OK;
}

// test hook (psba_hip.h): W_a and B_a | e_a as k_free_linearize stored them
int psba_get_free_obs_blocks(psba_handle h, double *W, double *Be) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  NEED(h, h->cnp != 6, "free-intrinsics camera blocks only (six-parameter blocks: psba_compute_jacobiQT, psba_compute_Wblks)");
  NEED(h, h->linearized && h->free_obs,
       "psba_linearize first (psba_linearize_ahead, psba_accept and every verb that moves the parameters or the model "
       "invalidate the blocks)");
  TRY(d2h(h, W, h->W, sizeof(double) * 3 * (size_t)h->cnp * h->d.nO));
  return d2h(h, Be, h->free_Be, sizeof(double) * 8 * (size_t)h->d.nO);
}

// s_a and w_a = omega_a / sigma_a of the observation weighting at a parameter set; without a weighting
// s = |e|^2 and w = 1
int psba_get_obs_weights(psba_handle h, int which, double *s, double *w) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  NEED(h, h->cnp != 6, "free-intrinsics models only (PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD); six-parameter blocks: psba_obs_sq_residuals");
  if (which != PSBA_PARAMS_CUR && which != PSBA_PARAMS_NEW) return fail(h, PSBA_E_INVALID, "%s: which = %d", __func__, which);
  NEED(h, !h->backsub_pending, "a damping try is in flight (psba_backsub_wait first)");
  NEED(h, which == PSBA_PARAMS_CUR || h->backsubbed, "PSBA_PARAMS_NEW: no proposal (psba_backsub first)");
  const size_t nO = (size_t)h->d.nO;
  if (!h->obs_sw) TRY(h->obs_sw.alloc(h, 2 * nO));
  TRY(launch_obs_weights_free(h, which, h->obs_sw, h->obs_sw + nO));
  if (s) TRY(d2h(h, s, h->obs_sw, sizeof(double) * nO));
  if (w) TRY(d2h(h, w, h->obs_sw + nO, sizeof(double) * nO));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  return PSBA_OK;
}

// ---- sba_func.h mirror ------------------------------------------------------------------

static int ensure_dbg(psba_ctx *h) {
  const Dims &d = h->d;
  if (!h->dbg_ex) TRY(h->dbg_ex.alloc(h, (size_t)2 * d.nO));
  if (!h->dbg_JA) TRY(h->dbg_JA.alloc(h, (size_t)12 * d.nO));
  if (!h->dbg_JB) TRY(h->dbg_JB.alloc(h, (size_t)6 * d.nO));
  if (!h->dbg_Y) TRY(h->dbg_Y.alloc(h, (size_t)18 * d.nO));
  if (!h->dbg_Vinv) TRY(h->dbg_Vinv.alloc(h, (size_t)9 * d.nP));
  if (!h->dbg_eb) TRY(h->dbg_eb.alloc(h, (size_t)3 * d.nP));
  return PSBA_OK;
}

static int relinearize_dump(psba_ctx *h) {
  TRY(ensure_dbg(h));
  TRY(launch_linearize(h, true));
  h->linearized = true;
  h->assembled = h->solved = h->backsubbed = false;
  return PSBA_OK;
}

static int reassemble_dump(psba_ctx *h) {
  NEED(h, h->linearized, "linearise first (compute_jacobiQT / compute_U / ...)");
  TRY(ensure_dbg(h));
  h->try_shortcut = false;  // the mirror always takes the general route
  h->cholmod_factor = false;
  TRY(launch_schur(h, h->mu_applied ? h->mu : 0.0, true));
  h->assembled = true;
  h->solved = h->backsubbed = false;
  if (h->comm) TRY(allreduce_schur(h));
  return PSBA_OK;
}

int psba_compute_exQT(psba_handle h, int which, double *ex) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  TRY(ensure_dbg(h));
  TRY(launch_residual(h, which, h->dbg_ex));
  return d2h(h, ex, h->dbg_ex, sizeof(double) * 2 * (size_t)h->d.nO);
}

int psba_compute_jacobiQT(psba_handle h, double *jac_A, double *jac_B) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  TRY(relinearize_dump(h));
  TRY(d2h(h, jac_A, h->dbg_JA, sizeof(double) * 12 * (size_t)h->d.nO));
  return d2h(h, jac_B, h->dbg_JB, sizeof(double) * 6 * (size_t)h->d.nO);
}

int psba_compute_U(psba_handle h, double coeff, double *out) {
  CHECK_H(h);
  NEED_SIX(h);
  NEED(h, h->uploaded, "no problem uploaded");
  h->coeff = coeff;
  TRY(relinearize_dump(h));
  return d2h(h, out, h->U, sizeof(double) * 36 * (size_t)h->d.nC);
}

static int download_V(psba_ctx *h, double *out, double mu) {
  if (!out) return PSBA_OK;
  std::vector<double> pv((size_t)9 * h->d.nP);
  TRY(d2h(h, pv.data(), h->PV, sizeof(double) * pv.size()));
  for (int i = 0; i < h->d.nP; i++) {
    const double *s = &pv[(size_t)9 * i];
    double *o = out + (size_t)9 * i;
    o[0] = s[0] + mu; o[1] = s[1]; o[2] = s[2];
    o[3] = s[1]; o[4] = s[3] + mu; o[5] = s[4];
    o[6] = s[2]; o[7] = s[4]; o[8] = s[5] + mu;
  }
  return PSBA_OK;
}

int psba_compute_V(psba_handle h, double coeff, double *out) {
  CHECK_H(h);
  NEED_SIX(h);
  NEED(h, h->uploaded, "no problem uploaded");
  h->coeff = coeff;
  TRY(relinearize_dump(h));
  return download_V(h, out, 0.0);
}

int psba_maxElmOfUV(psba_handle h, double *out) { return psba_max_diag(h, out); }

int psba_update_UV(psba_handle h, double mu, double *U, double *V) {
  CHECK_H(h);
  NEED_SIX(h);
  NEED(h, h->linearized, "linearise first");
  h->mu = mu;
  h->mu_applied = true;
  if (U) {
    TRY(d2h(h, U, h->U, sizeof(double) * 36 * (size_t)h->d.nC));
    for (int t = 0; t < h->d.nA; t++) U[36 * (t / 6) + 7 * (t % 6)] += mu;
  }
  return download_V(h, V, mu);
}

int psba_restore_UVdiag(psba_handle h) {
  CHECK_H(h);
  h->mu_applied = false;
  return PSBA_OK;
}

int psba_compute_Vinv(psba_handle h, double *Vinv) {
  CHECK_H(h);
  TRY(reassemble_dump(h));
  TRY(d2h(h, Vinv, h->dbg_Vinv, sizeof(double) * 9 * (size_t)h->d.nP));
  TRY(fetch_scalars(h));
  return h->h_status[0] == h->try_id ? PSBA_SINGULAR_V : PSBA_OK;
}

int psba_compute_Wblks(psba_handle h, double coeff, double *Wblks) {
  CHECK_H(h);
  NEED_SIX(h);
  NEED(h, h->uploaded, "no problem uploaded");
  h->coeff = coeff;
  TRY(relinearize_dump(h));
  return d2h(h, Wblks, h->W, sizeof(double) * 18 * (size_t)h->d.nO);
}

int psba_compute_Yblks(psba_handle h, double *Yblks) {
  CHECK_H(h);
  TRY(reassemble_dump(h));
  return d2h(h, Yblks, h->dbg_Y, sizeof(double) * 18 * (size_t)h->d.nO);
}

int psba_compute_S(psba_handle h, double *S) {
  CHECK_H(h);
  TRY(reassemble_dump(h));
  if (!S) return PSBA_OK;
  PSBA_HIP(h, hipMemcpy2DAsync(S, sizeof(double) * h->d.nA, h->red, sizeof(double) * h->n32,
                               sizeof(double) * h->d.nA, h->d.nA, hipMemcpyDeviceToHost, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  return PSBA_OK;
}

int psba_compute_g(psba_handle h, double coeff, double *g) {
  CHECK_H(h);
  NEED_SIX(h);
  NEED(h, h->uploaded, "no problem uploaded");
  h->coeff_g = coeff;
  TRY(relinearize_dump(h));
  if (!g) return PSBA_OK;
  TRY(d2h(h, g, h->ga, sizeof(double) * (size_t)h->d.nA));
  std::vector<double> pv((size_t)9 * h->d.nP);
  TRY(d2h(h, pv.data(), h->PV, sizeof(double) * pv.size()));
  for (int i = 0; i < h->d.nP; i++)
    for (int k = 0; k < 3; k++) g[h->d.nA + 3 * (size_t)i + k] = pv[(size_t)9 * i + 6 + k];
  return PSBA_OK;
}

int psba_compute_ea(psba_handle h, double *ea) {
  CHECK_H(h);
  TRY(reassemble_dump(h));
  return d2h(h, ea, h->red + (size_t)h->n32 * h->n32, sizeof(double) * (size_t)h->d.nA);
}

int psba_SPDinv_matVec(psba_handle h, double *dpa) {
  CHECK_H(h);
  NEED_DENSE(h);
  NEED(h, h->assembled, "compute_S / compute_ea first");
  NEED(h, !h->try_shortcut, "every camera is fixed: psba_schur_assemble assembled no S (compute_S / compute_ea first)");
  h->cholmod_factor = false;
  TRY(launch_chol_solve(h));
  h->assembled = false;
  h->solved = true;
  TRY(fetch_scalars(h));
  TRY(d2h(h, dpa, h->dp, sizeof(double) * (size_t)h->d.nA));
  return h->h_status[1] == h->try_id ? PSBA_NOT_SPD : PSBA_OK;
}

static int backsub_dump(psba_ctx *h) {
  NEED(h, h->solved, "SPDinv_matVec first");
  TRY(ensure_dbg(h));
  TRY(launch_backsub(h, h->mu_applied ? h->mu : 0.0, true));
  h->backsubbed = true;
  return PSBA_OK;
}

int psba_compute_eb(psba_handle h, double *eb) {
  CHECK_H(h);
  TRY(backsub_dump(h));
  return d2h(h, eb, h->dbg_eb, sizeof(double) * 3 * (size_t)h->d.nP);
}

int psba_compute_dpb(psba_handle h, double *dp) {
  CHECK_H(h);
  TRY(backsub_dump(h));
  return d2h(h, dp, h->dp, sizeof(double) * (size_t)h->d.nT);
}

int psba_compute_newp(psba_handle h, double *new_p) {
  CHECK_H(h);
  NEED(h, h->backsubbed, "compute_dpb first");
  if (!new_p) return PSBA_OK;
  TRY(d2h(h, new_p, h->cams[1 - h->cur], sizeof(double) * (size_t)h->d.nA));
  return d2h(h, new_p + h->d.nA, h->pts[1 - h->cur], sizeof(double) * (size_t)h->d.nB);
}

int psba_update_p(psba_handle h, double *p) {
  CHECK_H(h);
  TRY(psba_accept(h));
  if (!p) return PSBA_OK;
  TRY(d2h(h, p, h->cams[h->cur], sizeof(double) * (size_t)h->d.nA));
  return d2h(h, p + h->d.nA, h->pts[h->cur], sizeof(double) * (size_t)h->d.nB);
}

// ---- multi-GPU --------------------------------------------------------------------------

int psba_partition_points(int n3Dpts, const int *iidx, int n2Dprojs, int nranks, int *pt_begin) {
  if (n3Dpts <= 0 || nranks <= 0 || !iidx || !pt_begin || n2Dprojs < 0) return PSBA_E_INVALID;
  // contiguous point ranges; rank r ends at the first point whose cumulative observation
  // count reaches (r+1)/nranks of the total
  std::vector<long long> cum((size_t)n3Dpts + 1, 0);
  for (int a = 0; a < n2Dprojs; a++) {
    if (iidx[a] < 0 || iidx[a] >= n3Dpts) return PSBA_E_INVALID;
    cum[(size_t)iidx[a] + 1]++;
  }
  for (int i = 0; i < n3Dpts; i++) cum[(size_t)i + 1] += cum[i];
  pt_begin[0] = 0;
  int p = 0;
  for (int r = 1; r < nranks; r++) {
    const long long target = (long long)n2Dprojs * r / nranks;
    while (p < n3Dpts && cum[p] < target) p++;
    // keep at least one point per rank when there are enough points
    int lo = pt_begin[r - 1] + 1, hi = n3Dpts - (nranks - r);
    if (n3Dpts >= nranks) {
      if (p < lo) p = lo;
      if (p > hi) p = hi;
    }
    pt_begin[r] = p;
  }
  pt_begin[nranks] = n3Dpts;
  return PSBA_OK;
}

int psba_comm_unique_id(void *id128) {
  if (!id128) return PSBA_E_INVALID;
  static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id is 128 bytes");
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return PSBA_E_RCCL;
  memcpy(id128, &id, sizeof id);
  return PSBA_OK;
}

int psba_comm_init(psba_handle h, int nranks, int rank, const void *id128) {
  CHECK_H(h);
  if (nranks < 1 || rank < 0 || rank >= nranks || !id128)
    return fail(h, PSBA_E_INVALID, "psba_comm_init: bad rank %d / %d", rank, nranks);
  PSBA_HIP(h, hipSetDevice(h->device));
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  RCCL(h, ncclCommInitRank(&h->comm, nranks, id, rank));
  if (!h->stream2) {
    PSBA_HIP(h, hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    PSBA_HIP(h, hipEventCreateWithFlags(&h->k3_event, hipEventDisableTiming));
  }
  h->nranks = nranks;
  h->rank = rank;
  return PSBA_OK;
}

int psba_set_rank_layout(psba_handle h, int nranks, int rank) {
  CHECK_H(h);
  NEED(h, h->cnp == 6 || nranks <= 1, "free intrinsics (PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD): single rank only");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(h, PSBA_E_INVALID, "bad rank %d / %d", rank, nranks);
  if (h->comm) return fail(h, PSBA_E_STATE, "a communicator is attached: its layout is fixed");
  if (h->solver == PSBA_SOLVER_PCG && h->uploaded && nranks != h->nranks)
    return fail(h, PSBA_E_STATE, "PSBA_SOLVER_PCG: the rank layout is part of the block list, set it before psba_upload_problem");
  h->nranks = nranks;
  h->rank = rank;
  return PSBA_OK;
}

// (with the PSBA_SCHUR_PACKED test hook the buffer is the packed [tril(S) | e_a] sums a
// communicator would all-reduce: 36 doubles per block of the lower block triangle)
static bool packed_hook(psba_ctx *h) {
  return !h->comm && h->nranks > 1 && (h->nGroups > 0 || h->ring_nWg > 0) && getenv("PSBA_SCHUR_PACKED");
}

int psba_reduce_buffer_size(psba_handle h, long long *n_doubles) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  if (n_doubles) *n_doubles = packed_hook(h) ? (long long)h->packed_doubles : (long long)(h->n32 + 1) * h->n32;
  return PSBA_OK;
}

int psba_get_reduce_buffer(psba_handle h, double *out) {
  CHECK_H(h);
  NEED(h, h->assembled, "psba_schur_assemble first");
  NEED(h, !h->comm, "the reduce-buffer verbs are for handles without a communicator");
  NEED(h, !FREE_SPARSE(h), "no dense reduce buffer with PSBA_SOLVER_SPARSE (psba_get_sparse_S)");
  NEED(h, h->solver != PSBA_SOLVER_PCG, "no dense reduce buffer with PSBA_SOLVER_PCG (psba_get_sparse_S)");
  NEED(h, !h->try_shortcut, "every camera is fixed: this try assembled no S (PSBA_FIXED_NO_SHORTCUT=1 keeps the general route)");
  if (packed_hook(h)) return d2h(h, out, h->redp, sizeof(double) * h->packed_doubles);
  return d2h(h, out, h->red, sizeof(double) * (size_t)(h->n32 + 1) * h->n32);
}

int psba_set_reduce_buffer(psba_handle h, const double *in) {
  CHECK_H(h);
  NEED_DENSE(h);
  NEED(h, h->cnp == 6 || h->cnp == KD_CNP, SIX_ONLY);
  NEED(h, h->assembled, "psba_schur_assemble first");
  NEED(h, !h->comm, "the reduce-buffer verbs are for handles without a communicator");
  NEED(h, !h->try_shortcut, "every camera is fixed: this try assembled no S (PSBA_FIXED_NO_SHORTCUT=1 keeps the general route)");
  if (!in) return fail(h, PSBA_E_INVALID, "null buffer");
  if (packed_hook(h)) {  // the summed packed sums: psba_schur_solve scatters them (k_schur_expand)
    PSBA_HIP(h, hipMemcpyAsync(h->redp, in, sizeof(double) * h->packed_doubles, hipMemcpyHostToDevice, h->stream));
    PSBA_HIP(h, hipStreamSynchronize(h->stream));
    h->packed_pending = true;
    h->diag_done = false;
    return PSBA_OK;
  }
  PSBA_HIP(h, hipMemcpyAsync(h->red, in, sizeof(double) * (size_t)(h->n32 + 1) * h->n32,
                             hipMemcpyHostToDevice, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  h->diag_done = false;  // S changed under the factor of its first diagonal block
  return PSBA_OK;
}

int psba_comm_rank(psba_handle h, int *nranks, int *rank) {
  CHECK_H(h);
  if (nranks) *nranks = h->nranks;
  if (rank) *rank = h->rank;
  return PSBA_OK;
}

// ---- measurement ------------------------------------------------------------------------

static int prof_flush(psba_ctx *h) {
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  for (size_t k = 0; k < h->spans_used; k++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->spans[k].a, h->spans[k].b) == hipSuccess) {
      h->prof_ms[h->spans[k].kind] += ms;
      h->prof_n[h->spans[k].kind]++;
    }
  }
  h->spans_used = 0;
  return PSBA_OK;
}

int psba_profile_enable(psba_handle h, int on) {
  CHECK_H(h);
  TRY(prof_flush(h));
  h->prof = on < 0 ? ~0u : (unsigned)on;  // negative: every class; otherwise a bit mask of classes
  // event pairs are created here, not in front of the first profiled launches (hipEventCreate is
  // not cheap, and those launches may be the ones being timed)
  while (h->prof && h->spans.size() < 512) {
    psba_ctx::Span s;
    s.kind = 0;
    // timing events only: without the system-scope fence a default event carries (it flushes
    // caches between the kernels it sits between, and costs several microseconds itself)
    if (hipEventCreateWithFlags(&s.a, hipEventDisableSystemFence) != hipSuccess ||
        hipEventCreateWithFlags(&s.b, hipEventDisableSystemFence) != hipSuccess)
      break;
    h->spans.push_back(s);
  }
  return PSBA_OK;
}

int psba_profile_reset(psba_handle h) {
  CHECK_H(h);
  TRY(prof_flush(h));
  for (int k = 0; k < PSBA_K_COUNT; k++) {
    h->prof_ms[k] = 0;
    h->prof_n[k] = 0;
  }
  return PSBA_OK;
}

int psba_profile_get(psba_handle h, int kernel, double *total_ms, int *launches) {
  CHECK_H(h);
  if (kernel < 0 || kernel >= PSBA_K_COUNT) return fail(h, PSBA_E_INVALID, "bad kernel class");
  TRY(prof_flush(h));
  if (total_ms) *total_ms = h->prof_ms[kernel];
  if (launches) *launches = h->prof_n[kernel];
  return PSBA_OK;
}

int psba_algorithmic_bytes(psba_handle h, int kernel, double *bytes) {
  CHECK_H(h);
  NEED(h, h->uploaded, "no problem uploaded");
  const double nO = h->d.nO, nP = h->d.nP, nC = h->d.nC, nA = h->d.nA;
  double b = 0;
  switch (kernel) {
    case PSBA_K_LINEARIZE:
      b = nO * (16 + 8 + 144) + nP * (24 + 72 + 24) + nC * (120 + 288 + 48);
      break;
    case PSBA_K_SCHUR:  // SURVEY 8(d) K2, S counted once as the full square
      b = nO * (144 + 8) + nP * (72 + 24) + nC * (288 + 48) + 8 * nA * nA + 8 * nA;
      break;
    case PSBA_K_BACKSUB:  // SURVEY 8(d) K3 incl. the fused new-cost pass
      b = nO * 152 + nP * (72 + 24 + 24 + 24) + nA * 8 + nO * 24 + 8;
      break;
    case PSBA_K_CHOLESKY:
      b = 8 * nA * nA;
      break;
    case PSBA_K_RESIDUAL:
      b = nO * 24 + nP * 24 + nC * 120 + 8;
      break;
    default:
      return fail(h, PSBA_E_INVALID, "no byte model for kernel class %d", kernel);
  }
  if (bytes) *bytes = b;
  return PSBA_OK;
}

// ---- test hook: K2's static schedule without a device ----
struct psba_schur_plan {
  psba_ctx ctx;  // only the plan fields are used; no HIP call is made through it
  psba::SchurPlanHost plan;
  long long nBlocks = 0;
};

psba_schur_plan_t psba_schur_plan_create(int nCams, int n3Dpts, int n2Dprojs, const int *iidx,
                                         const int *jidx) {
  if (nCams <= 0 || n3Dpts <= 0 || n2Dprojs <= 0 || !iidx || !jidx) return nullptr;
  std::vector<int> ptr((size_t)n3Dpts + 1, 0);
  for (int a = 0; a < n2Dprojs; a++) {
    if (iidx[a] < 0 || iidx[a] >= n3Dpts || jidx[a] < 0 || jidx[a] >= nCams) return nullptr;
    // point-major, cameras ascending inside a point, as psba_upload_problem requires
    if (a && (iidx[a] < iidx[a - 1] || (iidx[a] == iidx[a - 1] && jidx[a] <= jidx[a - 1]))) return nullptr;
    ptr[(size_t)iidx[a] + 1]++;
  }
  for (int i = 0; i < n3Dpts; i++) ptr[(size_t)i + 1] += ptr[i];
  psba_schur_plan *p = new (std::nothrow) psba_schur_plan;
  if (!p) return nullptr;
  p->nBlocks = (long long)nCams * (nCams + 1) / 2;
  if (psba::build_schur_plan(&p->ctx, nCams, n3Dpts, n2Dprojs, iidx, jidx, ptr.data(), p->plan) != PSBA_OK) {
    delete p;
    return nullptr;
  }
  return p;
}

int psba_schur_plan_info(psba_schur_plan_t p, long long info[8]) {
  if (!p || !info) return PSBA_E_INVALID;
  info[0] = p->ctx.nGroups;
  info[1] = p->ctx.nGroups ? p->ctx.nWg : 0;
  info[2] = (long long)p->plan.items.size();
  info[3] = p->plan.real_items;
  info[4] = (long long)p->plan.slab_doubles;
  info[5] = p->nBlocks;
  info[6] = p->plan.runs ? p->plan.tasks : 0;  // > 0: the runs layout ([turn][512] per workgroup), number of runs
  info[7] = p->plan.pair_items;                // items that carry two products of one observation
  return PSBA_OK;
}

int psba_schur_plan_copy(psba_schur_plan_t p, unsigned long long *items, long long *wg, int *blockpos,
                         int *glo) {
  if (!p) return PSBA_E_INVALID;
  if (items) std::copy(p->plan.items.begin(), p->plan.items.end(), items);
  if (wg)
    for (size_t k = 0; k < p->plan.wgs.size(); k++) {
      const psba::SchurWg &w = p->plan.wgs[k];
      long long *o = wg + 8 * k;
      o[0] = w.group; o[1] = w.nblk; o[2] = w.obs0; o[3] = w.pt0;
      o[4] = w.item0; o[5] = w.item1; o[6] = (long long)w.slab_off; o[7] = w.itemD;
    }
  if (blockpos) std::copy(p->plan.blockpos.begin(), p->plan.blockpos.end(), blockpos);
  if (glo)  // block ranges: group g owns the blocks [glo[g], glo[g + 1]) of the canonical order tri(j) + k
    for (int g = 0; g <= p->ctx.nGroups; g++) glo[g] = p->ctx.gblk0[g];
  return PSBA_OK;
}

void psba_schur_plan_destroy(psba_schur_plan_t p) { delete p; }

// ---- test hook: the owner route's product lists (many cameras, long tracks, block-sparse S), host only ----
struct psba_owner_plan {
  psba::OwnerPlanHost plan;
};

psba_owner_plan_t psba_owner_plan_create(int nCams, int n3Dpts, int n2Dprojs, const int *iidx, const int *jidx,
                                         const unsigned char *pattern) {
  if (nCams <= 0 || n3Dpts <= 0 || n2Dprojs <= 0 || !iidx || !jidx) return nullptr;
  std::vector<int> ptr((size_t)n3Dpts + 1, 0);
  for (int a = 0; a < n2Dprojs; a++) {
    if (iidx[a] < 0 || iidx[a] >= n3Dpts || jidx[a] < 0 || jidx[a] >= nCams) return nullptr;
    // point-major, cameras ascending inside a point, as psba_upload_problem requires
    if (a && (iidx[a] < iidx[a - 1] || (iidx[a] == iidx[a - 1] && jidx[a] <= jidx[a - 1]))) return nullptr;
    ptr[(size_t)iidx[a] + 1]++;
  }
  for (int i = 0; i < n3Dpts; i++) ptr[(size_t)i + 1] += ptr[i];
  psba_owner_plan *p = new (std::nothrow) psba_owner_plan;
  if (!p) return nullptr;
  if (psba::build_owner_plan(nCams, n2Dprojs, iidx, jidx, ptr.data(), p->plan, pattern) != PSBA_OK) {
    delete p;
    return nullptr;
  }
  return p;
}

int psba_owner_plan_info(psba_owner_plan_t p, long long info[4]) {
  if (!p || !info) return PSBA_E_INVALID;
  info[0] = (long long)p->plan.waves.size();
  info[1] = (long long)p->plan.prod.size() / 64;  // ELL rows
  info[2] = p->plan.products;
  info[3] = (long long)p->plan.blocks.size();
  return PSBA_OK;
}

int psba_owner_plan_copy(psba_owner_plan_t p, long long *waves, int *units, int *prod, int *blocks, int *diag_slot) {
  if (!p) return PSBA_E_INVALID;
  if (waves)
    for (size_t w = 0; w < p->plan.waves.size(); w++) {
      waves[2 * w] = p->plan.waves[w].row0;
      waves[2 * w + 1] = p->plan.waves[w].len;
    }
  if (units)
    for (size_t u = 0; u < p->plan.units.size(); u++) {
      units[4 * u] = p->plan.units[u].j;
      units[4 * u + 1] = p->plan.units[u].k;
      units[4 * u + 2] = p->plan.units[u].multi;
      units[4 * u + 3] = p->plan.units[u].slot;
    }
  if (prod)
    for (size_t t = 0; t < p->plan.prod.size(); t++) {
      prod[2 * t] = p->plan.prod[t].x;
      prod[2 * t + 1] = p->plan.prod[t].y;
    }
  if (blocks)
    for (size_t b = 0; b < p->plan.blocks.size(); b++) {
      blocks[2 * b] = p->plan.blocks[b].x;
      blocks[2 * b + 1] = p->plan.blocks[b].y;
    }
  if (diag_slot) std::copy(p->plan.diag_slot.begin(), p->plan.diag_slot.end(), diag_slot);
  return PSBA_OK;
}

void psba_owner_plan_destroy(psba_owner_plan_t p) { delete p; }

#ifdef PSBA_BUILD_EXPERIMENTS
// ---- test hook: the ring route's schedule (schur_ring_plan.cpp), host only ----
struct psba_ring_plan {
  psba::RingPlanHost plan;
};

psba_ring_plan_t psba_ring_plan_create(int nCams, int n3Dpts, int n2Dprojs, const int *iidx, const int *jidx) {
  if (nCams <= 0 || n3Dpts <= 0 || n2Dprojs <= 0 || !iidx || !jidx) return nullptr;
  std::vector<int> ptr((size_t)n3Dpts + 1, 0);
  for (int a = 0; a < n2Dprojs; a++) {
    if (iidx[a] < 0 || iidx[a] >= n3Dpts || jidx[a] < 0 || jidx[a] >= nCams) return nullptr;
    if (a && (iidx[a] < iidx[a - 1] || (iidx[a] == iidx[a - 1] && jidx[a] <= jidx[a - 1]))) return nullptr;
    ptr[(size_t)iidx[a] + 1]++;
  }
  for (int i = 0; i < n3Dpts; i++) ptr[(size_t)i + 1] += ptr[i];
  psba_ring_plan *p = new (std::nothrow) psba_ring_plan;
  if (!p) return nullptr;
  if (psba::build_ring_plan(nCams, n3Dpts, n2Dprojs, iidx, jidx, ptr.data(), p->plan, true) != PSBA_OK) {
    delete p;
    return nullptr;
  }
  return p;
}

int psba_ring_plan_info(psba_ring_plan_t p, long long info[16]) {
  if (!p || !info) return PSBA_E_INVALID;
  const psba::RingPlanHost &q = p->plan;
  info[0] = q.nR;
  info[1] = q.nS;
  info[2] = q.nWg;
  info[3] = (long long)q.steps.size();
  info[4] = (long long)q.entries.size();
  info[5] = (long long)q.ops.size() / 2;
  info[6] = (long long)q.jobs.size();  // (each list ends in a few entries of slack the kernel may read but never uses)
  info[7] = q.products;
  info[8] = q.slots;
  info[9] = psba::RING_LANES;
  info[10] = psba::RING_SLOTS;
  info[11] = psba::RING_PAGE;
  info[12] = q.lat;
  info[13] = (long long)q.lane_blk.size();
  info[14] = (long long)q.blk_lane0.size();
  info[15] = q.loaded_recs;
  return PSBA_OK;
}

int psba_ring_plan_copy(psba_ring_plan_t p, long long *wg, int *steps, unsigned *entries, int *ops, int *jobs,
                        int *lane_blk, int *blk_lane0, int *rb) {
  if (!p) return PSBA_E_INVALID;
  const psba::RingPlanHost &q = p->plan;
  if (wg)
    for (size_t k = 0; k < q.wgs.size(); k++) {
      const psba::RingWg &w = q.wgs[k];
      long long *o = wg + 13 * k;
      o[12] = w.nwslots;
      o[0] = w.blk0; o[1] = w.nblk; o[2] = w.row0; o[3] = w.nrows; o[4] = w.copy; o[5] = w.nsteps;
      o[6] = w.step0; o[7] = w.ent0; o[8] = w.op0; o[9] = w.job0; o[10] = w.lane0; o[11] = w.bl0;
    }
  if (steps)
    for (size_t k = 0; k < q.steps.size(); k++) {
      steps[4 * k] = q.steps[k].op_begin; steps[4 * k + 1] = q.steps[k].op_end;
      steps[4 * k + 2] = q.steps[k].job_begin; steps[4 * k + 3] = q.steps[k].job_end;
    }
  if (entries) std::copy(q.entries.begin(), q.entries.end(), entries);
  if (ops) std::copy(q.ops.begin(), q.ops.end(), ops);
  if (jobs)
    for (size_t k = 0; k < q.jobs.size(); k++) {
      jobs[4 * k] = q.jobs[k].obs; jobs[4 * k + 1] = q.jobs[k].point;
      jobs[4 * k + 2] = q.jobs[k].slots; jobs[4 * k + 3] = q.jobs[k].earow;
    }
  if (lane_blk) std::copy(q.lane_blk.begin(), q.lane_blk.end(), lane_blk);
  if (blk_lane0) std::copy(q.blk_lane0.begin(), q.blk_lane0.end(), blk_lane0);
  if (rb) std::copy(q.rb.begin(), q.rb.end(), rb);
  return PSBA_OK;
}

void psba_ring_plan_destroy(psba_ring_plan_t p) { delete p; }
#endif  // PSBA_BUILD_EXPERIMENTS

}  // extern "C"
