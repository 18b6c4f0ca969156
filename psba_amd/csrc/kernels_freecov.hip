// kernels_freecov.hip -- covariance of the refined cameras and points with free intrinsics.
//
// Definition (the same text in include/psba_hip.h and DESIGN 7l).  The covariance is taken at the current parameters,
// on the linearization of psba_linearize(h, 1, 1).  That linearization is exactly what the route's normal equations
// see: the intrinsics mask, the groups, held poses and points, the priors' information in U and V, blocks weighted by
// omega / sigma.  Let N be that system and D the diagonal of psba_set_damping (I for the identity rule).  For mu >= 0
// and scale > 0 the covariance is built in three steps.
//   reduced camera part   X = S(mu)^-1 on the live coordinates of the folded S.  A live coordinate is not masked, is
//                         not a held pose coordinate, is not folded away by the groups, and is not padding
//   returned camera part  C_aa = scale E X E^T, where E copies a representative's shared intrinsic to the members of
//                         its group: rows and columns of masked and held coordinates are exactly 0 (not the inverse
//                         of the placeholder); a folded-away coordinate's row and column are bit-identical to its
//                         representative's, because shared intrinsics are perfectly correlated; C_aa is bit-symmetric
//   point i               C_bb,i = scale V*_i^-1 + sum_{j,k in cams(i)} Y_ij^T C_jk Y_ik, with the expanded C_aa,
//                         V*_i = V_i + mu D_i and Y_ij the block that k_free_Y stored for this mu.  A held point gives
//                         zeros; a point without observations, and one whose blocks Y are all zero, scale V*^-1
// mu = 0 is the covariance and needs a gauge: held poses or priors.  mu > 0 is a regularised inverse and not a
// covariance.  The cross blocks C_ab are not returned.  PARITY UNPINNED, as in 7h.
//
// Route.  The factorization and the inverse are those of kernels_cov.hip (k_cov_diag, k_cov_trsm, k_cov_update,
// k_cov_inverse, launched by launch_cov_factor / launch_cov_inverse), unchanged, between a compaction and a finish of
// this file.  Both read one table src[nA]: -1 for a masked or held coordinate, the coordinate itself when it is live,
// the representative's coordinate for one that is folded away.
//   k_fcov_map      the table, from the mask, the held poses and the groups (kd_folded)
//   k_fcov_compact  S with the identity on every row and column with src[r] != r and on the padding
//   k_fcov_finish   C[r][c] = scale X[src r][src c], 0 where either source is -1; reads the lower triangle of X and
//                   writes another buffer (the expansion reads entries other threads own), one thread both mirrors
//   k_fcov_points   one wave per point, any track length.  Z_j = sum_k C_jk Y_k on the matrix pipe
//                   (v_mfma_f64_16x16x4_f64; operand layout: top of kernels_free.hip): C_jk is the A operand, read
//                   through C_kj (C is bit-symmetric) so that the 16 lanes of a row group read consecutive addresses,
//                   Y_k the B operand (columns 3..15 supply 0.0); K goes over the block in steps of 4 and the
//                   accumulator chain runs in ascending k.  For blocks of 11, rows and columns >= 11 supply 0.0, as in
//                   k_free_schur.  Y_j^T Z_j is summed through LDS in ascending j (the six entries a <= b; the others
//                   are copies), COV_FJC cameras staged at a time.  V* is rebuilt with the route's own damping
//                   (damp_point_block under Marquardt) and sym3_inverse; Y is read, not recomputed
// No floating-point atomics: every sum is in an order that the upload fixes, two computes are bit-identical.
#include "camera_model.h"
#include "free_blocks.h"
#include "psba_internal.h"

namespace psba {

constexpr int COV_FJC = 32;  // cameras of a point whose rows Z_j are staged in LDS at a time (COV_JC of kernels_cov.hip)

#define FCOV_LAUNCHED(h)                                                                                            \
  do {                                                                                                              \
    hipError_t e__ = hipGetLastError();                                                                             \
    if (e__ != hipSuccess) return fail((h), PSBA_E_HIP, "covariance kernel launch failed: %s", hipGetErrorString(e__)); \
  } while (0)
#define FCOV_TRY(expr)         \
  do {                         \
    int rc__ = (expr);         \
    if (rc__ < 0) return rc__; \
  } while (0)

// ---- the coordinate map: one thread per coordinate of the camera part (rep and held_pose may be null: none) ----
template <class T>
__global__ __launch_bounds__(256) void k_fcov_map(KdGroups G, const unsigned char *held_pose, int nA, int *src) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nA) return;
  const int j = t / T::CNP, k = t % T::CNP;
  int s = t;
  if (k < T::NI ? !((G.mask >> k) & 1u) : (held_pose && held_pose[j]))
    s = -1;
  else if (T::CNP == KD_CNP && G.rep && kd_folded(G, t))
    s = KD_CNP * G.rep[j] + k;
  src[t] = s;
}

// ---- M = S with the identity on the rows and columns that are not live (src[r] != r) and on the padding ----
__global__ __launch_bounds__(256) void k_fcov_compact(const double *S, double *M, const int *src, int nA, int n32) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n32 * n32) return;
  const int r = (int)(t / n32), c = (int)(t % n32);
  const bool dead = r >= nA || c >= nA || src[r] != r || src[c] != c;
  M[t] = dead ? (r == c ? 1.0 : 0.0) : S[t];
}

// ---- C = scale E X E^T from the lower triangle of X; the padding's rows and columns are zero as well ----
__global__ __launch_bounds__(256) void k_fcov_finish(const double *X, double *C, const int *src, int nA, int n32, double scale) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n32 * n32) return;
  const int r = (int)(t / n32), c = (int)(t % n32);
  if (c > r) return;
  const int sr = r < nA ? src[r] : -1, sc = c < nA ? src[c] : -1;
  double v = 0.0;
  if (sr >= 0 && sc >= 0) v = scale * X[(size_t)max(sr, sc) * n32 + min(sr, sc)];
  C[t] = v;
  C[(size_t)c * n32 + r] = v;
}

// ---- the blocks C_jk of a list of camera pairs: one workgroup per pair ----
__global__ __launch_bounds__(256) void k_fcov_gather(const double *C, int ld, const int2 *pairs, int n_pairs, int cnp, double *out) {
  const int q = blockIdx.x;
  if (q >= n_pairs) return;
  const int2 jk = pairs[q];
  for (int t = threadIdx.x; t < cnp * cnp; t += 256)
    out[(size_t)cnp * cnp * q + t] = C[(size_t)(cnp * jk.x + t / cnp) * ld + cnp * jk.y + t % cnp];
}

// ---- the standard deviations: sqrt of the diagonal of C_aa, then of the three diagonal entries of every C_bb,i ----
__global__ __launch_bounds__(256) void k_fcov_sigmas(const double *C, int ld, const double *pts, int nA, int nT, double *sigma) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nT) return;
  const double v = t < nA ? C[(size_t)t * ld + t] : pts[9 * (size_t)((t - nA) / 3) + 4 * ((t - nA) % 3)];
  sigma[t] = __dsqrt_rn(v);
}

// ---- one wave per point: C_bb,i = scale V*^-1 + sum_j Y_j^T (sum_k C_jk Y_k) ----
template <class T>
__global__ __launch_bounds__(64) void k_fcov_points(const double *PV, const double *Y, const int *ptr, const int *jidx,
                                                    const unsigned char *held_pt, const double *C, int ld, double mu,
                                                    int marquardt, double dmin, double dmax, double scale, double *out,
                                                    int *status) {
  constexpr int CNP = T::CNP, WB = 3 * CNP, KS = (CNP + 3) / 4;
  __shared__ double sZ[COV_FJC * WB];
  const int i = blockIdx.x, lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  double *o = out + 9 * (size_t)i;
  if (held_pt && held_pt[i]) {  // (uniform over the wave)
    if (lane < 9) o[lane] = 0.0;
    return;
  }
  const int o0 = ptr[i], m = ptr[i + 1] - o0;
  const double *pv = PV + 9 * (size_t)i;
  double v[6], vi[6];
#pragma unroll
  for (int q = 0; q < 6; q++) v[q] = pv[q];
  if (marquardt) {
    damp_point_block(v, mu, dmin, dmax);
  } else {
    v[0] += mu;
    v[3] += mu;
    v[5] += mu;
  }
  if (sym3_inverse(v, vi) && lane == 0) status[1] = 1;
  // lanes 0..5 own the entries (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) -- the packing of vi
  const int ea = lane < 3 ? 0 : lane < 5 ? 1 : 2, eb = lane < 3 ? lane : lane < 5 ? lane - 2 : 2;
  // A operand: row `col` of C_jk; B operand: column `col` of Y_k (a lane outside the block or the three columns reads
  // entry 0 and supplies 0.0: the load may be issued ahead of the select)
  const bool alive = CNP == 16 || col < CNP, blive = col < 3;
  const int acol = alive ? col : 0, bcol = blive ? col : 0;
  double acc = 0.0;
  for (int j0 = 0; j0 < m; j0 += COV_FJC) {
    const int jn = min(COV_FJC, m - j0);
    // two cameras j per pass share the B operands: two independent accumulator chains, each in ascending k (an odd
    // last camera runs as a pair with itself and its second result is not stored)
    for (int jj = 0; jj < jn; jj += 2) {
      const bool two = jj + 1 < jn;
      const size_t cjo0 = (size_t)CNP * jidx[o0 + j0 + jj] + acol;  // C_jk[row][q] read as C_kj[q][row]
      const size_t cjo1 = two ? (size_t)CNP * jidx[o0 + j0 + jj + 1] + acol : cjo0;
      kd4 z0 = {0.0, 0.0, 0.0, 0.0}, z1 = {0.0, 0.0, 0.0, 0.0};
      for (int kc = 0; kc < m; kc++) {
        const double *ck = C + (size_t)(CNP * jidx[o0 + kc]) * ld, *yk = Y + WB * (size_t)(o0 + kc) + bcol;
        double a0[KS], a1[KS], b[KS];
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
          const int q = 4 * kk + kq;
          const bool qlive = CNP == 16 || q < CNP;
          const int qc = qlive ? q : 0;
          a0[kk] = ck[(size_t)qc * ld + cjo0];
          a1[kk] = ck[(size_t)qc * ld + cjo1];
          b[kk] = yk[3 * qc];
          if (!qlive || !alive) a0[kk] = a1[kk] = 0.0;
          if (!qlive || !blive) b[kk] = 0.0;
        }
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
          z0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[kk], b[kk], z0, 0, 0, 0);
          z1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[kk], b[kk], z1, 0, 0, 0);
        }
      }
      if (blive) {
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (CNP == 16 || kq + 4 * r < CNP) {
            sZ[WB * jj + 3 * (kq + 4 * r) + col] = z0[r];
            if (two) sZ[WB * (jj + 1) + 3 * (kq + 4 * r) + col] = z1[r];
          }
      }
    }
    __syncthreads();
    if (lane < 6)
      for (int jj = 0; jj < jn; jj++) {
        const double *yj = Y + WB * (size_t)(o0 + j0 + jj);
#pragma unroll
        for (int p = 0; p < CNP; p++) acc += yj[3 * p + ea] * sZ[WB * jj + 3 * p + eb];
      }
    __syncthreads();
  }
  if (lane < 6) {
    const double r = scale * vi[lane] + acc;
    o[3 * ea + eb] = r;
    o[3 * eb + ea] = r;
  }
}

// ---- host side ----
// S (the n32 x n32 head of the reduce buffer) -> fcov_C = scale E S^-1 E^T.  ev (may be null): three events recorded
// before the factor, between factor and inverse, and behind the finish
int launch_fcov_cameras(psba_ctx *h, double scale, hipEvent_t *ev) {
  const int n32 = h->n32, nA = h->d.nA;
  const size_t nn = (size_t)n32 * n32;
  FCOV_TRY(cov_workspaces(h));
  if (!h->fcov_C) FCOV_TRY(h->fcov_C.alloc(h, nn));
  if (!h->fcov_src) FCOV_TRY(h->fcov_src.alloc(h, (size_t)nA));
  KdGroups G;
  G.rep = h->kd_rep;
  G.gidx = h->kd_gidx;
  G.gptr = h->kd_gptr;
  G.gmem = h->kd_gmem;
  G.nmg = h->kd_nmg;
  G.mask = h->kd_mask;
  const unsigned char *hp = h->has_held ? (const unsigned char *)h->held_poses : nullptr;
  const unsigned nb = (unsigned)((nn + 255) / 256), na = (unsigned)((nA + 255) / 256);
  hipStream_t s = h->stream;
  if (h->cnp == KD_CNP)
    k_fcov_map<FreeKD><<<na, 256, 0, s>>>(G, hp, nA, h->fcov_src);
  else
    k_fcov_map<FreeK><<<na, 256, 0, s>>>(G, hp, nA, h->fcov_src);
  if (ev) PSBA_HIP(h, hipEventRecord(ev[0], s));
  k_fcov_compact<<<nb, 256, 0, s>>>(h->red, h->cov_L, h->fcov_src, nA, n32);
  FCOV_LAUNCHED(h);
  FCOV_TRY(launch_cov_factor(h));
  if (ev) PSBA_HIP(h, hipEventRecord(ev[1], s));
  FCOV_TRY(launch_cov_inverse(h));
  k_fcov_finish<<<nb, 256, 0, s>>>(h->cov_C, h->fcov_C, h->fcov_src, nA, n32, scale);
  FCOV_LAUNCHED(h);
  if (ev) PSBA_HIP(h, hipEventRecord(ev[2], s));
  return PSBA_OK;
}

// the point blocks from the stored V, the Y of the last assemble and fcov_C
int launch_fcov_points(psba_ctx *h, double mu, double scale) {
  const Dims &d = h->d;
  if (!h->cov_pts) FCOV_TRY(h->cov_pts.alloc(h, (size_t)9 * d.nP));
  const unsigned char *hq = h->has_held ? (const unsigned char *)h->held_pts : nullptr;
  const int marq = h->damp_kind == PSBA_DAMPING_MARQUARDT ? 1 : 0;
  if (h->cnp == KD_CNP)
    k_fcov_points<FreeKD><<<d.nP, 64, 0, h->stream>>>(h->PV, h->free_Y, h->ptr, h->jidx, hq, h->fcov_C, h->n32, mu, marq,
                                                      h->damp_dmin, h->damp_dmax, scale, h->cov_pts, h->cov_status);
  else
    k_fcov_points<FreeK><<<d.nP, 64, 0, h->stream>>>(h->PV, h->free_Y, h->ptr, h->jidx, hq, h->fcov_C, h->n32, mu, marq,
                                                     h->damp_dmin, h->damp_dmax, scale, h->cov_pts, h->cov_status);
  FCOV_LAUNCHED(h);
  return PSBA_OK;
}

// the blocks C_jk of n_pairs camera pairs (device list) into out_dev [n_pairs][cnp^2]
int launch_fcov_gather(psba_ctx *h, const int2 *pairs_dev, int n_pairs, double *out_dev) {
  k_fcov_gather<<<n_pairs, 256, 0, h->stream>>>(h->fcov_C, h->n32, pairs_dev, n_pairs, h->cnp, out_dev);
  FCOV_LAUNCHED(h);
  return PSBA_OK;
}

// sigma_dev [nT]: the square roots of the diagonals of fcov_C and of the point blocks
int launch_fcov_sigmas(psba_ctx *h, double *sigma_dev) {
  k_fcov_sigmas<<<(unsigned)((h->d.nT + 255) / 256), 256, 0, h->stream>>>(h->fcov_C, h->n32, h->cov_pts, h->d.nA, h->d.nT, sigma_dev);
  FCOV_LAUNCHED(h);
  return PSBA_OK;
}

}  // namespace psba
