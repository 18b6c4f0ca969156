// kernels_cov.hip -- covariance of the refined cameras and points on the dense routes: six-parameter blocks
// and free intrinsics, blocks of 11 and 16.  One camera part for both, two point kernels.
//
// Definition, six-parameter blocks (the same text in include/psba_hip.h and DESIGN 7h).  The covariance is taken at
// the current parameters and uses the linearization of psba_linearize(h, 1, 1): whitened, loss-weighted and masked by
// psba_set_fixed, i.e. exactly what the normal equations see.  N = J^T J on the free blocks.  For mu >= 0 and scale > 0,
//   C = scale (N + mu I)^-1 on the free entries, zero on rows and columns of fixed blocks
// (not the inverse of the placeholder).  Through the Schur complement:
//   cameras   C_aa = scale S(mu)^-1; rows and columns of fixed cameras are removed and returned as zeros
//   point i   C_bb,i = scale V*_i^-1 + sum_{j,k in cams(i)} Y_ij^T C_jk Y_ik,  Y_ij = W_ij V*_i^-1,  V*_i = V_i + mu I
//             (ordered pairs of the point's free cameras, j == k included); a fixed point gives zeros, a point whose
//             cameras are all fixed gives scale V*_i^-1; with every camera fixed no S is assembled and C_aa = 0
// The cross blocks C_ab are not returned.  mu = 0 is the true covariance and needs the gauge fixed (two fixed cameras;
// DESIGN 7c shows S is positive definite then); mu > 0 gives a regularised inverse, which is not a covariance.
// PARITY UNPINNED: the reference's SPDinv inverse is an intermediate of its solve and is never returned.
//
// Definition, free intrinsics (the same text in include/psba_hip.h and DESIGN 7l).  The covariance is taken at the
// current parameters, on the linearization of psba_linearize(h, 1, 1).  That linearization is exactly what the route's
// normal equations see: the intrinsics mask, the groups, held poses and points, the priors' information in U and V,
// blocks weighted by omega / sigma.  Let N be that system and D the diagonal of psba_set_damping (I for the identity
// rule).  For mu >= 0 and scale > 0 the covariance is built in three steps.
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
// covariance.  The cross blocks C_ab are not returned.  PARITY UNPINNED, as above.
//
// Route.  The camera part works on two private n32 x n32 squares (the identity padding rows of the reduce buffer make
// every 16 x 16 tile full) and never touches the Cholesky chain or its factor.  All bulk arithmetic is
// v_mfma_f64_16x16x4_f64 (operand layout: top of kernels_free.hip -- A operand A[l & 15][l >> 4], B operand
// B[l >> 4][l & 15], C/D col = l & 15, row = (l >> 4) + 4 reg); a 16 x 16 x 16 tile product is four of them.
//   0 map         one table src[nA] says what a coordinate is: -1 fixed, masked or held; itself when it is live; the
//                 representative's coordinate when the groups fold it away (blocks of 16 only).  Six-parameter blocks:
//                 from psba_set_fixed; free intrinsics: from the mask, the held poses and the groups (kd_folded)
//   1 compaction  S with the identity on every row and column with src[r] != r and on the padding
//   2 factor      right-looking blocked Cholesky on 16 x 16 tiles, three kernels per panel: one wave factors the
//                 diagonal tile and stores the inverse of its factor (status on a pivot that is not positive and finite);
//                 one wave per tile below forms X = C L_dd^-T; one wave per trailing tile C -= X_r X_c^T
//   3 inverse     one workgroup per 16-column strip of the identity: L X = E forward (block rows at or below the
//                 strip's own block only), L^T C = X backward; a block row is an MFMA accumulation over the earlier
//                 block rows -- four waves take the rows kb = first + w, first + w + 4, ... in ascending order and
//                 their four partial tiles are added in wave order -- then one product with the stored diagonal
//                 inverse.  The lower triangle of the second square is the inverse X
//   4 finish      C[r][c] = scale X[max(sr, sc)][min(sr, sc)] with sr = src[r], sc = src[c]; 0 where either is -1 and
//                 on the padding.  One thread writes both mirrors.  Never in place (the expansion over the groups
//                 reads entries other threads own): it writes over the factor, which is dead behind the inverse
//   5 points      one wave per point, two kernels that sum in different orders.  k_cov_points (blocks of 6): V*_i and
//                 Y_ij from the stored linearization, then the 3 x 3 sum j-major with k ascending (only the six
//                 entries a <= b are summed, the others are their copies).  k_fcov_points<FreeK | FreeKD>: any track
//                 length, Z_j = sum_k C_jk Y_k on the matrix pipe: C_jk is the A operand, read through C_kj (C is
//                 bit-symmetric) so that the 16 lanes of a row group read consecutive addresses, Y_k the B operand
//                 (columns 3..15 supply 0.0); K goes over the block in steps of 4 and the accumulator chain runs in
//                 ascending k.  For blocks of 11, rows and columns >= 11 supply 0.0, as in k_free_schur.  Y_j^T Z_j
//                 is summed through LDS in ascending j, COV_FJC cameras staged at a time.  V* is rebuilt with the
//                 route's own damping (damp_point_block under Marquardt) and sym3_inverse; Y is read, not recomputed
// No floating-point atomics: every sum has an order fixed by the upload, two computes are bit-identical.
#include "api_common.h"
#include "camera_model.h"
#include "free_blocks.h"

namespace psba {

typedef double cv4 __attribute__((ext_vector_type(4)));
// cameras of a point whose rows Z_j = sum_k C_jk Y_k are staged in LDS at a time (k_cov_points, k_fcov_points)
constexpr int COV_JC = 32, COV_FJC = 32;

#define COV_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// ---- 0 the coordinate map: one thread per coordinate of the camera part ----
__global__ __launch_bounds__(256) void k_cov_map_six(const unsigned char *fix, int nA, int *src) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < nA) src[t] = fix && fix[t / 6] ? -1 : t;
}

// (rep and held_pose may be null: none)
template <class T>
__global__ __launch_bounds__(256) void k_cov_map_free(KdGroups G, const unsigned char *held_pose, int nA, int *src) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nA) return;
  const int j = t / T::CNP, k = t % T::CNP;
  int s = t;
  if (k < T::NI ? !((kd_free_bits(G.mask, G.cmask, j) >> k) & 1u) : (held_pose && held_pose[j]))
    s = -1;
  else if (T::CNP == KD_CNP && G.rep && kd_folded(G, t))
    s = KD_CNP * G.rep[j] + k;
  src[t] = s;
}

// ---- 1 compaction: M = S with the identity on the rows and columns that are not live (src[r] != r) and on the padding ----
__global__ __launch_bounds__(256) void k_cov_compact(const double *S, double *M, const int *src, int nA, int n32) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n32 * n32) return;
  const int r = (int)(t / n32), c = (int)(t % n32);
  const bool dead = r >= nA || c >= nA || src[r] != r || src[c] != c;
  M[t] = dead ? (r == c ? 1.0 : 0.0) : S[t];
}

// ---- 2a the diagonal tile of panel p: its Cholesky factor in place (upper part zero) and the factor's inverse ----
__global__ __launch_bounds__(64) void k_cov_diag(double *M, double *Dinv, int ld, int p, int *status) {
  __shared__ double a[16][17], inv[16][17];
  const int lane = threadIdx.x;
  double *T = M + (size_t)(16 * p) * ld + 16 * p;
  for (int t = lane; t < 256; t += 64) a[t >> 4][t & 15] = T[(size_t)(t >> 4) * ld + (t & 15)];
  __syncthreads();
  bool bad = false;
  for (int j = 0; j < 16; j++) {
    double d = a[j][j];
    if (!(d > 0.0) || !isfinite(d)) {  // (the same value in every lane: the branch is uniform)
      bad = true;
      d = 1.0;
    }
    const double l = sqrt(d);
    __syncthreads();
    if (lane >= j && lane < 16) a[lane][j] = lane == j ? l : a[lane][j] / l;
    __syncthreads();
    for (int t = lane; t < 256; t += 64) {
      const int r = t >> 4, c = t & 15;
      if (c > j && r >= c) a[r][c] -= a[r][j] * a[c][j];
    }
    __syncthreads();
  }
  if (bad && lane == 0) status[0] = 1;
  if (lane < 16) {  // column `lane` of the inverse by forward substitution
    const int c = lane;
    for (int r = 0; r < 16; r++) {
      double s = 0.0;
      if (r >= c) {
        s = r == c ? 1.0 : 0.0;
        for (int k = c; k < r; k++) s -= a[r][k] * inv[k][c];
        s /= a[r][r];
      }
      inv[r][c] = s;
    }
  }
  __syncthreads();
  for (int t = lane; t < 256; t += 64) {
    const int r = t >> 4, c = t & 15;
    T[(size_t)r * ld + c] = c <= r ? a[r][c] : 0.0;
    Dinv[256 * (size_t)p + t] = inv[r][c];
  }
}

// ---- 2b one wave per tile (R, p), R > p: X = C L_pp^-T in place ----
__global__ __launch_bounds__(64) void k_cov_trsm(double *M, const double *Dinv, int ld, int p) {
  const int lane = threadIdx.x, col = lane & 15, k = lane >> 4;
  const int R = p + 1 + blockIdx.x;
  double *T = M + (size_t)(16 * R) * ld + 16 * p;
  const double *Li = Dinv + 256 * (size_t)p;
  double a[4], b[4];
#pragma unroll
  for (int kk = 0; kk < 4; kk++) {
    a[kk] = T[(size_t)col * ld + 4 * kk + k];
    b[kk] = Li[16 * col + 4 * kk + k];
  }
  cv4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < 4; kk++) acc = COV_MFMA(a[kk], b[kk], acc);
#pragma unroll
  for (int r = 0; r < 4; r++) T[(size_t)(k + 4 * r) * ld + col] = acc[r];
}

// ---- 2c one wave per trailing tile (R, C), p < C <= R: C -= X_R X_C^T ----
__global__ __launch_bounds__(64) void k_cov_update(double *M, int ld, int p) {
  // workgroup t of the lower triangle, rows first: t = r (r + 1) / 2 + c, c <= r (the square root may be one off)
  const int t = blockIdx.x;
  int r = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= t) r++;
  while (r * (r + 1) / 2 > t) r--;
  const int R = p + 1 + r, C = p + 1 + (t - r * (r + 1) / 2);
  const int lane = threadIdx.x, col = lane & 15, k = lane >> 4;
  double *T = M + (size_t)(16 * R) * ld + 16 * C;
  const double *XR = M + (size_t)(16 * R) * ld + 16 * p, *XC = M + (size_t)(16 * C) * ld + 16 * p;
  // the 16 products of an entry are summed on their own and subtracted once: the tile's entries are far larger than
  // what the elimination leaves of them, and a running C - x0 y0 - x1 y1 - ... would round 16 times at their size
  cv4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < 4; kk++)
    acc = COV_MFMA(XR[(size_t)col * ld + 4 * kk + k], XC[(size_t)col * ld + 4 * kk + k], acc);
#pragma unroll
  for (int r = 0; r < 4; r++) T[(size_t)(k + 4 * r) * ld + col] -= acc[r];
}

// ---- 3 strip s of the inverse: forward L X = E_s, backward L^T C = X, block rows s .. NT - 1, in X's strip ----
__global__ __launch_bounds__(256) void k_cov_inverse(const double *L, const double *Dinv, double *X, int ld, int NT) {
  __shared__ double part[4][256], sum[256];
  const int s = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 15, k = lane >> 4;
  double *Xs = X + 16 * s;  // tile r of the strip: Xs + 16 r ld
  Xs[(size_t)(16 * s + (tid >> 4)) * ld + (tid & 15)] = Dinv[256 * (size_t)s + tid];  // X_s = L_ss^-1
  __syncthreads();
  for (int r = s + 1; r < NT; r++) {  // X_r = L_rr^-1 (-sum_{s <= kb < r} L_r,kb X_kb)
    cv4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int kb = s + w; kb < r; kb += 4) {
      const double *Lt = L + (size_t)(16 * r) * ld + 16 * kb, *Xt = Xs + (size_t)(16 * kb) * ld;
#pragma unroll
      for (int kk = 0; kk < 4; kk++)
        acc = COV_MFMA(Lt[(size_t)col * ld + 4 * kk + k], Xt[(size_t)(4 * kk + k) * ld + col], acc);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) part[w][16 * (k + 4 * q) + col] = acc[q];
    __syncthreads();
    sum[tid] = -(((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]);
    __syncthreads();
    if (w == 0) {
      const double *Li = Dinv + 256 * (size_t)r;
      cv4 x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < 4; kk++) x = COV_MFMA(Li[16 * col + 4 * kk + k], sum[16 * (4 * kk + k) + col], x);
#pragma unroll
      for (int q = 0; q < 4; q++) Xs[(size_t)(16 * r + k + 4 * q) * ld + col] = x[q];
    }
    __syncthreads();
  }
  for (int r = NT - 1; r >= s; r--) {  // C_r = L_rr^-T (X_r - sum_{kb > r} L_kb,r^T C_kb)
    cv4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int kb = r + 1 + w; kb < NT; kb += 4) {
      const double *Lt = L + (size_t)(16 * kb) * ld + 16 * r, *Ct = Xs + (size_t)(16 * kb) * ld;
#pragma unroll
      for (int kk = 0; kk < 4; kk++)
        acc = COV_MFMA(Lt[(size_t)(4 * kk + k) * ld + col], Ct[(size_t)(4 * kk + k) * ld + col], acc);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) part[w][16 * (k + 4 * q) + col] = acc[q];
    __syncthreads();
    sum[tid] = Xs[(size_t)(16 * r + (tid >> 4)) * ld + (tid & 15)] -
               (((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]);
    __syncthreads();
    if (w == 0) {
      const double *Li = Dinv + 256 * (size_t)r;
      cv4 x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < 4; kk++) x = COV_MFMA(Li[16 * (4 * kk + k) + col], sum[16 * (4 * kk + k) + col], x);
#pragma unroll
      for (int q = 0; q < 4; q++) Xs[(size_t)(16 * r + k + 4 * q) * ld + col] = x[q];
    }
    __syncthreads();
  }
}

// ---- 4 finish: C = scale E X E^T from the lower triangle of X; the padding's rows and columns are zero as well ----
__global__ __launch_bounds__(256) void k_cov_finish(const double *X, double *C, const int *src, int nA, int n32, double scale) {
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
__global__ __launch_bounds__(256) void k_cov_gather(const double *C, int ld, const int2 *pairs, int n_pairs, int cnp, double *out) {
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

// ---- 5 one wave per point: C_bb,i = scale V*^-1 + sum_j sum_k Y_j^T C_jk Y_k (C = null: structure only) ----
__global__ __launch_bounds__(64) void k_cov_points(const double *W, const double *PV, const int *ptr, const int *jidx,
                                                   const unsigned char *fix_pts, const double *C, int ld, double mu,
                                                   double scale, double *Y, double *out, int *status) {
  __shared__ double sZ[COV_JC * 18];
  const int i = blockIdx.x, lane = threadIdx.x;
  double *o = out + 9 * (size_t)i;
  if (fix_pts && fix_pts[i]) {
    if (lane < 9) o[lane] = 0.0;
    return;
  }
  const int o0 = ptr[i], m = ptr[i + 1] - o0;
  const double *pv = PV + 9 * (size_t)i;
  double v[6], vi[6];
#pragma unroll
  for (int q = 0; q < 6; q++) v[q] = pv[q];
  v[0] += mu;
  v[3] += mu;
  v[5] += mu;
  if (sym3_inverse(v, vi) && lane == 0) status[1] = 1;
  // lanes 0..5 own the entries (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) -- the packing of vi
  const int ea = lane < 3 ? 0 : lane < 5 ? 1 : 2, eb = lane < 3 ? lane : lane < 5 ? lane - 2 : 2;
  double acc = 0.0;
  if (C) {
    for (int t = lane; t < 6 * m; t += 64) {
      const size_t off = 18 * (size_t)(o0 + t / 6) + 3 * (t % 6);
      const double w0 = W[off], w1 = W[off + 1], w2 = W[off + 2];
      Y[off] = w0 * vi[0] + w1 * vi[1] + w2 * vi[2];
      Y[off + 1] = w0 * vi[1] + w1 * vi[3] + w2 * vi[4];
      Y[off + 2] = w0 * vi[2] + w1 * vi[4] + w2 * vi[5];
    }
    __syncthreads();
    for (int j0 = 0; j0 < m; j0 += COV_JC) {
      const int jn = min(COV_JC, m - j0);
      for (int t = lane; t < 18 * jn; t += 64) {  // Z_j[p][b] = sum_k (ascending) sum_q C_jk[p][q] Y_k[q][b]
        const int jj = t / 18, e = t % 18;
        const double *row = C + (size_t)(6 * jidx[o0 + j0 + jj] + e / 3) * ld;
        double z = 0.0;
        for (int kc = 0; kc < m; kc++) {
          const double *cb = row + 6 * jidx[o0 + kc], *yk = Y + 18 * (size_t)(o0 + kc) + e % 3;
#pragma unroll
          for (int q = 0; q < 6; q++) z += cb[q] * yk[3 * q];
        }
        sZ[t] = z;
      }
      __syncthreads();
      if (lane < 6)
        for (int jj = 0; jj < jn; jj++) {
          const double *yj = Y + 18 * (size_t)(o0 + j0 + jj);
#pragma unroll
          for (int p = 0; p < 6; p++) acc += yj[3 * p + ea] * sZ[18 * jj + 3 * p + eb];
        }
      __syncthreads();
    }
  }
  if (lane < 6) {
    const double r = scale * vi[lane] + acc;
    o[3 * ea + eb] = r;
    o[3 * eb + ea] = r;
  }
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
// S (the n32 x n32 head of the reduce buffer) -> cov_A = scale E S^-1 E^T (E = I without groups): map, compaction
// into cov_A, its Cholesky factor in place (cov_dinv; cov_status[0] on a bad pivot), the lower triangle of the inverse
// in cov_X, the finish back into cov_A.  A structure-only try (six-parameter blocks, every camera fixed) assembled no
// S: C_aa = 0.  ev (may be null): three events recorded before the factor, between factor and inverse, and at the end
int launch_cov_cameras(psba_ctx *h, double scale, hipEvent_t *ev) {
  const int n32 = h->n32, NT = n32 / 16, nA = h->d.nA;
  const size_t nn = (size_t)n32 * n32;
  hipStream_t s = h->stream;
  if (!h->cov_A) TRY(h->cov_A.alloc(h, nn));
  if (h->try_shortcut) {
    for (int k = 0; ev && k < 3; k++) PSBA_HIP(h, hipEventRecord(ev[k], s));
    PSBA_HIP(h, hipMemsetAsync(h->cov_A, 0, sizeof(double) * nn, s));
    return PSBA_OK;
  }
  if (!h->cov_X) TRY(h->cov_X.alloc(h, nn));
  if (!h->cov_dinv) TRY(h->cov_dinv.alloc(h, (size_t)256 * NT));
  if (!h->cov_src) TRY(h->cov_src.alloc(h, (size_t)nA));
  const unsigned nb = (unsigned)((nn + 255) / 256), na = (unsigned)((nA + 255) / 256);
  const unsigned char *hp = h->has_held ? (const unsigned char *)h->held_poses : nullptr;
  if (h->cnp == 6)
    k_cov_map_six<<<na, 256, 0, s>>>(h->fix_cams, nA, h->cov_src);
  else if (h->cnp == KD_CNP)
    k_cov_map_free<FreeKD><<<na, 256, 0, s>>>(kd_groups(h), hp, nA, h->cov_src);
  else
    k_cov_map_free<FreeK><<<na, 256, 0, s>>>(kd_groups(h), hp, nA, h->cov_src);
  if (ev) PSBA_HIP(h, hipEventRecord(ev[0], s));
  k_cov_compact<<<nb, 256, 0, s>>>(h->red, h->cov_A, h->cov_src, nA, n32);
  for (int p = 0; p < NT; p++) {
    k_cov_diag<<<1, 64, 0, s>>>(h->cov_A, h->cov_dinv, n32, p, h->cov_status);
    const int rest = NT - p - 1;
    if (rest > 0) {
      k_cov_trsm<<<rest, 64, 0, s>>>(h->cov_A, h->cov_dinv, n32, p);
      k_cov_update<<<rest * (rest + 1) / 2, 64, 0, s>>>(h->cov_A, n32, p);
    }
  }
  PSBA_HIP(h, hipGetLastError());
  if (ev) PSBA_HIP(h, hipEventRecord(ev[1], s));
  k_cov_inverse<<<NT, 256, 0, s>>>(h->cov_A, h->cov_dinv, h->cov_X, n32, NT);
  k_cov_finish<<<nb, 256, 0, s>>>(h->cov_X, h->cov_A, h->cov_src, nA, n32, scale);
  PSBA_HIP(h, hipGetLastError());
  if (ev) PSBA_HIP(h, hipEventRecord(ev[2], s));
  return PSBA_OK;
}

// the point blocks from the stored linearization and C_aa in cov_A.  Six-parameter blocks: Y is formed from W into
// cov_Y; after a structure-only try there is no C_aa to read and the blocks are scale V*^-1 alone.  Free intrinsics:
// the stored V, the Y of the last assemble (free_Y)
int launch_cov_points(psba_ctx *h, double mu, double scale) {
  const Dims &d = h->d;
  hipStream_t s = h->stream;
  if (!h->cov_pts) TRY(h->cov_pts.alloc(h, (size_t)9 * d.nP));
  if (h->cnp == 6) {
    const bool with_C = !h->try_shortcut;
    if (with_C && !h->cov_Y) TRY(h->cov_Y.alloc(h, (size_t)18 * d.nO));
    k_cov_points<<<d.nP, 64, 0, s>>>(h->W, h->PV, h->ptr, h->jidx, h->fix_pts, with_C ? h->cov_A.get() : nullptr, h->n32,
                                     mu, scale, h->cov_Y, h->cov_pts, h->cov_status);
  } else {
    const unsigned char *hq = h->has_held ? (const unsigned char *)h->held_pts : nullptr;
    const int marq = h->damp_kind == PSBA_DAMPING_MARQUARDT ? 1 : 0;
    if (h->cnp == KD_CNP)
      k_fcov_points<FreeKD><<<d.nP, 64, 0, s>>>(h->PV, h->free_Y, h->ptr, h->jidx, hq, h->cov_A, h->n32, mu, marq,
                                                h->damp_dmin, h->damp_dmax, scale, h->cov_pts, h->cov_status);
    else
      k_fcov_points<FreeK><<<d.nP, 64, 0, s>>>(h->PV, h->free_Y, h->ptr, h->jidx, hq, h->cov_A, h->n32, mu, marq,
                                               h->damp_dmin, h->damp_dmax, scale, h->cov_pts, h->cov_status);
  }
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

// the blocks C_jk of n_pairs camera pairs (device list) into out_dev [n_pairs][cnp^2]
int launch_cov_gather(psba_ctx *h, const int2 *pairs_dev, int n_pairs, double *out_dev) {
  k_cov_gather<<<n_pairs, 256, 0, h->stream>>>(h->cov_A, h->n32, pairs_dev, n_pairs, h->cnp, out_dev);
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

// sigma_dev [nT]: the square roots of the diagonals of C_aa and of the point blocks
int launch_fcov_sigmas(psba_ctx *h, double *sigma_dev) {
  k_fcov_sigmas<<<(unsigned)((h->d.nT + 255) / 256), 256, 0, h->stream>>>(h->cov_A, h->n32, h->cov_pts, h->d.nA, h->d.nT, sigma_dev);
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

}  // namespace psba
