// kernels_cov.hip -- covariance of the refined cameras and points on the fixed-K dense route.
//
// Definition (the same text in include/psba_hip.h and DESIGN 7h).  The covariance is taken at the current parameters
// and uses the linearization of psba_linearize(h, 1, 1): whitened, loss-weighted and masked by psba_set_fixed, i.e.
// exactly what the normal equations see.  N = J^T J on the free blocks.  For mu >= 0 and scale > 0,
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
// Route.  The kernels work on a private n32 x n32 copy of S (the identity padding rows of the reduce buffer make every
// 16 x 16 tile full) and never touch the Cholesky chain or its factor.  All bulk arithmetic is v_mfma_f64_16x16x4_f64
// (operand layout: top of kernels_free.hip -- A operand A[l & 15][l >> 4], B operand B[l >> 4][l & 15], C/D
// col = l & 15, row = (l >> 4) + 4 reg); a 16 x 16 x 16 tile product is four of them.
//   1 compaction  rows and columns of fixed cameras (and of the padding) get the identity; zeroed in the result
//   2 factor      right-looking blocked Cholesky on 16 x 16 tiles, three kernels per panel: one wave factors the
//                 diagonal tile and stores the inverse of its factor (status on a pivot that is not positive and finite);
//                 one wave per tile below forms X = C L_dd^-T; one wave per trailing tile C -= X_r X_c^T
//   3 inverse     one workgroup per 16-column strip of the identity: L X = E forward (block rows at or below the
//                 strip's own block only), L^T C = X backward; a block row is an MFMA accumulation over the earlier
//                 block rows -- four waves take the rows kb = first + w, first + w + 4, ... in ascending order and
//                 their four partial tiles are added in wave order -- then one product with the stored diagonal
//                 inverse.  The lower triangle of C is the result; a last kernel mirrors it and applies scale
//   4 points      one wave per point: V*_i and Y_ij from the stored linearization, then the 3 x 3 sum j-major with k
//                 ascending (only the six entries a <= b are summed, the others are their copies)
// No floating-point atomics: every sum has an order fixed by the problem's size, two computes are bit-identical.
#include "camera_model.h"
#include "psba_internal.h"

namespace psba {

typedef double cv4 __attribute__((ext_vector_type(4)));
constexpr int COV_JC = 32;  // cameras of a point whose C_jk Y_k rows are staged in LDS at a time

#define COV_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ bool cov_held(const unsigned char *fix, int r, int nA) { return r >= nA || (fix && fix[r / 6]); }

// ---- 1 compaction: M = S with the identity on the rows and columns of fixed cameras and of the padding ----
__global__ __launch_bounds__(256) void k_cov_compact(const double *S, double *M, const unsigned char *fix, int nA, int n32) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n32 * n32) return;
  const int r = (int)(t / n32), c = (int)(t % n32);
  M[t] = (cov_held(fix, r, nA) || cov_held(fix, c, nA)) ? (r == c ? 1.0 : 0.0) : S[t];
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

// ---- the lower triangle of X is the result: scale it, zero the held rows and columns, mirror it ----
__global__ __launch_bounds__(256) void k_cov_finish(double *X, const unsigned char *fix, int nA, int n32, double scale) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n32 * n32) return;
  const int r = (int)(t / n32), c = (int)(t % n32);
  if (c > r) return;
  const double v = (cov_held(fix, r, nA) || cov_held(fix, c, nA)) ? 0.0 : scale * X[t];
  X[t] = v;
  X[(size_t)c * n32 + r] = v;
}

__global__ __launch_bounds__(64) void k_cov_gather(const double *X, int ld, const int2 *pairs, int n_pairs, double *out) {
  const int q = blockIdx.x, t = threadIdx.x;
  if (q >= n_pairs || t >= 36) return;
  const int2 jk = pairs[q];
  out[36 * (size_t)q + t] = X[(size_t)(6 * jk.x + t / 6) * ld + 6 * jk.y + t % 6];
}

// ---- 4 one wave per point: C_bb,i = scale V*^-1 + sum_j sum_k Y_j^T C_jk Y_k (C = null: structure only) ----
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

// ---- host side ----
#define COV_TRY(expr)            \
  do {                           \
    int rc__ = (expr);           \
    if (rc__ < 0) return rc__;   \
  } while (0)
#define COV_LAUNCHED(h)                                                                                        \
  do {                                                                                                         \
    hipError_t e__ = hipGetLastError();                                                                        \
    if (e__ != hipSuccess) return fail((h), PSBA_E_HIP, "covariance kernel launch failed: %s", hipGetErrorString(e__)); \
  } while (0)

// The camera part in stages, so that the factorization and the inverse run unchanged between a compaction and a finish
// chosen by the caller (this file's for the fixed-K route, kernels_freecov.hip's for the free-intrinsics route).
// the two squares and the inverses of the factor's diagonal tiles, on first use
int cov_workspaces(psba_ctx *h) {
  const size_t nn = (size_t)h->n32 * h->n32;
  if (!h->cov_L) COV_TRY(h->cov_L.alloc(h, nn));
  if (!h->cov_C) COV_TRY(h->cov_C.alloc(h, nn));
  if (!h->cov_dinv) COV_TRY(h->cov_dinv.alloc(h, (size_t)256 * (h->n32 / 16)));
  return PSBA_OK;
}

// cov_L (a compacted copy of S) -> its Cholesky factor in place, cov_dinv, cov_status[0] on a bad pivot
int launch_cov_factor(psba_ctx *h) {
  const int n32 = h->n32, NT = n32 / 16;
  hipStream_t s = h->stream;
  for (int p = 0; p < NT; p++) {
    k_cov_diag<<<1, 64, 0, s>>>(h->cov_L, h->cov_dinv, n32, p, h->cov_status);
    const int rest = NT - p - 1;
    if (rest > 0) {
      k_cov_trsm<<<rest, 64, 0, s>>>(h->cov_L, h->cov_dinv, n32, p);
      k_cov_update<<<rest * (rest + 1) / 2, 64, 0, s>>>(h->cov_L, n32, p);
    }
  }
  COV_LAUNCHED(h);
  return PSBA_OK;
}

// the factor in cov_L -> the lower triangle of its inverse in cov_C
int launch_cov_inverse(psba_ctx *h) {
  const int n32 = h->n32, NT = n32 / 16;
  k_cov_inverse<<<NT, 256, 0, h->stream>>>(h->cov_L, h->cov_dinv, h->cov_C, n32, NT);
  COV_LAUNCHED(h);
  return PSBA_OK;
}

// S (the n32 x n32 head of the reduce buffer) -> cov_C = scale S^-1 with zeros on the held rows and columns.
// ev (may be null): three events recorded before the factor, between factor and inverse, and behind the inverse
int launch_cov_cameras(psba_ctx *h, double scale, hipEvent_t *ev) {
  const int n32 = h->n32, nA = h->d.nA;
  const size_t nn = (size_t)n32 * n32;
  COV_TRY(cov_workspaces(h));
  const unsigned nb = (unsigned)((nn + 255) / 256);
  hipStream_t s = h->stream;
  if (ev) PSBA_HIP(h, hipEventRecord(ev[0], s));
  k_cov_compact<<<nb, 256, 0, s>>>(h->red, h->cov_L, h->fix_cams, nA, n32);
  COV_TRY(launch_cov_factor(h));
  if (ev) PSBA_HIP(h, hipEventRecord(ev[1], s));
  COV_TRY(launch_cov_inverse(h));
  k_cov_finish<<<nb, 256, 0, s>>>(h->cov_C, h->fix_cams, nA, n32, scale);
  COV_LAUNCHED(h);
  if (ev) PSBA_HIP(h, hipEventRecord(ev[2], s));
  return PSBA_OK;
}

// the point blocks from the stored linearization and cov_C (with_C = false: every camera fixed, scale V*^-1 alone)
int launch_cov_points(psba_ctx *h, double mu, double scale, bool with_C) {
  const Dims &d = h->d;
  if (!h->cov_pts) COV_TRY(h->cov_pts.alloc(h, (size_t)9 * d.nP));
  if (with_C && !h->cov_Y) COV_TRY(h->cov_Y.alloc(h, (size_t)18 * d.nO));
  k_cov_points<<<d.nP, 64, 0, h->stream>>>(h->W, h->PV, h->ptr, h->jidx, h->fix_pts, with_C ? h->cov_C.get() : nullptr,
                                           h->n32, mu, scale, h->cov_Y, h->cov_pts, h->cov_status);
  COV_LAUNCHED(h);
  return PSBA_OK;
}

// the blocks C_jk of n_pairs camera pairs (device list) into out_dev [n_pairs][36]
int launch_cov_gather(psba_ctx *h, const int2 *pairs_dev, int n_pairs, double *out_dev) {
  k_cov_gather<<<n_pairs, 64, 0, h->stream>>>(h->cov_C, h->n32, pairs_dev, n_pairs, out_dev);
  COV_LAUNCHED(h);
  return PSBA_OK;
}

}  // namespace psba
