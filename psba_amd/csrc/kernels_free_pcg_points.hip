// kernels_free_pcg_points.hip -- covariance of chosen 3-D points on the block-sparse route of the free-intrinsics camera
// blocks of 11 and 16 (psba_sparse_point_covariance).  What kernels_free_pcg_many.hip does for the unit
// columns of chosen cameras, for the right-hand sides Y of chosen points: three columns per point, five points per
// panel of 16 columns (column 15 is always idle), the iteration of 7o unchanged, and a contraction back to 3 x 3 blocks
// on v_mfma_f64_16x16x4_f64.
//
// DEFINITION (the text of include/psba_hip.h).
//   * The linearization is psba_linearize(h, 1, 1) at the current parameters, as for psba_sparse_camera_covariance: the
//     mask, the per-camera masks, held poses and points, priors, observation weighting and the damping rule are in S, V
//     and Y.
//   * For a chosen point i and c < 3 the right-hand side b_{i,c} holds, in its rows of camera j in cams(i), column c of
//     Y_ij (cnp x 3, as k_free_Y stored it for this mu); every other row is +0.0.  The column x_{i,c} solves
//     S(mu) x = b_{i,c} by the route's conjugate gradients: block-Jacobi preconditioning, psba_set_solver's tol and
//     max_iter, the stop rule of psba_schur_solve on this route with r.r judged against this column's own b.b.
//   * Block (a, b) of the chosen list is scale [ delta_ab V*_a^-1 + sum_{j in cams(a)} Y_aj^T x_b[rows of j] ], the sum
//     in ascending j.  V*_i = V_i + mu D_i is rebuilt with the route's own damping (D = I, or Marquardt's diagonal of
//     psba_set_damping) and inverted by the closed form; |det| < 1e-16 gives PSBA_SINGULAR_V.
//   * Block (a, b) with position a >= b is taken from the columns solved for sel_pts[b] and written to both sides;
//     inside a diagonal block the lower triangle is the matrix.  So C is bit-symmetric.
//   * A held point: nothing is solved; its rows and columns of C and its rows of cols are exactly +0.0, its iters 0 and
//     its relres 0.  A point without observations, and one whose blocks Y are all zero: b = 0, the columns start stopped
//     with x = 0 (iters 0, relres 0) and the diagonal block is scale V*^-1.
//   * Masked and held-pose coordinates need no case of their own: their rows of W, and hence of Y, are +0.0 by
//     construction, so b, every iterate and cols are zero there (cols: +0.0).
//   * C = scale (...); cols is not scaled.
//   * mu = 0 needs a gauge, held poses or priors; mu > 0 gives a regularised inverse and NOT a covariance.
// COLUMNS ARE INDEPENDENT.  A column's bits, iteration count and relres depend on none of: which other points are
// chosen, their order, the column's position in its panel, the batch.  Each column has its own alpha, beta and stop
// (k_fpcgm_update / k_fpcgm_direction), every inner product is summed from per-workgroup partials in a fixed order, a
// workgroup's partial of a column is the sum of its 16 strands, which hold the same coordinates whatever the column's
// position, the grids depend on nA and nC only, and there are no floating-point atomics.
// THE START'S SUMS.  Unlike the unit start, b.b and the first r.z are sums.  k_fpcgp_start leaves per-workgroup partials
// [workgroup][16] in the panel's scalar block, in partial slots the iteration has not used yet (r.r of slot 3, r.z of
// slot 0; the scalar block is NOT widened), and a second launch of one workgroup per panel, k_fpcgp_scalars, adds them
// with fpcgm_sum_partials into MF_BB and MF_RZ of slot 0 and writes the rest of the scalars.  k_fpcgm_spmm / _update /
// _direction then run unchanged.
// WHO WRITES C.  k_fcovp_contract: the wave of (chosen position a, panel) writes, for every position b <= a whose
// columns the panel holds, the entries of block (a, b) and their mirrors in block (b, a); of a diagonal block the lane
// of (i, c), i >= c, writes (i, c) and (c, i).  Every entry of C has exactly one writer over the batches.
#include <cmath>
#include <vector>

#include "api_common.h"
#include "camera_model.h"
#include "free_blocks.h"
#include "free_pcg_many.h"

namespace psba {

constexpr int FPP_PTS = 5;   // points of a panel: columns 3 a + c, a < 5, c < 3; column 15 idle

// start of a batch: panel y solves for the points at positions 5 y .. 5 y + 4 of pts [n_pts] (positions >= n_pts: idle
// columns).  A thread owns (coordinate, column): it looks its camera up in the point's slice of jidx (cameras ascend
// inside a point), reads the camera's whole b from Y -- column c of Y_ij, [cnp][3] -- and forms z = M^-1 b of its row
// itself, as k_fpcgm_update forms a camera's residual.  x = 0, r = b, z = M^-1 b, p = z, q = 0; the partials of b.b and
// of r.z per column and workgroup.  A held point's columns get b = 0 here and are marked dead by k_fpcgp_scalars
template <class T>
__global__ __launch_bounds__(256) void k_fpcgp_start(const int *pts, int n_pts, const int *ptr, const int *jidx,
                                                     const double *Y, const unsigned char *held_pt, const double *minv,
                                                     double *x_all, double *r_all, double *z_all, double *p_all, double *q_all,
                                                     int n, double *pc_all, size_t vstride) {
  constexpr int CNP = T::CNP, C2 = CNP * CNP, WB = 3 * CNP;
  __shared__ double sW[256], sA[16], sB[16];
  double *pc = pc_all + (size_t)MF_ALL * blockIdx.y;
  const size_t off = vstride * blockIdx.y;
  const int col = threadIdx.x & 15, a = col / 3, c = col % 3, pos = FPP_PTS * blockIdx.y + a;
  const bool used = col < 3 * FPP_PTS && pos < n_pts;
  const int i = used ? pts[pos] : 0;
  const bool on = used && !(held_pt && held_pt[i]);
  const int o0 = on ? ptr[i] : 0, o1 = on ? ptr[i + 1] : 0;
  double bb = 0.0, rz = 0.0;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < (size_t)16 * n; t += (size_t)gridDim.x * 256) {
    const int coord = (int)(t >> 4), j = coord / CNP, row = coord % CNP;
    int lo = o0, hi = o1;  // the first observation of the point whose camera is >= j
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (jidx[mid] < j) lo = mid + 1; else hi = mid;
    }
    double own = 0.0, zz = 0.0;
    if (lo < o1 && jidx[lo] == j) {
      const double *y = Y + (size_t)WB * lo + c, *m = minv + (size_t)C2 * j + CNP * row;
#pragma unroll
      for (int k = 0; k < CNP; k++) {
        const double bk = y[3 * k];
        zz += m[k] * bk;
        own = k == row ? bk : own;
      }
    }
    x_all[off + t] = 0.0;
    r_all[off + t] = own;
    z_all[off + t] = zz;
    p_all[off + t] = zz;
    q_all[off + t] = 0.0;
    bb += own * own;
    rz += own * zz;
  }
  fpcgm_block_sums(bb, sW, sA);
  fpcgm_block_sums(rz, sW, sB);
  if (threadIdx.x < 16) {
    pc[MF_RRP + 16 * FPCG_CAP * 3 + 16 * blockIdx.x + col] = sA[col];
    pc[MF_RZP + 16 * blockIdx.x + col] = sB[col];
  }
}

// one workgroup per panel, after k_fpcgp_start: the panel's scalars written whole.  b.b and r.z of slot 0 are the sums
// of the start's npart partials; a column of an idle position, of a held point or with b.b == 0 starts stopped
__global__ __launch_bounds__(256) void k_fpcgp_scalars(const int *pts, int n_pts, const unsigned char *held_pt, int npart,
                                                       double *pc_all) {
  __shared__ double sW[256], sA[16], sB[16];
  double *pc = pc_all + (size_t)MF_ALL * blockIdx.x;
  fpcgm_sum_partials(pc + MF_RRP + 16 * FPCG_CAP * 3, npart, sW, sA);
  fpcgm_sum_partials(pc + MF_RZP, npart, sW, sB);
  if (threadIdx.x < MF_N) pc[threadIdx.x] = 0.0;
  __syncthreads();
  if (threadIdx.x < 16) {
    const int col = threadIdx.x, pos = FPP_PTS * blockIdx.x + col / 3;
    const bool used = col < 3 * FPP_PTS && pos < n_pts;
    const bool live = used && !(held_pt && held_pt[pts[used ? pos : 0]]) && sA[col] != 0.0;
    pc[MF_BB + col] = live ? sA[col] : 0.0;
    pc[MF_RZ + col] = live ? sB[col] : 0.0;
    pc[MF_DEAD + col] = live ? 0.0 : 1.0;
    pc[MF_ACT + col] = live ? 1.0 : 0.0;
    pc[MF_DONE + col] = live ? 0.0 : 1.0;
  }
}

// one wave per (chosen position a, panel y of the batch): T = sum_j Y_aj^T X[rows j][16 columns], one accumulator chain
// in ascending j, K ascending inside a block (four steps for blocks of 16, three for blocks of 11 with rows >= 11
// supplying 0.0).  A operand: lane l supplies Y_aj^T[l & 15][4 t + (l >> 4)] = Y_aj[4 t + (l >> 4)][l & 15], rows 3 .. 15
// supply 0.0; B operand: X[cnp j + 4 t + (l >> 4)][l & 15].  T[i][n] is register 0 of lane (l >> 4 = i, l & 15 = n).
// Column n = 3 m + c belongs to position b = p0 + 5 y + m.  The wave writes block (a, b) and its mirror for b <= a (the
// mirror rule; of the diagonal block the lower triangle), adds V*^-1 on the diagonal block, multiplies by scale.  A held
// point on either side gives +0.0.  status[0]: some |det V*| < 1e-16
template <class T>
__global__ __launch_bounds__(64) void k_fcovp_contract(const double *x_all, size_t vstride, const int *sel, int n_sel, int p0,
                                                       const int *ptr, const int *jidx, const double *Y, const double *PV,
                                                       const unsigned char *held_pt, double mu, int marquardt, double dmin,
                                                       double dmax, double scale, double *C, int *status) {
  constexpr int CNP = T::CNP, WB = 3 * CNP, KS = CNP == 16 ? 4 : 3;
  const int a = blockIdx.x, pb = p0 + FPP_PTS * blockIdx.y;  // the panel's first position
  if (a < pb) return;                                           // (uniform) nothing of block row a comes from this panel
  const int lane = threadIdx.x, kq = lane >> 4, nn = lane & 15;
  const int ia = sel[a];
  const bool held_a = held_pt && held_pt[ia];
  const double *x = x_all + vstride * blockIdx.y;
  kd4 acc = {0.0, 0.0, 0.0, 0.0};
  if (!held_a) {
    const bool arow = nn < 3;
    const int o1 = ptr[ia + 1];
    for (int o = ptr[ia]; o < o1; o++) {
      const double *y = Y + (size_t)WB * o + (arow ? nn : 0), *xj = x + (size_t)16 * CNP * jidx[o] + nn;
      double av[KS], bv[KS];
#pragma unroll
      for (int t = 0; t < KS; t++) {
        const int k = 4 * t + kq;
        const bool kin = CNP == 16 || k < CNP;
        const int kk = kin ? k : 0;
        av[t] = y[3 * kk];
        bv[t] = xj[16 * kk];
        if (!kin || !arow) av[t] = 0.0;
        if (!kin) bv[t] = 0.0;
      }
#pragma unroll
      for (int t = 0; t < KS; t++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t], bv[t], acc, 0, 0, 0);
    }
  }
  const int m = nn / 3, c = nn % 3, b = pb + m, i = kq;
  if (nn >= 3 * FPP_PTS || b >= n_sel || b > a || i >= 3) return;
  double v = 0.0;
  if (a == b) {
    if (i < c) return;  // the lower triangle is the matrix
    if (!held_a) {
      const double *pv = PV + 9 * (size_t)ia;
      double w[6], wi[6];
#pragma unroll
      for (int q = 0; q < 6; q++) w[q] = pv[q];
      if (marquardt) {
        damp_point_block(w, mu, dmin, dmax);
      } else {
        w[0] += mu;
        w[3] += mu;
        w[5] += mu;
      }
      if (sym3_inverse(w, wi) && i == 0 && c == 0) status[0] = 1;
      // sym6 packing (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); here c <= i
      const double vi = c == 0 ? (i == 0 ? wi[0] : i == 1 ? wi[1] : wi[2]) : c == 1 ? (i == 1 ? wi[3] : wi[4]) : wi[5];
      v = scale * (vi + acc[0]);
    }
  } else if (!held_a && !(held_pt && held_pt[sel[b]])) {
    v = scale * acc[0];
  }
  const size_t N = (size_t)3 * n_sel;
  C[((size_t)3 * a + i) * N + (size_t)3 * b + c] = v;
  C[((size_t)3 * b + c) * N + (size_t)3 * a + i] = v;
}

// the solved columns of a batch into cols [3 n_pts][nA], not scaled: row 15 y + n = column n < 15 of panel y.
// x + 0.0: a zero of either sign is returned as +0.0
__global__ __launch_bounds__(256) void k_fcovp_cols(const double *x_all, size_t vstride, int n_pts, int nA, double *cols) {
  const size_t all = (size_t)3 * n_pts * nA;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < all; t += (size_t)gridDim.x * 256) {
    const int rowc = (int)(t / nA), coord = (int)(t % nA), y = rowc / 15, n = rowc % 15;
    cols[t] = x_all[vstride * y + (size_t)16 * coord + n] + 0.0;
  }
}

// ---- host side ----

// the columns of the chosen points in batches of at most FCOVM_PANELS panels (40 points), bursts of 8 iterations
// between host synchronisations; per column the host reads what fcm_compute reads.  Returns PSBA_OK, PSBA_NOT_SPD,
// PSBA_SINGULAR_V or PSBA_PCG_MAXIT (or an error)
template <class T>
static int fcp_compute(psba_ctx *h, double mu, double scale, int n_sel, const int *sel, double *C, double *cols, int *iters,
                       double *relres) {
  const int n = h->d.nA, g = fcm_vec_grid(n);
  const size_t vs = (size_t)16 * n, N = (size_t)3 * n_sel;
  hipStream_t s = h->stream;
  const int panels = (n_sel + FPP_PTS - 1) / FPP_PTS, cap = panels < FCOVM_PANELS ? panels : FCOVM_PANELS;
  TRY(fcm_buffers(h, cap));
  DevBuf<int> sel_dev, st_dev;
  DevBuf<double> C_dev, cols_dev;
  TRY(sel_dev.alloc(h, (size_t)n_sel));
  TRY(st_dev.alloc(h, 1));
  TRY(C_dev.alloc(h, N * N));
  if (cols) TRY(cols_dev.alloc(h, (size_t)cap * 3 * FPP_PTS * n));
  PSBA_HIP(h, hipMemcpyAsync(sel_dev, sel, sizeof(int) * n_sel, hipMemcpyHostToDevice, s));
  PSBA_HIP(h, hipMemsetAsync(st_dev, 0, sizeof(int), s));
  const size_t vc = vs * h->fcm_cap;
  double *x = h->fcm_vec, *r0 = x + vc, *z = r0 + vc, *p = z + vc, *q = p + vc;
  double *pc = h->fcm_scal, *ipc = pc + (size_t)MF_ALL * FCOVM_PANELS, *hs = h->fcm_host, *ihs = hs + (size_t)MF_N * FCOVM_PANELS;
  const int zero4[4] = {0, 0, 0, 0}, stamp = 1;
  const unsigned char *held = h->has_held ? (const unsigned char *)h->held_pts : nullptr;
  const int marq = h->damp_kind == PSBA_DAMPING_MARQUARDT ? 1 : 0;
  const double tol2 = h->pcg_tol * h->pcg_tol;
  ProfScope ps(h, PSBA_K_CHOLESKY);
  PSBA_HIP(h, hipMemsetAsync(ipc, 0, sizeof(double) * 16, s));
  PSBA_HIP(h, hipMemcpyAsync(h->fcm_status, zero4, sizeof zero4, hipMemcpyHostToDevice, s));
  TRY(launch_fbsr_diag_inverse(h, h->pcg_minv, ipc, h->fcm_status, stamp));
  bool not_spd = false, exhausted = false;
  for (int p0 = 0; p0 < n_sel; p0 += FPP_PTS * FCOVM_PANELS) {
    const int npt = n_sel - p0 < FPP_PTS * FCOVM_PANELS ? n_sel - p0 : FPP_PTS * FCOVM_PANELS;
    const int np = (npt + FPP_PTS - 1) / FPP_PTS;
    hipLaunchKernelGGL(k_fpcgp_start<T>, dim3(g, np), dim3(256), 0, s, sel_dev.get() + p0, npt, h->ptr.get(), h->jidx.get(),
                       h->free_Y.get(), held, h->pcg_minv.get(), x, r0, z, p, q, n, pc, vs);
    hipLaunchKernelGGL(k_fpcgp_scalars, dim3(np), dim3(256), 0, s, sel_dev.get() + p0, npt, held, g, pc);
    PSBA_HIP(h, hipGetLastError());
    std::vector<char> open((size_t)16 * np, 1);
    std::vector<int> its((size_t)16 * np, 0);
    std::vector<double> rel((size_t)16 * np, 0.0);
    bool any_open = true;
    for (int it = 0; any_open;) {
      const int burst = it + 8 < h->pcg_maxit ? 8 : h->pcg_maxit - it;
      if (burst > 0) TRY(launch_fpcgm_burst(h, np, it, burst));
      const int last = burst > 0 ? it + burst - 1 : it;
      if (burst > 0) it += burst;
      PSBA_HIP(h, hipMemcpy2DAsync(hs, sizeof(double) * MF_N, pc, sizeof(double) * MF_ALL, sizeof(double) * MF_N, np,
                                   hipMemcpyDeviceToHost, s));
      PSBA_HIP(h, hipMemcpyAsync(ihs, ipc, sizeof(double) * 16, hipMemcpyDeviceToHost, s));
      PSBA_HIP(h, hipStreamSynchronize(s));
      if (ihs[1] != 0.0) not_spd = true;  // a bad pivot of a diagonal block (k_fbsr_diag_inverse's fail slot)
      any_open = false;
      for (int y = 0; y < np; y++) {
        const double *c = hs + (size_t)MF_N * y;
        for (int col = 0; col < 3 * FPP_PTS; col++) {
          const int at = 16 * y + col;
          if (!open[at]) continue;
          open[at] = 0;
          if (c[MF_DEAD + col] != 0.0) continue;  // nothing was solved: 0 iterations, relres 0
          its[at] = it;
          if (c[MF_FAIL + col] != 0.0) {
            not_spd = true;
            rel[at] = NAN;
            continue;
          }
          const double bb = c[MF_BB + col];
          double rr = c[MF_RR + 16 * (last & 3) + col];
          bool converged = false;
          if (c[MF_DONE + col] != 0.0) {  // the test held inside the burst: the column stopped there
            its[at] = (int)c[MF_DONE + col] - 1;
            rr = c[MF_RRFIN + col];
            converged = true;
          } else if (rr <= tol2 * bb) {  // ... or in its last iteration
            converged = true;
          }
          rel[at] = bb > 0.0 ? sqrt(rr / bb) : 0.0;
          if (converged) continue;
          if (!(rr - rr == 0.0)) {  // a non-finite residual: reported like a failed factorization
            not_spd = true;
            continue;
          }
          if (it >= h->pcg_maxit) {
            exhausted = true;
            continue;
          }
          open[at] = 1;
          any_open = true;
        }
      }
      if (burst <= 0) break;
    }
    hipLaunchKernelGGL(k_fcovp_contract<T>, dim3(n_sel, np), dim3(64), 0, s, x, vs, sel_dev.get(), n_sel, p0, h->ptr.get(),
                       h->jidx.get(), h->free_Y.get(), h->PV.get(), held, mu, marq, h->damp_dmin, h->damp_dmax, scale,
                       C_dev.get(), st_dev.get());
    if (cols) {
      const size_t work = (size_t)3 * npt * n;
      const int gg = (int)((work + 255) / 256 < 1024 ? (work + 255) / 256 : 1024);
      hipLaunchKernelGGL(k_fcovp_cols, dim3(gg), dim3(256), 0, s, x, vs, npt, n, cols_dev.get());
      PSBA_HIP(h, hipMemcpyAsync(cols + (size_t)3 * p0 * n, cols_dev, sizeof(double) * (size_t)3 * npt * n, hipMemcpyDeviceToHost, s));
    }
    PSBA_HIP(h, hipGetLastError());
    PSBA_HIP(h, hipStreamSynchronize(s));
    for (int k = 0; k < 3 * npt; k++) {
      const int at = 16 * (k / (3 * FPP_PTS)) + k % (3 * FPP_PTS);
      if (iters) iters[(size_t)3 * p0 + k] = its[at];
      if (relres) relres[(size_t)3 * p0 + k] = rel[at];
    }
  }
  int st = 0;
  PSBA_HIP(h, hipMemcpyAsync(C, C_dev, sizeof(double) * N * N, hipMemcpyDeviceToHost, s));
  PSBA_HIP(h, hipMemcpyAsync(&st, st_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  PSBA_HIP(h, hipStreamSynchronize(s));
  return not_spd ? PSBA_NOT_SPD : st ? PSBA_SINGULAR_V : exhausted ? PSBA_PCG_MAXIT : PSBA_OK;
}

int launch_fcovp_compute(psba_ctx *h, double mu, double scale, int n_sel, const int *sel, double *C, double *cols, int *iters,
                         double *relres) {
  return h->cnp == KD_CNP ? fcp_compute<FreeKD>(h, mu, scale, n_sel, sel, C, cols, iters, relres)
                          : fcp_compute<FreeK>(h, mu, scale, n_sel, sel, C, cols, iters, relres);
}

}  // namespace psba
