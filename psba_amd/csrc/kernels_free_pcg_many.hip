// kernels_free_pcg_many.hip -- chosen columns of S(mu)^-1 on the block-sparse route of the free-intrinsics camera blocks
// of 11 and 16 (psba_sparse_camera_covariance, psba_sparse_S_times_many).  What kernels_free_pcg.hip does
// for one right-hand side, for panels of 16: a chosen camera contributes cnp right-hand sides e_q, which form one panel
// [nA][16] (a block of 11 leaves the panel's columns 11 .. 15 idle), and the product Q_j = sum_k B_jk P_k of a block row
// is a chain of 16 x 16 matrix products on v_mfma_f64_16x16x4_f64.
//
// DEFINITION (the text of include/psba_hip.h).
//   * The linearization is psba_linearize(h, 1, 1) at the current parameters, as for psba_free_covariance_compute: the
//     mask, the per-camera masks, held poses and points, priors, observation weighting and the damping rule are in S.
//   * A coordinate is live if it is neither masked nor a held pose coordinate (the predicates of k_cov_map_free; groups
//     cannot be set on this route).
//   * For a live chosen coordinate q the column x_q solves S(mu) x_q = e_q by the route's conjugate gradients: block-
//     Jacobi preconditioning, psba_set_solver's tol and max_iter, the stop rule of k_fpcg_update.
//   * For a masked or held chosen coordinate nothing is solved: its row and column of C and its row of cols are exactly
//     +0.0, not the inverse of the placeholder.
//   * C is taken from the solved columns: block (a, b) of the chosen list with position a >= b from the columns solved
//     for camera sel[b], rows of camera sel[a], written to both sides; inside a diagonal block the lower triangle is the
//     matrix.  So C is bit-symmetric.
//   * C = scale (...); cols is not scaled.
//   * mu = 0 needs a gauge, held poses or priors; mu > 0 gives a regularised inverse and NOT a covariance.
// COLUMNS ARE INDEPENDENT.  A column's bits, iteration count and relres depend neither on which other cameras are
// chosen nor on the batch it lands in: each column has its own alpha, beta and stop, a stopped column is frozen while
// the others go on, every inner product is summed from per-workgroup partials in a fixed order, the grids depend on nA
// and nC only, and there are no floating-point atomics (the rule of the route, kernels_free.hip).
#include <cmath>

#include "api_common.h"
#include "free_blocks.h"
#include "free_pcg_many.h"

namespace psba {

constexpr int FSPMM_TRIP = 4;  // entries of a row whose loads are in flight together (k_fpcgm_spmm)

template <class T>
__device__ __forceinline__ bool fcm_live(unsigned mask, const unsigned short *cmask, const unsigned char *held, int j, int k) {
  return k < T::NI ? ((kd_free_bits(mask, cmask, j) >> k) & 1u) != 0 : !(held && held[j]);
}

__device__ __forceinline__ bool fpcgm_converged_before(const double *pc, int col, int it, double rz, double bb, double tol2) {
  if (rz == 0.0) return true;
  return it > 0 && pc[MF_RR + 16 * ((it - 1) & 3) + col] <= tol2 * bb;
}

// Q = S P for panels of 16 columns and the partial sums of p.q per column: one wave per (block row, panel), a persistent
// grid of fpcg_row_grid(nC) workgroups of four waves in x (rows in grid stride), the panels in y.  The row walk is
// bs_rowptr / bs_rowent as k_fpcg_spmv reads it.  Per entry the wave issues KS = 4 (blocks of 16) or 3 (blocks of 11)
// v_mfma_f64_16x16x4_f64: in step t lane l (i = l & 15, k = l >> 4, c = 4 t + k) supplies element (i, c) of the block as
// the A operand and P_other[c][l & 15] as the B operand; rows and columns >= 11 of a block of 11 supply 0.0.  how = 0
// reads the block as stored (B[i][c]), how = 1 transposed (B[c][i]), how = 2 the diagonal block through its lower
// triangle by address (B[max(i, c)][min(i, c)]): the strict upper triangle is never loaded.  One accumulator chain per
// row in the order of the walk, K ascending inside a block; FSPMM_TRIP entries' loads are in flight together and the
// order of the adds does not depend on that.  The accumulator holds Q[k + 4 r][l & 15] in register r.
// use_act: a panel all of whose columns have stopped is left alone (its partials are read by nobody)
template <class T>
__global__ __launch_bounds__(256) void k_fpcgm_spmm(const double *val, const int *rowptr, const int2 *rowent, int nC,
                                                    const double *p_all, double *q_all, double *pc_all, int slot,
                                                    size_t vstride, int use_act) {
  constexpr int CNP = T::CNP, C2 = CNP * CNP, KS = CNP == 16 ? 4 : 3;
  __shared__ double sW[4][16];
  double *pc = pc_all + (size_t)MF_ALL * blockIdx.y;
  if (use_act) {
    bool any = false;
#pragma unroll
    for (int c = 0; c < 16; c++) any = any || pc[MF_ACT + c] != 0.0;
    if (!any) return;
  }
  const double *p = p_all + vstride * blockIdx.y;
  double *q = q_all + vstride * blockIdx.y;
  const int lane = threadIdx.x & 63, k = lane >> 4, i = lane & 15;
  const bool irow = CNP == 16 || i < CNP;
  double pq = 0.0;
  for (int j = blockIdx.x * 4 + (threadIdx.x >> 6); j < nC; j += gridDim.x * 4) {
    kd4 acc = {0.0, 0.0, 0.0, 0.0};
    const int e1 = rowptr[j + 1];
    for (int e0 = rowptr[j]; e0 < e1; e0 += FSPMM_TRIP) {
      double a[FSPMM_TRIP][KS], b[FSPMM_TRIP][KS];
#pragma unroll
      for (int u = 0; u < FSPMM_TRIP; u++) {
        const bool on = e0 + u < e1;
        const int2 en = on ? rowent[e0 + u] : make_int2(0, 0);
        const int how = en.y >> 28;
        const double *B = val + (size_t)C2 * en.x;
        const double *po = p + (size_t)(16 * CNP) * (en.y & 0x0fffffff);
#pragma unroll
        for (int t = 0; t < KS; t++) {
          const int c = 4 * t + k;
          const bool cin = on && (CNP == 16 || c < CNP);
          const int cc = cin ? c : 0, ii = irow ? i : 0;
          const int hi = ii > cc ? ii : cc, lo = ii > cc ? cc : ii;
          const int at = how == 0 ? CNP * ii + cc : how == 1 ? CNP * cc + ii : CNP * hi + lo;
          a[u][t] = cin && irow ? B[at] : 0.0;
          b[u][t] = cin ? po[16 * cc + i] : 0.0;
        }
      }
#pragma unroll
      for (int u = 0; u < FSPMM_TRIP; u++) {
        if (e0 + u < e1) {  // (uniform in the wave)
#pragma unroll
          for (int t = 0; t < KS; t++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][t], b[u][t], acc, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = k + 4 * r;
      if (CNP == 16 || row < CNP) {
        const size_t at = (size_t)16 * (CNP * (size_t)j + row) + i;
        q[at] = acc[r];
        pq += p[at] * acc[r];
      }
    }
  }
  pq += __shfl_xor(pq, 16, 64);
  pq += __shfl_xor(pq, 32, 64);
  if (lane < 16) sW[threadIdx.x >> 6][lane] = pq;
  __syncthreads();
  if (threadIdx.x < 16)
    pc[MF_PQP + 16 * FPCG_CAP * slot + 16 * blockIdx.x + threadIdx.x] =
        ((sW[0][threadIdx.x] + sW[1][threadIdx.x]) + sW[2][threadIdx.x]) + sW[3][threadIdx.x];
}

// start of a batch: panel y solves for camera sel[y]; column n of the panel is the unit vector of the camera's
// coordinate n, generated here.  x = 0, r = e_q, z = M^-1 r (column n of the camera's block inverse), p = z, q = 0; the
// panel's scalars are written whole (workgroup 0): b.b = 1 and r.z of slot 0 = the diagonal entry of the inverse.  A
// column of a masked or held coordinate, and columns >= 11 of a block of 11, start stopped with x = 0
template <class T>
__global__ __launch_bounds__(256) void k_fpcgm_start(const int *sel, unsigned mask, const unsigned short *cmask,
                                                     const unsigned char *held, const double *minv, double *x_all, double *r_all,
                                                     double *z_all, double *p_all, double *q_all, int n, double *pc_all,
                                                     size_t vstride) {
  constexpr int CNP = T::CNP, C2 = CNP * CNP;
  const int cam = sel[blockIdx.y], col = threadIdx.x & 15;
  const bool live = col < CNP && fcm_live<T>(mask, cmask, held, cam, col);
  double *pc = pc_all + (size_t)MF_ALL * blockIdx.y;
  const size_t off = vstride * blockIdx.y;
  if (blockIdx.x == 0) {
    if (threadIdx.x < MF_N) pc[threadIdx.x] = 0.0;
    __syncthreads();
    if (threadIdx.x < 16) {
      pc[MF_BB + col] = live ? 1.0 : 0.0;
      pc[MF_RZ + col] = live ? minv[(size_t)C2 * cam + CNP * col + col] : 0.0;
      pc[MF_DEAD + col] = live ? 0.0 : 1.0;
      pc[MF_ACT + col] = live ? 1.0 : 0.0;
      pc[MF_DONE + col] = live ? 0.0 : 1.0;
    }
  }
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < (size_t)16 * n; t += (size_t)gridDim.x * 256) {
    const int coord = (int)(t >> 4), j = coord / CNP, row = coord % CNP;
    const bool mine = live && j == cam;
    const double bt = mine && row == col ? 1.0 : 0.0;
    const double zz = mine ? minv[(size_t)C2 * cam + CNP * row + col] : 0.0;
    x_all[off + t] = 0.0;
    r_all[off + t] = bt;
    z_all[off + t] = zz;
    p_all[off + t] = zz;
    q_all[off + t] = 0.0;
  }
}

// k_fpcg_update per column: x += alpha p, r -= alpha q with the column's alpha = r.z / p.Sp; z = M^-1 r with the
// camera's block (a thread forms the new residual of all rows of its camera itself from the old r, kept in two buffers
// used in turn); the partials of r.r and of the next r.z per column.  A thread owns one column (the grid's stride is a
// multiple of 16).  The stop test is that of k_fpcg_update, before the iteration on the previous r.r, with r.z = 0
// counting as converged; a column that has stopped or failed is left as it is.  npq: the partials of p.Sp
template <class T>
__global__ __launch_bounds__(256) void k_fpcgm_update(double *x_all, const double *r_all, double *rn_all, const double *p_all,
                                                      const double *q_all, const double *minv, double *z_all, int n,
                                                      double *pc_all, int it, int npq, double tol2, size_t vstride) {
  constexpr int CNP = T::CNP;
  __shared__ double sW[256], sPQ[16], sA[16], sB[16];
  double *pc = pc_all + (size_t)MF_ALL * blockIdx.y;
  const size_t off = vstride * blockIdx.y;
  const int col = threadIdx.x & 15;
  fpcgm_sum_partials(pc + MF_PQP + 16 * FPCG_CAP * (it & 3), npq, sW, sPQ);
  const double pq = sPQ[col], rz = pc[MF_RZ + 16 * (it & 3) + col], bb = pc[MF_BB + col];
  const bool failed = pc[MF_FAIL + col] != 0.0;
  const bool conv = !failed && fpcgm_converged_before(pc, col, it, rz, bb, tol2);
  const bool active = !failed && !conv && pq > 0.0;
  if (blockIdx.x == 0 && threadIdx.x < 16) {
    if (conv && pc[MF_DONE + col] == 0.0) {
      pc[MF_RRFIN + col] = it > 0 ? pc[MF_RR + 16 * ((it - 1) & 3) + col] : 0.0;
      pc[MF_DONE + col] = (double)(it + 1);  // it iterations were carried out (+1: zero means "not yet")
    } else if (!failed && !conv && !(pq > 0.0)) {
      pc[MF_FAIL + col] = 1.0;  // not positive definite, or a break-down, or not a number
    }
  }
  const double alpha = active ? rz / pq : 0.0;
  double rr = 0.0, rzn = 0.0;
  if (active) {
    const double *r = r_all + off, *q = q_all + off;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < (size_t)16 * n; t += (size_t)gridDim.x * 256) {
      const int coord = (int)(t >> 4), j = coord / CNP, row = coord % CNP;
      const double *m = minv + (size_t)(CNP * CNP) * j + CNP * row;
      const size_t cb = (size_t)16 * CNP * j + col;
      double zz = 0.0, own = 0.0;
#pragma unroll
      for (int c = 0; c < CNP; c++) {
        const double rc = r[cb + 16 * c] - alpha * q[cb + 16 * c];
        zz += m[c] * rc;
        own = c == row ? rc : own;
      }
      x_all[off + t] += alpha * p_all[off + t];
      rn_all[off + t] = own;
      z_all[off + t] = zz;
      rr += own * own;
      rzn += own * zz;
    }
  }
  fpcgm_block_sums(rr, sW, sA);
  fpcgm_block_sums(rzn, sW, sB);
  if (threadIdx.x < 16 && active) {
    pc[MF_RRP + 16 * FPCG_CAP * (it & 3) + 16 * blockIdx.x + col] = sA[col];
    pc[MF_RZP + 16 * FPCG_CAP * ((it + 1) & 3) + 16 * blockIdx.x + col] = sB[col];
  }
}

// k_fpcg_direction per column: p = z + beta p with beta = r.z_new / r.z; the totals of this iteration's r.r and of the
// next r.z (zeros once the column has stopped, so that it stays stopped), and whether the column goes into the next
// iteration -- what k_fpcgm_spmm reads to leave a finished panel alone
__global__ __launch_bounds__(256) void k_fpcgm_direction(const double *z_all, double *p_all, int n, double *pc_all, int it,
                                                         double tol2, size_t vstride) {
  __shared__ double sW[256], sA[16], sB[16];
  double *pc = pc_all + (size_t)MF_ALL * blockIdx.y;
  const size_t off = vstride * blockIdx.y;
  const int col = threadIdx.x & 15;
  const double rz = pc[MF_RZ + 16 * (it & 3) + col], bb = pc[MF_BB + col];
  const bool stopped = pc[MF_FAIL + col] != 0.0 || fpcgm_converged_before(pc, col, it, rz, bb, tol2);
  fpcgm_sum_partials(pc + MF_RRP + 16 * FPCG_CAP * (it & 3), gridDim.x, sW, sA);
  fpcgm_sum_partials(pc + MF_RZP + 16 * FPCG_CAP * ((it + 1) & 3), gridDim.x, sW, sB);
  const double rr = sA[col], rzn = sB[col];
  if (blockIdx.x == 0 && threadIdx.x < 16) {
    pc[MF_RR + 16 * (it & 3) + col] = stopped ? 0.0 : rr;
    pc[MF_RZ + 16 * ((it + 1) & 3) + col] = stopped ? 0.0 : rzn;
    pc[MF_ACT + col] = stopped || rzn == 0.0 || rr <= tol2 * bb ? 0.0 : 1.0;
  }
  if (stopped) return;
  const double beta = rzn / rz;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < (size_t)16 * n; t += (size_t)gridDim.x * 256)
    p_all[off + t] = z_all[off + t] + beta * p_all[off + t];
}

// the chosen rows of a batch's solved columns into C [N][N], N = n_sel cnp: panel y holds the columns of the camera at
// position b = b0 + y of the chosen list; block (a, b), a >= b, = scale x rows of camera sel[a], written to both sides;
// of the diagonal block the lower triangle alone is read.  Rows and columns of dead coordinates are +0.0.  cols (may be
// null) [panels][cnp][nA]: the columns themselves, not scaled, dead rows +0.0
template <class T>
__global__ __launch_bounds__(256) void k_fcovm_gather(const double *x_all, size_t vstride, const int *sel, int n_sel, int b0,
                                                      unsigned mask, const unsigned short *cmask, const unsigned char *held,
                                                      double scale, double *C, double *cols, int nA) {
  constexpr int CNP = T::CNP, C2 = CNP * CNP;
  const double *x = x_all + vstride * blockIdx.y;
  const int b = b0 + blockIdx.y, camb = sel[b];
  const size_t N = (size_t)CNP * n_sel;
  const size_t nC_part = (size_t)C2 * n_sel, nall = nC_part + (cols ? (size_t)CNP * nA : 0);
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < nall; t += (size_t)gridDim.x * 256) {
    if (t < nC_part) {
      const int a = (int)(t / C2), i = (int)(t % C2) / CNP, nn = (int)(t % C2) % CNP;
      if (a < b || (a == b && i < nn)) continue;
      const int cama = sel[a];
      const bool live = fcm_live<T>(mask, cmask, held, cama, i) && fcm_live<T>(mask, cmask, held, camb, nn);
      const double v = live ? scale * x[(size_t)16 * (CNP * (size_t)cama + i) + nn] : 0.0;
      C[((size_t)CNP * a + i) * N + (size_t)CNP * b + nn] = v;
      C[((size_t)CNP * b + nn) * N + (size_t)CNP * a + i] = v;
    } else {
      const size_t u = t - nC_part;
      const int nn = (int)(u / nA), coord = (int)(u % nA);
      const bool live = fcm_live<T>(mask, cmask, held, camb, nn) && fcm_live<T>(mask, cmask, held, coord / CNP, coord % CNP);
      cols[((size_t)CNP * blockIdx.y + nn) * nA + coord] = live ? x[(size_t)16 * coord + nn] : 0.0;
    }
  }
}

// ---- host side ----

// the vector kernels' grid: a panel has 16 nA entries; at most FPCG_CAP workgroups, a function of nA alone
int fcm_vec_grid(int n) { return ((size_t)16 * n + 255) / 256 < (size_t)FPCG_CAP ? (int)(((size_t)16 * n + 255) / 256) : FPCG_CAP; }

// the verb's own buffers: six vectors [panels][nA][16] (x, r, z, p, q and r's second buffer), the panels' scalar blocks
// and the small block the inverse kernel reports into; allocated at first use, dropped with the problem
int fcm_buffers(psba_ctx *h, int panels) {
  if (h->fcm_cap < panels) {
    h->fcm_cap = 0;
    TRY(h->fcm_vec.alloc(h, (size_t)6 * panels * 16 * h->d.nA));
    h->fcm_cap = panels;
  }
  if (!h->fcm_scal) TRY(h->fcm_scal.alloc(h, (size_t)MF_ALL * FCOVM_PANELS + 16));
  if (!h->fcm_status) TRY(h->fcm_status.alloc(h, 4));
  if (!h->fcm_host) TRY(h->fcm_host.alloc(h, (size_t)MF_N * FCOVM_PANELS + 16));
  return PSBA_OK;
}

template <class T>
static int fbsr_times_many(psba_ctx *h, int n_panels, const double *X, double *Y) {
  const int n = h->d.nA, nC = h->d.nC;
  const size_t vs = (size_t)16 * n;
  for (int b0 = 0; b0 < n_panels; b0 += FCOVM_PANELS) {
    const int np = n_panels - b0 < FCOVM_PANELS ? n_panels - b0 : FCOVM_PANELS;
    TRY(fcm_buffers(h, np));
    double *p = h->fcm_vec, *q = p + vs * h->fcm_cap;
    PSBA_HIP(h, hipMemcpyAsync(p, X + vs * b0, sizeof(double) * vs * np, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_fpcgm_spmm<T>, dim3(fpcg_row_grid(nC), np), dim3(256), 0, h->stream, h->bs_val, h->bs_rowptr,
                       h->bs_rowent, nC, p, q, h->fcm_scal, 0, vs, 0);
    PSBA_HIP(h, hipGetLastError());
    PSBA_HIP(h, hipMemcpyAsync(Y + vs * b0, q, sizeof(double) * vs * np, hipMemcpyDeviceToHost, h->stream));
    PSBA_HIP(h, hipStreamSynchronize(h->stream));
  }
  return PSBA_OK;
}

// the columns of the chosen cameras in batches of at most FCOVM_PANELS panels, bursts of 8 iterations between host
// synchronisations; per column the host reads what fpcg_solve reads for its one.  Returns PSBA_OK, PSBA_NOT_SPD or
// PSBA_PCG_MAXIT (or an error)
template <class T>
static int fcm_compute(psba_ctx *h, double scale, int n_sel, const int *sel, double *C, double *cols, int *iters, double *relres) {
  constexpr int CNP = T::CNP;
  const int n = h->d.nA, nC = h->d.nC, g = fcm_vec_grid(n), gs = fpcg_row_grid(nC);
  const size_t vs = (size_t)16 * n, N = (size_t)CNP * n_sel;
  hipStream_t s = h->stream;
  const int cap = n_sel < FCOVM_PANELS ? n_sel : FCOVM_PANELS;
  TRY(fcm_buffers(h, cap));
  DevBuf<int> sel_dev;
  DevBuf<double> C_dev, cols_dev;
  TRY(sel_dev.alloc(h, (size_t)n_sel));
  TRY(C_dev.alloc(h, N * N));
  if (cols) TRY(cols_dev.alloc(h, (size_t)cap * CNP * n));
  PSBA_HIP(h, hipMemcpyAsync(sel_dev, sel, sizeof(int) * n_sel, hipMemcpyHostToDevice, s));
  const size_t vc = vs * h->fcm_cap;
  double *x = h->fcm_vec, *r0 = x + vc, *z = r0 + vc, *p = z + vc, *q = p + vc, *r1 = q + vc;
  double *pc = h->fcm_scal, *ipc = pc + (size_t)MF_ALL * FCOVM_PANELS, *hs = h->fcm_host, *ihs = hs + (size_t)MF_N * FCOVM_PANELS;
  const int zero4[4] = {0, 0, 0, 0}, stamp = 1;
  const unsigned char *held = h->has_held ? h->held_poses.get() : nullptr;
  const double tol2 = h->pcg_tol * h->pcg_tol;
  ProfScope ps(h, PSBA_K_CHOLESKY);
  PSBA_HIP(h, hipMemsetAsync(ipc, 0, sizeof(double) * 16, s));
  PSBA_HIP(h, hipMemcpyAsync(h->fcm_status, zero4, sizeof zero4, hipMemcpyHostToDevice, s));
  TRY(launch_fbsr_diag_inverse(h, h->pcg_minv, ipc, h->fcm_status, stamp));
  bool not_spd = false, exhausted = false;
  for (int b0 = 0; b0 < n_sel; b0 += FCOVM_PANELS) {
    const int np = n_sel - b0 < FCOVM_PANELS ? n_sel - b0 : FCOVM_PANELS;
    hipLaunchKernelGGL(k_fpcgm_start<T>, dim3(g, np), dim3(256), 0, s, sel_dev.get() + b0, h->kd_mask, h->kd_cmask.get(), held,
                       h->pcg_minv.get(), x, r0, z, p, q, n, pc, vs);
    std::vector<char> open((size_t)16 * np, 1);
    std::vector<int> its((size_t)16 * np, 0);
    std::vector<double> rel((size_t)16 * np, 0.0);
    bool any_open = true;
    for (int it = 0; any_open;) {
      const int burst = it + 8 < h->pcg_maxit ? 8 : h->pcg_maxit - it;
      int last = it;
      for (int k = 0; k < burst; k++, it++) {
        double *rc = (it & 1) ? r1 : r0, *rn = (it & 1) ? r0 : r1;
        hipLaunchKernelGGL(k_fpcgm_spmm<T>, dim3(gs, np), dim3(256), 0, s, h->bs_val, h->bs_rowptr, h->bs_rowent, nC, p, q, pc,
                           it & 3, vs, 1);
        hipLaunchKernelGGL(k_fpcgm_update<T>, dim3(g, np), dim3(256), 0, s, x, rc, rn, p, q, h->pcg_minv.get(), z, n, pc, it, gs,
                           tol2, vs);
        hipLaunchKernelGGL(k_fpcgm_direction, dim3(g, np), dim3(256), 0, s, z, p, n, pc, it, tol2, vs);
        last = it;
      }
      PSBA_HIP(h, hipMemcpy2DAsync(hs, sizeof(double) * MF_N, pc, sizeof(double) * MF_ALL, sizeof(double) * MF_N, np,
                                   hipMemcpyDeviceToHost, s));
      PSBA_HIP(h, hipMemcpyAsync(ihs, ipc, sizeof(double) * 16, hipMemcpyDeviceToHost, s));
      PSBA_HIP(h, hipGetLastError());
      PSBA_HIP(h, hipStreamSynchronize(s));
      if (ihs[1] != 0.0) not_spd = true;  // a bad pivot of a diagonal block (k_fbsr_diag_inverse's fail slot)
      any_open = false;
      for (int y = 0; y < np; y++) {
        const double *c = hs + (size_t)MF_N * y;
        for (int col = 0; col < CNP; col++) {
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
    const size_t work = (size_t)CNP * CNP * n_sel + (cols ? (size_t)CNP * n : 0);
    const int gg = (int)((work + 255) / 256 < 1024 ? (work + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_fcovm_gather<T>, dim3(gg, np), dim3(256), 0, s, x, vs, sel_dev.get(), n_sel, b0, h->kd_mask,
                       h->kd_cmask.get(), held, scale, C_dev.get(), cols ? cols_dev.get() : nullptr, n);
    PSBA_HIP(h, hipGetLastError());
    if (cols)
      PSBA_HIP(h, hipMemcpyAsync(cols + (size_t)CNP * b0 * n, cols_dev, sizeof(double) * (size_t)CNP * np * n, hipMemcpyDeviceToHost, s));
    PSBA_HIP(h, hipStreamSynchronize(s));
    for (int y = 0; y < np; y++)
      for (int col = 0; col < CNP; col++) {
        if (iters) iters[(size_t)CNP * (b0 + y) + col] = its[16 * y + col];
        if (relres) relres[(size_t)CNP * (b0 + y) + col] = rel[16 * y + col];
      }
  }
  PSBA_HIP(h, hipMemcpyAsync(C, C_dev, sizeof(double) * N * N, hipMemcpyDeviceToHost, s));
  PSBA_HIP(h, hipStreamSynchronize(s));
  return not_spd ? PSBA_NOT_SPD : exhausted ? PSBA_PCG_MAXIT : PSBA_OK;
}

// for kernels_free_pcg_points.hip (free_pcg_many.h): iterations it0 .. it0 + burst - 1 on the first np panels of the
// verbs' buffers, launched exactly as fcm_compute launches them
template <class T>
static int fcm_burst(psba_ctx *h, int np, int it0, int burst) {
  const int n = h->d.nA, nC = h->d.nC, g = fcm_vec_grid(n), gs = fpcg_row_grid(nC);
  const size_t vs = (size_t)16 * n, vc = vs * h->fcm_cap;
  hipStream_t s = h->stream;
  double *x = h->fcm_vec, *r0 = x + vc, *z = r0 + vc, *p = z + vc, *q = p + vc, *r1 = q + vc, *pc = h->fcm_scal;
  const double tol2 = h->pcg_tol * h->pcg_tol;
  for (int it = it0; it < it0 + burst; it++) {
    double *rc = (it & 1) ? r1 : r0, *rn = (it & 1) ? r0 : r1;
    hipLaunchKernelGGL(k_fpcgm_spmm<T>, dim3(gs, np), dim3(256), 0, s, h->bs_val, h->bs_rowptr, h->bs_rowent, nC, p, q, pc,
                       it & 3, vs, 1);
    hipLaunchKernelGGL(k_fpcgm_update<T>, dim3(g, np), dim3(256), 0, s, x, rc, rn, p, q, h->pcg_minv.get(), z, n, pc, it, gs,
                       tol2, vs);
    hipLaunchKernelGGL(k_fpcgm_direction, dim3(g, np), dim3(256), 0, s, z, p, n, pc, it, tol2, vs);
  }
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

#define FPCGM_DISPATCH(fn, ...) (h->cnp == KD_CNP ? fn<FreeKD>(__VA_ARGS__) : fn<FreeK>(__VA_ARGS__))
int launch_fbsr_times_many(psba_ctx *h, int n_panels, const double *X, double *Y) {
  return FPCGM_DISPATCH(fbsr_times_many, h, n_panels, X, Y);
}
int launch_fcovm_compute(psba_ctx *h, double scale, int n_sel, const int *sel, double *C, double *cols, int *iters, double *relres) {
  return FPCGM_DISPATCH(fcm_compute, h, scale, n_sel, sel, C, cols, iters, relres);
}

int launch_fpcgm_burst(psba_ctx *h, int np, int it0, int burst) { return FPCGM_DISPATCH(fcm_burst, h, np, it0, burst); }

}  // namespace psba
