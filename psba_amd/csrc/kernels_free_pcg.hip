// kernels_free_pcg.hip -- block-sparse S and conjugate gradients on the free-intrinsics camera blocks of 11 and 16
// (PSBA_SOLVER_SPARSE, psba_schur_path = 6).  What kernels_pcg.hip is to the blocks of 6:
//   * storage: the lower block triangle as a list of CNP x CNP blocks (bs_jk[b] = (j, k), k <= j, bs_val[b][CNP^2]
//     row-major), every diagonal block present -- the plan's blocks plus one for each camera without a product
//     (build_block_rows, blockprod_plan.cpp).  k_free_schur / k_free_combine (kernels_free.hip, LIST instantiation)
//     store each block once, k_fbsr_finalize adds U and the damping;
//   * solve: conjugate gradients on S x = e_a, preconditioned with the inverses of the diagonal blocks, with the
//     recurrences, the four-slot rotation of the scalars and the stop rule of kernels_pcg.hip (test before an
//     iteration on the previous r.r, r.z == 0 counts as converged, bursts of 8 per host synchronisation);
//   * intrinsics shared between cameras (psba_set_sparse_intrinsics_groups, blocks of 16): the list stays
//     unfolded and undamped and the solve folds -- p kept expanded, a launch behind the product that sums the members' q,
//     the block Jacobi of the folded matrix.  Every launch site tests h->kd_rep: without groups nothing changes.
// RULE OF THE ROUTE (kernels_free.hip): no floating-point atomics.  q = S p is formed by one wave per block row in the
// order of the row walk; every inner product is written as one partial sum per workgroup of a persistent grid (at most
// FPCG_CAP of them) and every workgroup of the consuming kernel adds the partials in the same order, so all agree
// without a hand-shake and two solves of the same blocks give the same bits.
#include "free_blocks.h"
#include "psba_internal.h"

namespace psba {

// the scalar block (doubles, device): the totals of kernels_pcg.hip's layout, then the partial sums.  p.Sp, r.r and
// r.z of iteration `it` live in slot it % 4 (r.z of the next iteration in slot (it + 1) % 4).  A partial array is
// written whole by its producer before any consumer runs, so nothing is ever zeroed between iterations; the totals
// PF_RR / PF_RZ are written by workgroup 0 of k_fpcg_direction (PF_BB and r.z of slot 0 by k_fpcg_update at it = 0),
// into slots no workgroup of that launch reads
enum { PF_BB = 0, PF_FAIL = 1, PF_DONE = 2, PF_RRFIN = 3, PF_RR = 4, PF_RZ = 8, PF_N = 16,
       PF_PQP = 16, PF_RRP = 16 + 4 * FPCG_CAP, PF_RZP = 16 + 8 * FPCG_CAP, PF_BBP = 16 + 12 * FPCG_CAP,
       PF_ALL = 16 + 13 * FPCG_CAP };
constexpr int FSPMV_TRIP = 4;  // blocks of a row whose loads are in flight together (k_fpcg_spmv)
constexpr int FINV_CAMS = 8;   // cameras of a workgroup of k_fbsr_diag_inverse, 16 lanes each

// the sum of the workgroup's 256 values, the same bits in every thread: a shuffle tree per wave, then wave 0 .. 3
__device__ __forceinline__ double fpcg_block_sum(double v, double *sRed) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
  __syncthreads();
  return s;
}
// the sum of n <= FPCG_CAP <= 256 partials: every workgroup that calls this gets the same bits
__device__ __forceinline__ double fpcg_sum_partials(const double *part, int n, double *sRed) {
  return fpcg_block_sum((int)threadIdx.x < n ? part[threadIdx.x] : 0.0, sRed);
}
__device__ __forceinline__ bool fpcg_converged_before(const double *pc, int it, double rz, double bb, double tol2) {
  if (rz == 0.0) return true;
  return it > 0 && pc[PF_RR + ((it - 1) & 3)] <= tol2 * bb;
}

// diagonal blocks += U_j, + mu (mu D_r) on the diagonal -- the block of a camera without a product is written whole
// (nothing else stores it); e_a = g_a - the units' sums in unit order; the accumulators of the try's back-substitution
// zeroed, the try stamp set.  One thread per entry of a diagonal block and per coordinate: O(blocks)
template <class T>
__global__ __launch_bounds__(256) void k_fbsr_finalize(double *val, const int *diag, double *ea, const double *U,
                                                       const double *ga, const double *eapart, const int *cuptr, double mu,
                                                       const double *D, int nC, double *scal, int *status, int try_id) {
  constexpr int CNP = T::CNP, C2 = CNP * CNP;
  if (blockIdx.x == 0 && threadIdx.x < 4 * SC_NPART) scal[SC_PART + threadIdx.x] = 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 64) status[3] = try_id;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nU = (size_t)C2 * nC;
  if (t < nU) {
    const int j = (int)(t / C2), e = (int)(t % C2);
    const int ds = diag[j];
    double *dst = val + (size_t)C2 * (ds & ~FBSR_ADDED) + e;
    double v = (ds & FBSR_ADDED) ? U[t] : *dst + U[t];
    if (e / CNP == e % CNP) v += D ? mu * D[CNP * (size_t)j + e / CNP] : mu;
    *dst = v;
  } else if (t < nU + (size_t)CNP * nC) {
    const size_t c = t - nU;
    const int j = (int)(c / CNP), r = (int)(c % CNP);
    double s = 0.0;
    for (int u = cuptr[j]; u < cuptr[j + 1]; u++) s += eapart[CNP * (size_t)u + r];
    ea[c] = ga[c] - s;
  }
}

// inverse of every diagonal block: Cholesky of the CNP x CNP block read through its lower triangle, X = L^-1, then
// M = X^T X -- the loops of k_bsr_diag_inverse spread over 16 lanes, the block in LDS (a thread per camera would keep
// three 16 x 16 arrays in scratch).  Lane r of a camera's 16 owns row r of L, column r of X and row r of M; every sum
// runs in ascending k.  A coordinate whose row and column are zero off the diagonal (masked, held) keeps exact zeros
// in its row and column of L, X and M.  A pivot that is not > 0 sets status[1] and the fail slot.
// GRP (shared intrinsics; the list holds undamped blocks): the input block of a representative is the folded
// one k_fgrp_sum built (mu D added there); every other camera's is its own plus mu D, with the rows and columns of the
// folded-away coordinates of a member replaced by the placeholder coeff + mu D.  The three loops are the same
struct FgInv {
  KdGroups G;
  const double *fblk;  // [nmg][256]
  const double *D;     // null: I
  double mu, coeff;
};
template <class T, bool GRP>
__global__ __launch_bounds__(16 * FINV_CAMS) void k_fbsr_diag_inverse(const double *val, const int *diag, double *minv,
                                                                       int nC, double *pc, int *status, int try_id, FgInv fi) {
  constexpr int CNP = T::CNP, C2 = CNP * CNP, LD = 17;
  __shared__ double sA[FINV_CAMS][16 * LD], sX[FINV_CAMS][16 * LD];
  const int g = threadIdx.x >> 4, r = threadIdx.x & 15;
  const int j = blockIdx.x * FINV_CAMS + g;
  const bool valid = j < nC;
  double *A = sA[g], *X = sX[g];
  if (valid && GRP) {
    const int grp = fi.G.gidx[j];
    const bool isrep = grp >= 0 && fi.G.rep[j] == j;
    const unsigned away = grp >= 0 && !isrep ? kd_free_bits(fi.G.mask, fi.G.cmask, j) & 0x3FFu : 0u;
    const double *a = isrep ? fi.fblk + (size_t)C2 * grp : val + (size_t)C2 * (diag[j] & ~FBSR_ADDED);
    for (int e = r; e < C2; e += 16) {
      const int i = e / CNP, c = e % CNP;
      double v = a[e];
      if (!isrep) {
        if (((away >> i) | (away >> c)) & 1u) v = i == c ? fi.coeff : 0.0;
        if (i == c) v += fi.D ? fi.mu * fi.D[CNP * (size_t)j + i] : fi.mu;
      }
      A[LD * i + c] = v;
    }
  } else if (valid) {
    const double *a = val + (size_t)C2 * (diag[j] & ~FBSR_ADDED);
    for (int e = r; e < C2; e += 16) A[LD * (e / CNP) + e % CNP] = a[e];  // (the strict upper triangle is never read back)
  } else {
    for (int c = 0; c < CNP; c++) A[LD * r + c] = r == c ? 1.0 : 0.0;
  }
  bool bad = false;
  for (int c = 0; c < CNP; c++) {
    __syncthreads();
    double v = 0.0;
    if (r >= c && r < CNP) {
      v = A[LD * r + c];
      for (int k = 0; k < c; k++) v -= A[LD * r + k] * A[LD * c + k];
    }
    const double d = __shfl(v, c, 16);
    if (!(d > 0.0)) bad = true;
    const double s = sqrt(d), is = 1.0 / s;
    if (r == c)
      A[LD * r + c] = s;
    else if (r > c && r < CNP)
      A[LD * r + c] = v * is;
  }
  __syncthreads();
  if (r < CNP) {  // column r of X = L^-1
    for (int i = r; i < CNP; i++) {
      if (i == r) {
        X[LD * i + r] = 1.0 / A[LD * i + i];
      } else {
        double v = 0.0;
        for (int k = r; k < i; k++) v -= A[LD * i + k] * X[LD * k + r];
        X[LD * i + r] = v / A[LD * i + i];
      }
    }
  }
  __syncthreads();
  if (r < CNP) {  // row r of M, into A (L is not read any more)
    for (int c = 0; c < CNP; c++) {
      double v = 0.0;
      for (int k = r > c ? r : c; k < CNP; k++) v += X[LD * k + r] * X[LD * k + c];
      A[LD * r + c] = v;
    }
  }
  __syncthreads();
  if (valid) {
    double *m = minv + (size_t)C2 * j;
    for (int e = r; e < C2; e += 16) m[e] = A[LD * (e / CNP) + e % CNP];
    if (bad && r == 0) {
      status[1] = try_id;
      pc[PF_FAIL] = 1.0;
    }
  }
}

// q = S p and the partial sums of p.q: one wave per block row (a persistent grid of at most FPCG_CAP workgroups of four
// waves, rows in grid stride), the row's entries in the order of the walk.  A block is read in the shape of the MFMA
// accumulator tile: lane (k = lane >> 4, col = lane & 15) holds B[k + 4 t][col], t < 4, so each of the four loads of a
// wave covers four whole rows of the block -- 512 contiguous bytes of a block of 16, 352 of a block of 11, whose idle
// lanes (col >= 11, row >= 11) supply 0.0.  (Blocks of 11 start at odd multiples of 8 bytes, so the loads are 8 bytes
// wide.)  A block as stored adds B[row][col] x[col] to row's sum, a transposed one B[row][col] x[row] to col's sum, the
// diagonal block both through its lower triangle; the two kinds of sums are reduced across lanes once per row, by
// butterflies over the 16 lanes of a row and over the four lanes of a column.  FSPMV_TRIP blocks' loads are in flight
// together; the order of the adds is the order of the walk whatever the trip
template <class T>
__global__ __launch_bounds__(256) void k_fpcg_spmv(const double *val, const int *rowptr, const int2 *rowent, int nC,
                                                   const double *p, double *q, double *pqpart) {
  constexpr int CNP = T::CNP, C2 = CNP * CNP;
  __shared__ double sRed[4];
  const int lane = threadIdx.x & 63, k = lane >> 4, col = lane & 15;
  const bool live = CNP == 16 || col < CNP;
  const int ccol = live ? col : 0;
  double pq = 0.0;
  for (int j = blockIdx.x * 4 + (threadIdx.x >> 6); j < nC; j += gridDim.x * 4) {
    double aN[4] = {0.0, 0.0, 0.0, 0.0}, aT = 0.0;
    const int e1 = rowptr[j + 1];
    for (int e0 = rowptr[j]; e0 < e1; e0 += FSPMV_TRIP) {
      double b[FSPMV_TRIP][4], xr[FSPMV_TRIP][4], xc[FSPMV_TRIP];
      int how[FSPMV_TRIP];
#pragma unroll
      for (int u = 0; u < FSPMV_TRIP; u++) {
        const bool on = e0 + u < e1;
        const int2 en = on ? rowent[e0 + u] : make_int2(0, 0);
        how[u] = on ? en.y >> 28 : 3;  // 3: nothing
        const double *B = val + (size_t)C2 * en.x;
        const double *xo = p + (size_t)CNP * (en.y & 0x0fffffff);
        xc[u] = on && live ? xo[ccol] : 0.0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const int row = k + 4 * t;
          const bool in = on && live && (CNP == 16 || row < CNP);
          b[u][t] = in ? B[CNP * row + ccol] : 0.0;
          xr[u][t] = in ? xo[row] : 0.0;
        }
      }
#pragma unroll
      for (int u = 0; u < FSPMV_TRIP; u++) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const int row = k + 4 * t;
          const bool asN = how[u] == 0 || (how[u] == 2 && col <= row);
          const bool asT = how[u] == 1 || (how[u] == 2 && col < row);
          aN[t] += asN ? b[u][t] * xc[u] : 0.0;
          aT += asT ? b[u][t] * xr[u][t] : 0.0;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) aN[t] += __shfl_xor(aN[t], m, 64);
    }
    aT += __shfl_xor(aT, 16, 64);
    aT += __shfl_xor(aT, 32, 64);
    // row `col` of the result: its as-stored sum sits in the lanes k = col & 3 (register col >> 2), its transposed sum
    // in every lane of column col
    const int t = col >> 2;
    const double yN = t == 0 ? aN[0] : t == 1 ? aN[1] : t == 2 ? aN[2] : aN[3];
    if (live && k == (col & 3)) {
      const double y = yN + aT;
      q[(size_t)CNP * j + col] = y;
      pq += p[(size_t)CNP * j + col] * y;
    }
  }
  const double s = fpcg_block_sum(pq, sRed);
  if (threadIdx.x == 0) pqpart[blockIdx.x] = s;
}

// start: x = 0, r = b, z = M^-1 r, p = z, q = 0; the partials of r.z (slot 0) and b.b.  One thread per unknown in grid
// stride (the grid of k_fpcg_update).  GRP (shared intrinsics): p is kept expanded -- the thread of a
// folded-away entry forms its representative's z itself, from b and the inverses, which this launch does not write
template <class T, bool GRP>
__global__ __launch_bounds__(256) void k_fpcg_start(const double *b, const double *minv, double *x, double *r, double *z,
                                                    double *p, double *q, int n, double *pc, KdGroups G) {
  constexpr int CNP = T::CNP;
  __shared__ double sRed[4];
  double rz = 0.0, bb = 0.0;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
    const int j = t / CNP, row = t % CNP;
    const double *m = minv + (size_t)(CNP * CNP) * j + CNP * row;
    const double *bj = b + (size_t)CNP * j;
    double zz = 0.0;
#pragma unroll
    for (int c = 0; c < CNP; c++) zz += m[c] * bj[c];
    const double bt = b[t];
    double pz = zz;
    if (GRP && kd_folded(G, t)) {
      const int jr = G.rep[j];
      const double *mr = minv + (size_t)(CNP * CNP) * jr + CNP * row, *br = b + (size_t)CNP * jr;
      pz = 0.0;
#pragma unroll
      for (int c = 0; c < CNP; c++) pz += mr[c] * br[c];
    }
    x[t] = 0.0;
    r[t] = bt;
    z[t] = zz;
    p[t] = pz;
    q[t] = 0.0;
    rz += bt * zz;
    bb += bt * bt;
  }
  const double s0 = fpcg_block_sum(rz, sRed), s1 = fpcg_block_sum(bb, sRed);
  if (threadIdx.x == 0) {
    pc[PF_RZP + blockIdx.x] = s0;
    pc[PF_BBP + blockIdx.x] = s1;
  }
}

// x += alpha p, r -= alpha q with alpha = r.z / p.Sp; z = M^-1 r with the camera's block -- a thread forms the new
// residual of all rows of its camera itself from the old r (r is kept in two buffers used in turn), as k_pcg_update
// does; the partials of r.r and of the next r.z.  npq: the partials of p.Sp (the grid of k_fpcg_spmv)
template <class T>
__global__ __launch_bounds__(256) void k_fpcg_update(double *x, const double *r, double *rn, const double *p, const double *q,
                                                     const double *minv, double *z, int n, double *pc, int it, int npq,
                                                     int *status, int try_id, double tol2) {
  constexpr int CNP = T::CNP;
  __shared__ double sRed[4];
  const double pq = fpcg_sum_partials(pc + PF_PQP + FPCG_CAP * (it & 3), npq, sRed);
  double rz, bb;
  if (it == 0) {  // the start kernel's partials: every workgroup adds them itself, workgroup 0 keeps the totals
    rz = fpcg_sum_partials(pc + PF_RZP, gridDim.x, sRed);
    bb = fpcg_sum_partials(pc + PF_BBP, gridDim.x, sRed);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      pc[PF_RZ] = rz;
      pc[PF_BB] = bb;
    }
  } else {
    rz = pc[PF_RZ + (it & 3)];
    bb = pc[PF_BB];
  }
  if (fpcg_converged_before(pc, it, rz, bb, tol2)) {  // the rest of a burst after convergence: nothing to do
    if (blockIdx.x == 0 && threadIdx.x == 0 && pc[PF_DONE] == 0.0) {
      pc[PF_RRFIN] = it > 0 ? pc[PF_RR + ((it - 1) & 3)] : 0.0;
      pc[PF_DONE] = (double)(it + 1);  // it iterations were carried out (+1: zero means "not yet")
    }
    return;
  }
  if (!(pq > 0.0)) {  // not positive definite (or a break-down): the LM loop raises mu
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      status[1] = try_id;
      pc[PF_FAIL] = 1.0;
    }
    return;
  }
  const double alpha = rz / pq;
  double rr = 0.0, rzn = 0.0;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
    const int j = t / CNP, row = t % CNP;
    const double *m = minv + (size_t)(CNP * CNP) * j + CNP * row;
    double zz = 0.0, own = 0.0;
#pragma unroll
    for (int c = 0; c < CNP; c++) {
      const double rc = r[(size_t)CNP * j + c] - alpha * q[(size_t)CNP * j + c];
      zz += m[c] * rc;
      own = c == row ? rc : own;
    }
    x[t] += alpha * p[t];
    rn[t] = own;
    z[t] = zz;
    rr += own * own;
    rzn += own * zz;
  }
  const double s0 = fpcg_block_sum(rr, sRed), s1 = fpcg_block_sum(rzn, sRed);
  if (threadIdx.x == 0) {
    pc[PF_RRP + FPCG_CAP * (it & 3) + blockIdx.x] = s0;
    pc[PF_RZP + FPCG_CAP * ((it + 1) & 3) + blockIdx.x] = s1;
  }
}

// p = z + beta p with beta = r.z_new / r.z; the totals of this iteration's r.r and of the next r.z (zeros once the
// solve has converged, so that it stays converged: k_fpcg_update wrote no partials then).  GRP: a folded-away entry t
// takes z[rep(t)] + beta p[t] -- p[t] has its representative's bits by induction, so the result has them too, and the
// launch reads nothing that it writes but the entry's own p
template <bool GRP>
__global__ __launch_bounds__(256) void k_fpcg_direction(const double *z, double *p, int n, double *pc, int it, double tol2,
                                                        KdGroups G) {
  __shared__ double sRed[4];
  const double rz = pc[PF_RZ + (it & 3)], bb = pc[PF_BB];
  if (fpcg_converged_before(pc, it, rz, bb, tol2)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      pc[PF_RR + (it & 3)] = 0.0;
      pc[PF_RZ + ((it + 1) & 3)] = 0.0;
    }
    return;
  }
  const double rr = fpcg_sum_partials(pc + PF_RRP + FPCG_CAP * (it & 3), gridDim.x, sRed);
  const double rzn = fpcg_sum_partials(pc + PF_RZP + FPCG_CAP * ((it + 1) & 3), gridDim.x, sRed);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    pc[PF_RR + (it & 3)] = rr;
    pc[PF_RZ + ((it + 1) & 3)] = rzn;
  }
  const double beta = rzn / rz;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
    const int s = GRP && kd_folded(G, t) ? KD_CNP * G.rep[t / KD_CNP] + t % KD_CNP : t;
    p[t] = z[s] + beta * p[t];
  }
}

// ---- intrinsics shared between cameras under this solver (psba_set_sparse_intrinsics_groups) ----
// Blocks of 16 only, and only on a handle with groups.  The list keeps S0, the unfolded blocks without damping; the
// solve works on A = P^T S0 P + mu D, embedded at nA (a folded-away coordinate: coeff + mu D on the diagonal, zero
// elsewhere, e_a = 0).  Every sum over the members of a group runs in ascending camera order.
constexpr int FG_PART = 10 * KD_CNP;  // doubles of a member's partial: the ten intrinsic rows of the folded block

// the placeholder's product, rounded operation by operation (no contraction: tests hold it to the bit)
__device__ __forceinline__ double fg_placeholder(double coeff, double mu, const double *D, size_t t, double x) {
#pragma clang fp contract(off)
  const double d = coeff + (D ? mu * D[t] : mu);
  return d * x;
}

// e_a folded, a launch behind k_fbsr_finalize: thread (group, k) sums the members' entries in the order of
// k_kd_fold_cols on the e_a row (so the bits are those of the dense route) and clears the folded-away ones itself
__global__ __launch_bounds__(256) void k_fbsr_fold_ea(double *ea, KdGroups G) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 10 * G.nmg) return;
  const int g = t / 10, k = t % 10;
  const int m0 = G.gptr[g], m1 = G.gptr[g + 1];
  if (!((kd_free_bits(G.mask, G.cmask, G.gmem[m0]) >> k) & 1u)) return;  // (the members carry equal rows)
  double s = 0.0;
  for (int q = m0; q < m1; q++) s += ea[KD_CNP * (size_t)G.gmem[q] + k];
  ea[KD_CNP * (size_t)G.gmem[m0] + k] = s;
  for (int q = m0 + 1; q < m1; q++) ea[KD_CNP * (size_t)G.gmem[q] + k] = 0.0;
}

// The folded diagonal block of a representative r, rows k < 10 shared: (k, c) = sum over the members m of
// S0[(m, k)][(r, c)] for a column c that is not shared, sum over m and m' of S0[(m, k)][(m', c)] for one that is.
// First step: one wave per member m walks m's block row in the order of bs_rowent and keeps, of every block whose other
// camera is of m's group, the entries that belong to the sums -- lane (k = lane >> 4 (+ 4, + 8), c = lane & 15), the
// diagonal block read through its lower triangle -- and writes its 10 x 16 partial.  A missing block is zero
__global__ __launch_bounds__(256) void k_fgrp_partial(const double *val, const int *rowptr, const int2 *rowent, KdGroups G,
                                                      int nmem, double *part) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nmem) return;
  const int lane = threadIdx.x & 63, kr = lane >> 4, c = lane & 15;
  const int m = G.gmem[q], g = G.gidx[m], r = G.rep[m];
  const unsigned bits = kd_free_bits(G.mask, G.cmask, m) & 0x3FFu;
  const bool cshared = (bits >> c) & 1u;
  double acc[3] = {0.0, 0.0, 0.0};
  const int e1 = rowptr[m + 1];
  for (int e = rowptr[m]; e < e1; e++) {
    const int2 en = rowent[e];
    const int o = en.y & 0x0fffffff, how = en.y >> 28;
    if (G.gidx[o] != g) continue;
    const bool take = cshared || o == r;
    const double *B = val + (size_t)(KD_CNP * KD_CNP) * en.x;
#pragma unroll
    for (int t = 0; t < 3; t++) {
      const int k = kr + 4 * t;  // (k < 12: inside the block)
      const bool asrow = how == 0 || (how == 2 && k >= c);
      const double v = B[asrow ? KD_CNP * k + c : KD_CNP * c + k];
      acc[t] += take && ((bits >> k) & 1u) ? v : 0.0;
    }
  }
#pragma unroll
  for (int t = 0; t < 3; t++) {
    const int k = kr + 4 * t;
    if (k < 10) part[(size_t)FG_PART * q + KD_CNP * k + c] = acc[t];
  }
}

// Second step: thread (group, i, j <= i) adds the partials of the group in ascending member order -- row i of the
// partials where i is shared, row j, column i where only j is -- or takes the representative's own entry where neither
// is; mu D on the diagonal; the entry and its mirror
__global__ __launch_bounds__(256) void k_fgrp_sum(const double *val, const int *diag, const double *part, KdGroups G, double mu,
                                                  const double *D, double *blk) {
  const int g = blockIdx.x, i = threadIdx.x >> 4, j = threadIdx.x & 15;
  if (j > i) return;
  const int m0 = G.gptr[g], m1 = G.gptr[g + 1], r = G.gmem[m0];
  const unsigned bits = kd_free_bits(G.mask, G.cmask, r) & 0x3FFu;
  const bool is = (bits >> i) & 1u, js = (bits >> j) & 1u;
  double v;
  if (!is && !js) {
    v = val[(size_t)(KD_CNP * KD_CNP) * (diag[r] & ~FBSR_ADDED) + KD_CNP * i + j];
  } else {
    const int at = is ? KD_CNP * i + j : KD_CNP * j + i;
    v = 0.0;
    for (int q = m0; q < m1; q++) v += part[(size_t)FG_PART * q + at];
  }
  if (i == j) v += D ? mu * D[KD_CNP * (size_t)r + i] : mu;
  double *b = blk + (size_t)(KD_CNP * KD_CNP) * g;
  b[KD_CNP * i + j] = v;
  b[KD_CNP * j + i] = v;
}

// q <- P^T q + mu D p behind k_fpcg_spmv, and the partials of p.q over the kept coordinates into the slot k_fpcg_update
// reads (the grid of k_fpcg_update: its workgroups' count replaces the product kernel's).  The thread of a
// representative's shared entry sums the members' q and clears the folded-away ones itself: no other thread touches
// them.  xdiag (psba_sparse_S_times): a folded-away entry gets its placeholder times xdiag in the place of 0
__global__ __launch_bounds__(256) void k_fpcg_fold(double *q, const double *p, KdGroups G, double coeff, double mu,
                                                   const double *D, const double *xdiag, int n, double *pqpart) {
  __shared__ double sRed[4];
  double pq = 0.0;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
    const int j = t / KD_CNP, k = t % KD_CNP;
    const bool sh = k < 10 && ((kd_free_bits(G.mask, G.cmask, j) >> k) & 1u);
    const int g = sh ? G.gidx[j] : -1;
    if (g >= 0 && G.rep[j] != j) continue;
    double s = q[t];
    if (g >= 0) {
      const int m0 = G.gptr[g], m1 = G.gptr[g + 1];
      s = 0.0;
      for (int u = m0; u < m1; u++) s += q[KD_CNP * (size_t)G.gmem[u] + k];
      for (int u = m0 + 1; u < m1; u++) {
        const size_t tm = KD_CNP * (size_t)G.gmem[u] + k;
        q[tm] = xdiag ? fg_placeholder(coeff, mu, D, tm, xdiag[tm]) : 0.0;
      }
    }
    const double y = s + (D ? mu * D[t] : mu) * p[t];
    q[t] = y;
    pq += p[t] * y;
  }
  const double tot = fpcg_block_sum(pq, sRed);
  if (threadIdx.x == 0) pqpart[blockIdx.x] = tot;
}

// psba_sparse_S_times under groups: p = P x (a folded-away entry takes its representative's x)
__global__ __launch_bounds__(256) void k_fpcg_expand(const double *x, double *p, KdGroups G, int n) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < n) p[t] = x[kd_folded(G, t) ? KD_CNP * G.rep[t / KD_CNP] + t % KD_CNP : t];
}

template <class T>
static int fbsr_finalize(psba_ctx *h, double mu, const double *D) {
  const int nC = h->d.nC;
  const size_t n = (size_t)(T::CNP * T::CNP + T::CNP) * nC;
  const bool grp = T::CNP == KD_CNP && h->kd_rep;  // shared intrinsics: S0 without damping, then e_a folded
  h->bs_mu = mu;
  h->bs_D = D;
  ProfScope ps(h, PSBA_K_SCHUR);
  hipLaunchKernelGGL(k_fbsr_finalize<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->bs_val, h->bs_diag,
                     h->bs_ea, h->U, h->ga, h->free_eapart, h->free_cuptr, grp ? 0.0 : mu, grp ? nullptr : D, nC, h->scal,
                     h->status, h->try_id);
  if (grp)
    hipLaunchKernelGGL(k_fbsr_fold_ea, dim3((unsigned)((10 * h->kd_nmg + 255) / 256)), dim3(256), 0, h->stream, h->bs_ea,
                       kd_groups(h));
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

// q = A p behind the block product under groups: the fold's launch (grid and partials of k_fpcg_update)
static void fpcg_fold(psba_ctx *h, double *q, const double *p, const double *xdiag, int n, double *pqpart) {
  hipLaunchKernelGGL(k_fpcg_fold, dim3(fpcg_vec_grid(n)), dim3(256), 0, h->stream, q, p, kd_groups(h), h->coeff, h->bs_mu,
                     h->bs_D, xdiag, n, pqpart);
}

// y = S x with the solve's own product kernel (psba_sparse_S_times): x goes into the solve's p, the product into its q
// (both free between solves), the partials of x.Sx into slot 0 -- launch_fpcg_solve clears the scalar block.  Under
// groups y = A x with the solve's three steps: x into r's second buffer, p = P x, the block product, the fold
template <class T>
static int fbsr_times(psba_ctx *h, const double *x_host, double *y_host) {
  const int n = h->d.nA, nC = h->d.nC;
  double *p = h->pcg_vec + 2 * (size_t)n, *q = p + n, *x = q + n;
  const bool grp = T::CNP == KD_CNP && h->kd_rep;
  PSBA_HIP(h, hipMemcpyAsync(grp ? x : p, x_host, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  if (grp) hipLaunchKernelGGL(k_fpcg_expand, dim3((n + 255) / 256), dim3(256), 0, h->stream, x, p, kd_groups(h), n);
  hipLaunchKernelGGL(k_fpcg_spmv<T>, dim3(fpcg_row_grid(nC)), dim3(256), 0, h->stream, h->bs_val, h->bs_rowptr, h->bs_rowent,
                     nC, p, q, h->pcg_scal + PF_PQP);
  if (grp) fpcg_fold(h, q, p, x, n, h->pcg_scal + PF_PQP);
  PSBA_HIP(h, hipGetLastError());
  PSBA_HIP(h, hipMemcpyAsync(y_host, q, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  PSBA_HIP(h, hipStreamSynchronize(h->stream));
  return PSBA_OK;
}

// S x = e_a by preconditioned conjugate gradients; dpa into dp[0 .. nA).  The host side of launch_pcg_solve; the
// scalars of a burst are copied behind its last k_fpcg_direction, which is where this route's totals are written.
// GRP (shared intrinsics): the folded diagonal blocks first, the fold behind every block product
template <class T, bool GRP>
static int fpcg_solve(psba_ctx *h) {
  const int n = h->d.nA, nC = h->d.nC, g = fpcg_vec_grid(n), gs = fpcg_row_grid(nC);
  hipStream_t s = h->stream;
  double *x = h->dp, *r0 = h->pcg_vec, *z = r0 + n, *p = z + n, *q = p + n, *r1 = q + n, *pc = h->pcg_scal;
  FgInv fi = {};
  if (GRP) fi = FgInv{kd_groups(h), h->fg_blk, h->bs_D, h->bs_mu, h->coeff};
  ProfScope ps(h, PSBA_K_CHOLESKY);
  PSBA_HIP(h, hipMemsetAsync(pc, 0, sizeof(double) * PF_ALL, s));
  if (GRP) {
    hipLaunchKernelGGL(k_fgrp_partial, dim3((h->kd_nmem + 3) / 4), dim3(256), 0, s, h->bs_val, h->bs_rowptr, h->bs_rowent, fi.G,
                       h->kd_nmem, h->fg_part);
    hipLaunchKernelGGL(k_fgrp_sum, dim3(h->kd_nmg), dim3(256), 0, s, h->bs_val, h->bs_diag, h->fg_part, fi.G, fi.mu, fi.D,
                       h->fg_blk);
  }
  hipLaunchKernelGGL((k_fbsr_diag_inverse<T, GRP>), dim3((nC + FINV_CAMS - 1) / FINV_CAMS), dim3(16 * FINV_CAMS), 0, s,
                     h->bs_val, h->bs_diag, h->pcg_minv, nC, pc, h->status, h->try_id, fi);
  hipLaunchKernelGGL((k_fpcg_start<T, GRP>), dim3(g), dim3(256), 0, s, h->bs_ea, h->pcg_minv, x, r0, z, p, q, n, pc, fi.G);
  double hs[PF_N];
  h->pcg_iters = 0;
  h->pcg_relres = 1.0;
  const double tol2 = h->pcg_tol * h->pcg_tol;
  bool converged = false, failed = false;
  for (int it = 0; it < h->pcg_maxit;) {
    const int burst = it + 8 < h->pcg_maxit ? 8 : h->pcg_maxit - it;
    int last = it;
    for (int k = 0; k < burst; k++, it++) {
      double *rc = (it & 1) ? r1 : r0, *rn = (it & 1) ? r0 : r1;
      hipLaunchKernelGGL(k_fpcg_spmv<T>, dim3(gs), dim3(256), 0, s, h->bs_val, h->bs_rowptr, h->bs_rowent, nC, p, q,
                         pc + PF_PQP + FPCG_CAP * (it & 3));
      if (GRP) fpcg_fold(h, q, p, nullptr, n, pc + PF_PQP + FPCG_CAP * (it & 3));
      hipLaunchKernelGGL(k_fpcg_update<T>, dim3(g), dim3(256), 0, s, x, rc, rn, p, q, h->pcg_minv, z, n, pc, it, GRP ? g : gs,
                         h->status, h->try_id, tol2);
      hipLaunchKernelGGL(k_fpcg_direction<GRP>, dim3(g), dim3(256), 0, s, z, p, n, pc, it, tol2, fi.G);
      last = it;
    }
    PSBA_HIP(h, hipMemcpyAsync(h->pcg_host, pc, sizeof(double) * PF_N, hipMemcpyDeviceToHost, s));
    PSBA_HIP(h, hipGetLastError());
    PSBA_HIP(h, hipStreamSynchronize(s));
    for (int k = 0; k < PF_N; k++) hs[k] = h->pcg_host[k];
    h->pcg_iters = it;
    if (hs[PF_FAIL] != 0.0) {
      failed = true;
      break;
    }
    double rr = hs[PF_RR + (last & 3)];
    if (hs[PF_DONE] != 0.0) {  // the test held inside the burst: the device stopped iterating there
      h->pcg_iters = (int)hs[PF_DONE] - 1;
      rr = hs[PF_RRFIN];
      converged = true;
    } else if (rr <= tol2 * hs[PF_BB]) {  // ... or in its last iteration
      converged = true;
    }
    h->pcg_relres = hs[PF_BB] > 0.0 ? sqrt(rr / hs[PF_BB]) : 0.0;
    if (converged) break;
    if (!(rr - rr == 0.0)) {
      // a non-finite residual (NaN or Inf in S or e_a that the curvature test has not met yet): reported like a
      // failed factorization, never as an exhausted budget
      PSBA_HIP(h, hipMemcpyAsync(h->status + 1, &h->try_id, sizeof(int), hipMemcpyHostToDevice, s));
      PSBA_HIP(h, hipStreamSynchronize(s));
      failed = true;
      break;
    }
  }
  h->pcg_exhausted = !converged && !failed;
  return PSBA_OK;
}

// the block inverses alone, for a caller with scalars and a status word of its own (kernels_free_pcg_many.hip): a bad
// pivot sets pc[PF_FAIL] and status[1] = stamp
template <class T>
static int fbsr_diag_inverse(psba_ctx *h, double *minv, double *pc, int *status, int stamp) {
  const int nC = h->d.nC;
  hipLaunchKernelGGL((k_fbsr_diag_inverse<T, false>), dim3((nC + FINV_CAMS - 1) / FINV_CAMS), dim3(16 * FINV_CAMS), 0,
                     h->stream, h->bs_val, h->bs_diag, minv, nC, pc, status, stamp, FgInv{});
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

#define FPCG_DISPATCH(fn, ...) (h->cnp == KD_CNP ? fn<FreeKD>(__VA_ARGS__) : fn<FreeK>(__VA_ARGS__))
int launch_fbsr_finalize(psba_ctx *h, double mu, const double *D) { return FPCG_DISPATCH(fbsr_finalize, h, mu, D); }
int launch_fbsr_times(psba_ctx *h, const double *x_host, double *y_host) { return FPCG_DISPATCH(fbsr_times, h, x_host, y_host); }
int launch_fpcg_solve(psba_ctx *h) {
  if (h->cnp != KD_CNP) return fpcg_solve<FreeK, false>(h);
  return h->kd_rep ? fpcg_solve<FreeKD, true>(h) : fpcg_solve<FreeKD, false>(h);
}
int launch_fbsr_diag_inverse(psba_ctx *h, double *minv, double *pc, int *status, int stamp) {
  return FPCG_DISPATCH(fbsr_diag_inverse, h, minv, pc, status, stamp);
}

}  // namespace psba
