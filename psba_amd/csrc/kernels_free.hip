// kernels_free.hip -- free intrinsics: one route for both camera blocks, templated on the block.
//   PSBA_CAMERA_FREE_K   11 parameters (fu, u0, v0, ar, s | local rotation | translation), the layout the reference's
//                        driver reads (PSBA/main.cpp:73, 140-149: origin_cnp = 11) before it strips the intrinsics
//   PSBA_CAMERA_FREE_KD  16 parameters (fu, u0, v0, ar, s | k1, k2, k3, k4, k5 | local rotation | translation)
// The reference reads these columns and never optimises them: there is no reference arithmetic to match -- PARITY
// UNPINNED; the judges are the oracle's twin (oracle/psba_oracle.c, orc_fk_*; tests/test_freek.py) and the numpy twin
// tests/freekd_twin.py (central differences, a dense solve of the full normal equations).
//
// The tile is that of v_mfma_f64_16x16x4_f64 (A operand A[l & 15][l >> 4], B operand B[l >> 4][l & 15], C/D
// col = l & 15, row = (l >> 4) + 4 reg):
//   U_j  = sum A^T A   the four Jacobian rows of two observations are the K dimension, one register is A and B
//   g_a  = sum A^T e   the same A operand against a B operand that holds e in column 0
//   S_jk -= Y_a W_b^T  one instruction per product, K = 3 padded to 4
// A block of 16 fills the tile.  A block of 11 runs the same instructions: the lanes with col >= 11 supply 0.0 as their
// operand and rows and columns >= 11 of the accumulator are not stored, so every buffer keeps stride 11 (the guards
// are compile-time constants: the 16 instantiation is the code it was before the template).
// RULE OF THIS ROUTE: no floating-point atomics.  Every sum is formed in an order the upload fixes -- a wave per
// camera unit / per segment of a block's product list, partial results combined in unit / segment order -- so two
// runs give bit-identical reduce buffers and LM logs.
#include "camera_model.h"
#include "free_blocks.h"
#include "psba_internal.h"
#include "schur_common.h"

namespace psba {

// per observation: W (or Y) is CNP x 3 row-major; per unit: the partial A^T A (CNP x CNP) | A^T e (CNP); the LDS row
// of a staged observation is A (2 x CNP) | e | pad (an odd stride: 25 and 35)

// ---- held poses and points (psba_set_held) ----
// A held pose is the six pose coordinates NI .. CNP-1 of a camera (its intrinsics stay under the mask and the groups),
// a held point its three coordinates.  Each held coordinate is what a coordinate held by psba_set_intrinsics_mask is:
// its column of A (B for a point) is zeroed behind T::linearize, before W, Be and the LDS rows are written, so W, the
// sums and g are exactly 0 there and k_free_Y, k_free_schur, the combine, finalize and fold kernels run unchanged on
// the zeros; the stored diagonal entry is the placeholder coeff (k_free_damp_diag clamps it as it stands); the
// maximum of the diagonal skips it; dp is exactly 0 and the proposal takes the current bits.  The cost is untouched.
// The kernels that read the two byte masks are templated on HELD; a handle without a non-zero entry in either mask
// runs the false instantiations, which are the code as it was (no load of a mask).  With HELD both masks are
// allocated ([nC] and [nP]), so no kernel tests a pointer.
struct FreeArgs {
  const double *camconst, *cams, *pts, *impts;
  const int *iidx, *jidx, *ptr, *cam_obs;
  const int4 *cam_units;
  double *W, *Be, *upart;
  double coeff;
  unsigned mask;
  int nO;
  const double *pub_src;  // the look-ahead linearization carries the try's scalar block to the host (see k_linearize)
  double *pub_dst;
  double pub_stamp;
  const unsigned char *held_pose, *held_pt;  // read by the HELD instantiations only (last: the other offsets stay)
  const double *isig;                        // read by the WGT instantiations only (below)
  RobustLoss rl;
  const unsigned short *cmask;               // per-camera masks, null: none (kd_free_bits)
};

// ---- observation weighting (psba_set_obs_weighting) ----
// Observation a may carry a standard deviation sigma_a > 0 (without sigmas sigma_a = 1), and a loss (kind, c) may be
// set, with the kinds, formulas and conventions of DESIGN 7b (PSBA_LOSS_*, robust_eval in camera_model.h).  With e_a
// the route's residual:
//   s_a = |e_a / sigma_a|^2        F = sum_a rho(s_a) + the priors' two sums (the priors are not weighted)
// IRLS without the rho'' term: omega_a = sqrt(rho'(s_a)).  The kernel first multiplies e, both rows of A, and B by
// 1 / sigma_a (the reciprocal is stored once at the setter) and then by omega_a -- the order of whiten_obs followed by
// robust_scale on the fixed route: two roundings per entry.  Everything behind the per-observation blocks reads the
// weighted blocks and is otherwise unchanged: W, Be, U, g_a, V, g_b, D of Marquardt, Y, S, e_a, the fold of the
// groups, the back-substitution and gain_den.  A zeroed column stays zero under the scaling, so every exact guarantee
// of the mask, the groups, the damping, the holds and the priors keeps holding.  psba_residual, psba_begin, the try's
// new cost and the costs of psba_levmar are all F; psba_get_free_obs_blocks returns the weighted W and B | e.
// The kernels that see observations are templated on WGT; a handle without a weighting runs the false instantiations,
// which are the code as it was (no load of the table, no loss argument read).  With WGT the table 1 / sigma [nO] is
// always allocated (ones when only a loss is set), so no kernel tests a pointer.  The weights are per observation:
// no sum is new, and every reduction keeps the order the upload fixes.
// e <- e / sigma_a; s_a, rho(s_a) and omega_a of the scaled e
__device__ __forceinline__ void free_weight(const RobustLoss &rl, double is, double &e0, double &e1, double &s, double &rho,
                                            double &om) {
  PSBA_FP_PINNED;
  e0 *= is;
  e1 *= is;
  s = e0 * e0 + e1 * e1;
  robust_eval(rl, s, rho, om);
}

// ---- Gaussian priors on cameras and points (psba_set_priors) ----
// A camera j may carry a mean m_j [CNP] (the order of the camera block) and a symmetric positive semi-definite
// information matrix L_j [CNP x CNP]; a point i n_i [3] and G_i [3 x 3].  With d = m - p (the sign of e = measured -
// projected) the cost is F = sum |e_a|^2 + sum_j d_j^T L_j d_j + sum_i d_i^T G_i d_i: the priors are extra residual
// rows, so psba_residual, psba_begin, the try's new cost and psba_levmar all see F.  With s the sums of the kernels:
//   U_j[r][c] = coeff (s_rc + L_j[r][c])            g_a,j[r] = coeff_g (s_r + sum_c L_j[r][c] d_j[c])
// the inner sum from zero in ascending c, one add into s; d at the parameter set being linearized (current, or the
// proposal for the look-ahead set).  Points the same with G_i on the six stored entries of V_i and on g_b,i.  A held
// coordinate (mask, psba_set_held) has its column deleted from the prior rows too: row and column of L (G) are not
// added to U (V), g stays exactly 0 there, and the gradient of a free coordinate still takes the whole d, the held
// deviations included.  A coordinate folded away by the groups is not held here: U carries L and the fold sums the
// members' rows and columns, so a shared intrinsic gets the sum of its members' priors.  The cost counts the whole
// quadratic form, q = sum_r d_r (sum_c L[r][c] d[c]), r and c ascending.  Everything behind U, V and g (the maximum of
// the diagonal, Marquardt's D, Y, S, e_a, the back-substitution, gain_den) reads the stored values and is unchanged.
// Storage is compacted: an index per block (-1: no prior) into records mean | information of the blocks that have
// one, and the list of those blocks for the cost kernels.  The kernels that read them are templated on PRIOR; a
// handle on which no block has a prior runs the false instantiations, which are the code as it was.  With PRIOR all
// tables are allocated, so no kernel tests a pointer.
struct FreePriors {
  const int *cidx, *pidx;      // [nC], [nP] record of the block, -1: none
  const double *crec, *prec;   // [n][CNP + CNP^2], [n][12]
};
template <int N>
__device__ __forceinline__ double prior_row(const double *rec, const double *x, int r) {  // sum_c L[r][c] (m[c] - x[c])
  double t = 0.0;
#pragma unroll
  for (int c = 0; c < N; c++) t += rec[N + N * r + c] * (rec[c] - x[c]);
  return t;
}
template <int N>
__device__ __forceinline__ double prior_quad(const double *rec, const double *x) {  // d^T L d, rows ascending
  double q = 0.0;
#pragma unroll
  for (int r = 0; r < N; r++) q += (rec[r] - x[r]) * prior_row<N>(rec, x, r);
  return q;
}

template <class T>
__device__ __forceinline__ void free_load(const FreeArgs &p, int a, int &i, int &j, double *cam, double *q0, double *M,
                                          double2 &m) {
  i = p.iidx[a];
  j = p.jidx[a];
#pragma unroll
  for (int k = 0; k < T::CNP; k++) cam[k] = p.cams[T::CNP * (size_t)j + k];
#pragma unroll
  for (int k = 0; k < 4; k++) q0[k] = p.camconst[9 * (size_t)j + 5 + k];
#pragma unroll
  for (int k = 0; k < 3; k++) M[k] = p.pts[3 * (size_t)i + k];
  m = reinterpret_cast<const double2 *>(p.impts)[a];
}

// sums of one value over the wave and over the workgroup's waves, in a fixed order (a shuffle tree, then wave 0 .. n)
__device__ __forceinline__ double free_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// camera-major: one wave per unit = up to 64 observations of one camera, one per lane.  e, A (masked), B; W_a and
// (B | e) to global memory, the Jacobian rows to LDS, then U and g_a of the unit by MFMA
template <class T, bool HELD, bool WGT>
__global__ __launch_bounds__(64) void k_free_linearize(FreeArgs p) {
  constexpr int CNP = T::CNP, ROW = 2 * CNP + 3;
  __shared__ double sJ[KD_UNIT][ROW];
  const int lane = threadIdx.x;
  if (p.pub_dst && blockIdx.x == 0) scal_publish(p.pub_src, p.pub_dst, p.pub_stamp);
  const int4 u = p.cam_units[blockIdx.x];
  const int n = u.z - u.y;
  const unsigned mask = kd_free_bits(p.mask, p.cmask, u.x);  // (the unit's camera: one load per wave, none without a table)
  if (lane < n) {
    const int a = p.cam_obs[u.y + lane];
    int i, j;
    double cam[CNP], q0[4], M[3], e[2], A[2 * CNP], B[6];
    double2 m;
    free_load<T>(p, a, i, j, cam, q0, M, m);
    T::linearize(cam, q0, M, m.x, m.y, e, A, B, mask);
    if (WGT) {  // e, A, B by 1 / sigma_a, then by omega_a of the scaled e (before anything is stored)
      const double is = p.isig[a];
      double s, rho, om;
      free_weight(p.rl, is, e[0], e[1], s, rho, om);
      e[0] *= om;
      e[1] *= om;
#pragma unroll
      for (int k = 0; k < 2 * CNP; k++) A[k] = (A[k] * is) * om;
#pragma unroll
      for (int k = 0; k < 6; k++) B[k] = (B[k] * is) * om;
    }
    if (HELD) {  // (selects on registers, before anything is stored)
      const bool hp = p.held_pose[j] != 0, hq = p.held_pt[i] != 0;
#pragma unroll
      for (int k = T::NI; k < CNP; k++) {
        A[k] = hp ? 0.0 : A[k];
        A[CNP + k] = hp ? 0.0 : A[CNP + k];
      }
#pragma unroll
      for (int k = 0; k < 6; k++) B[k] = hq ? 0.0 : B[k];
    }
    double *w = p.W + 3 * CNP * (size_t)a;
#pragma unroll
    for (int r = 0; r < CNP; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) w[3 * r + c] = p.coeff * (A[r] * B[c] + A[CNP + r] * B[3 + c]);
    double *be = p.Be + 8 * (size_t)a;
#pragma unroll
    for (int k = 0; k < 6; k++) be[k] = B[k];
    be[6] = e[0];
    be[7] = e[1];
#pragma unroll
    for (int k = 0; k < 2 * CNP; k++) sJ[lane][k] = A[k];
    sJ[lane][2 * CNP] = e[0];
    sJ[lane][2 * CNP + 1] = e[1];
  } else {
#pragma unroll
    for (int k = 0; k < 2 * CNP + 2; k++) sJ[lane][k] = 0.0;
  }
  __syncthreads();
  const int col = lane & 15, k = lane >> 4;  // k: row 0 / 1 of the even observation, row 0 / 1 of the odd one
  const bool live = CNP == 16 || col < CNP;  // (a lane outside the block: operand 0.0, nothing stored; its index
                                             // is clamped as well, the load may be issued ahead of the select)
  kd4 accU = {0.0, 0.0, 0.0, 0.0}, accG = {0.0, 0.0, 0.0, 0.0};
  const int steps = (n + 1) >> 1;
  for (int t = 0; t < steps; t++) {
    const double *row = sJ[2 * t + (k >> 1)];
    const double v = live ? row[(k & 1) * CNP + (live ? col : 0)] : 0.0;
    const double ev = col == 0 ? row[2 * CNP + (k & 1)] : 0.0;
    accU = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, accU, 0, 0, 0);
    accG = __builtin_amdgcn_mfma_f64_16x16x4f64(v, ev, accG, 0, 0, 0);
  }
  double *up = p.upart + (CNP * CNP + CNP) * (size_t)blockIdx.x;
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (live && (CNP == 16 || k + 4 * r < CNP)) up[CNP * (k + 4 * r) + col] = accU[r];
  if (col == 0) {
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (CNP == 16 || k + 4 * r < CNP) up[CNP * CNP + k + 4 * r] = accG[r];
  }
}

// the units of one camera in unit order: U_j (full CNP x CNP, scaled by coeff, the placeholder coeff on the diagonal
// of a masked intrinsic and of a held pose coordinate) and g_a,j (scaled by coeff_g).  A camera without observations
// has zero sums
template <class T, bool HELD, bool PRIOR>
__global__ __launch_bounds__(256) void k_free_finish_cams(const double *upart, const int *cuptr, int nC, double coeff,
                                                          double coeff_g, unsigned mask0, const unsigned short *cmask,
                                                          const unsigned char *held_pose, double *U, double *ga, FreePriors pr,
                                                          const double *cams) {
  constexpr int CNP = T::CNP, UP = CNP * CNP + CNP;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)nC * UP) return;
  const int j = (int)(t / UP), e = (int)(t % UP);
  const unsigned mask = kd_free_bits(mask0, cmask, j);
  double s = 0.0;
  for (int u = cuptr[j]; u < cuptr[j + 1]; u++) s += upart[UP * (size_t)u + e];
  if (PRIOR) {  // (a held row or column of the information matrix is dropped; the gradient takes the whole d)
    const int k = pr.cidx[j];
    if (k >= 0) {
      const double *rec = pr.crec + (size_t)(CNP + CNP * CNP) * k;
      const bool hp = HELD && held_pose[j];
      const int r = e < CNP * CNP ? e / CNP : e - CNP * CNP, c = e < CNP * CNP ? e % CNP : r;
      const bool hr = r < T::NI ? !((mask >> r) & 1u) : hp, hc = c < T::NI ? !((mask >> c) & 1u) : hp;
      if (!hr && !hc) s += e < CNP * CNP ? rec[CNP + e] : prior_row<CNP>(rec, cams + (size_t)CNP * j, r);
    }
  }
  if (e < CNP * CNP) {
    const int r = e / CNP, c = e % CNP;
    bool held = r == c && r < T::NI && !((mask >> r) & 1u);
    if (HELD) held = held || (r == c && r >= T::NI && held_pose[j]);
    U[(size_t)CNP * CNP * j + e] = held ? coeff : coeff * s;
  } else {
    ga[(size_t)CNP * j + (e - CNP * CNP)] = coeff_g * s;
  }
}

// V_i and g_b,i: thread per point over its contiguous observations, in observation order.  A held point: its B is
// zero, so the sums are; the diagonal takes the placeholder (V_i = coeff I, g_b,i = 0)
template <bool HELD, bool PRIOR>
__global__ __launch_bounds__(256) void k_free_point_sums(const double *Be, const int *ptr, int nP, double coeff,
                                                         double coeff_g, const unsigned char *held_pt, double *PV,
                                                         FreePriors pr, const double *pts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nP) return;
  double v[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
  for (int a = ptr[i]; a < ptr[i + 1]; a++) {
    const double *be = Be + 8 * (size_t)a;
    double B[6];
#pragma unroll
    for (int k = 0; k < 6; k++) B[k] = be[k];
    const double e0 = be[6], e1 = be[7];
    int q = 0;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = r; c < 3; c++) v[q++] += B[r] * B[c] + B[3 + r] * B[3 + c];
#pragma unroll
    for (int r = 0; r < 3; r++) g[r] += B[r] * e0 + B[3 + r] * e1;
  }
  if (PRIOR) {  // (a held point: the placeholder below overwrites the sums)
    const int k = pr.pidx[i];
    if (k >= 0) {
      const double *rec = pr.prec + 12 * (size_t)k;
      int q = 0;
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = r; c < 3; c++) v[q++] += rec[3 + 3 * r + c];
#pragma unroll
      for (int r = 0; r < 3; r++) g[r] += prior_row<3>(rec, pts + 3 * (size_t)i, r);
    }
  }
  double *pv = PV + 9 * (size_t)i;
#pragma unroll
  for (int k = 0; k < 6; k++) pv[k] = coeff * v[k];
#pragma unroll
  for (int k = 0; k < 3; k++) pv[6 + k] = coeff_g * g[k];
  if (HELD && held_pt[i]) {
    pv[0] = pv[3] = pv[5] = coeff;
    pv[1] = pv[2] = pv[4] = 0.0;
    pv[6] = pv[7] = pv[8] = 0.0;
  }
}

// cost: per-workgroup partial sums; k_free_sum_columns adds them in workgroup order
template <class T, bool WGT>
__global__ __launch_bounds__(256) void k_free_residual(FreeArgs p, double *part) {
  __shared__ double sRed[4];
  double sum = 0.0;
  for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < p.nO; a += gridDim.x * blockDim.x) {
    int i, j;
    double cam[T::CNP], q0[4], M[3], e0, e1;
    double2 m;
    free_load<T>(p, a, i, j, cam, q0, M, m);
    T::residual(cam, q0, M, m.x, m.y, e0, e1);
    if (WGT) {  // rho(|e / sigma_a|^2)
      double s, rho, om;
      free_weight(p.rl, p.isig[a], e0, e1, s, rho, om);
      sum += rho;
    } else {
      sum += e0 * e0 + e1 * e1;
    }
  }
  sum = free_wave_sum(sum);
  if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

// psba_get_obs_weights: one thread per observation, s_a and w_a = omega_a / sigma_a (the factor the blocks are
// multiplied by) at the parameter set of p, from the residual alone.  On a handle without a weighting isig is null
// (s = |e|^2, w = 1): the only kernel of the file that tests the pointer, and no solver path runs it
template <class T>
__global__ __launch_bounds__(256) void k_free_obs_weights(FreeArgs p, double *s_out, double *w_out) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= p.nO) return;
  int i, j;
  double cam[T::CNP], q0[4], M[3], e0, e1;
  double2 m;
  free_load<T>(p, a, i, j, cam, q0, M, m);
  T::residual(cam, q0, M, m.x, m.y, e0, e1);
  const double is = p.isig ? p.isig[a] : 1.0;
  double s, rho, om;
  free_weight(p.rl, is, e0, e1, s, rho, om);
  s_out[a] = s;
  w_out[a] = om * is;
}

// dst[q] = head[q] + sum over rows r < n of part[ncol r + q], in row order (q < ncol <= 4; head may be null)
__global__ __launch_bounds__(64) void k_free_sum_columns(const double *head, const double *part, int n, int ncol, double *dst) {
  const int q = threadIdx.x;
  if (q >= ncol) return;
  double v = head ? head[q] : 0.0;
  for (int r = 0; r < n; r++) v += part[(size_t)ncol * r + q];
  dst[q] = v;
}

// the prior part of the cost: thread per block that has a prior (list [n], its record rec[idx[list]], its parameters
// x[N list]), d^T L d per block, per-workgroup partial sums as k_free_residual's (k_free_sum_columns adds them in
// workgroup order, behind the observations' partials)
template <int N>
__global__ __launch_bounds__(256) void k_free_prior_cost(const int *list, const int *idx, const double *rec, const double *x,
                                                         int n, double *part) {
  __shared__ double sRed[4];
  double sum = 0.0;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const int b = list[t];
    sum += prior_quad<N>(rec + (size_t)(N + N * N) * idx[b], x + (size_t)N * b);
  }
  sum = free_wave_sum(sum);
  if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

// the largest diagonal entry of U and V over the free parameters (a maximum does not depend on the order)
template <class T, bool HELD>
__global__ __launch_bounds__(1024) void k_free_max_diag(const double *U, const double *PV, int nC, int nP, unsigned mask,
                                                        const unsigned short *cmask, const unsigned char *held_pose,
                                                        const unsigned char *held_pt, double *out) {
  constexpr int CNP = T::CNP;
  __shared__ double sRed[16];
  double m = 0.0;
  for (int t = threadIdx.x; t < CNP * nC; t += blockDim.x) {
    const int r = t % CNP;
    if (HELD && r >= T::NI && held_pose[t / CNP]) continue;
    if (r >= T::NI || ((kd_free_bits(mask, cmask, t / CNP) >> r) & 1u)) m = fmax(m, U[(size_t)CNP * CNP * (t / CNP) + (CNP + 1) * r]);
  }
  for (int i = threadIdx.x; i < nP; i += blockDim.x) {
    if (HELD && held_pt[i]) continue;
    const double *v = PV + 9 * (size_t)i;
    m = fmax(m, fmax(v[0], fmax(v[3], v[5])));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
  if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; w++) m = fmax(m, sRed[w]);
    *out = m;
  }
}

// the damping rule of a try (psba_set_damping).  D null: N + mu I, and the kernels below are what they were
// -- the branch on D is uniform and its side loads nothing.  D set: N + mu D, D [nT] written by k_free_damp_diag for
// the linearization the try reads; the point kernels form their three entries from PV in registers (damp_point_block)
struct FreeDamp {
  const double *D;
  double dmin, dmax;
};

// one thread per parameter, behind k_free_finish_cams and k_free_point_sums: D_k = clamp(N_kk) of this linearization.
// Cameras: U_j[k][k] (a held coordinate: its placeholder coeff).  With groups a shared coordinate of a representative
// takes the sum over its members in ascending camera order (the folded diagonal of k_kd_max_diag_groups), a
// folded-away one coeff, as a masked coordinate.  Points: the diagonal of V_i
template <class T>
__global__ __launch_bounds__(256) void k_free_damp_diag(const double *U, const double *PV, const int *rep, const int *gidx,
                                                        const int *gptr, const int *gmem, unsigned mask,
                                                        const unsigned short *cmask, double coeff, int nA, int nT, double dmin,
                                                        double dmax, double *D) {
  constexpr int CNP = T::CNP;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nT) return;
  double n;
  if (t < nA) {
    const int j = t / CNP, r = t % CNP;
    n = U[(size_t)CNP * CNP * j + (CNP + 1) * r];
    const int g = (rep && r < 10 && ((kd_free_bits(mask, cmask, j) >> r) & 1u)) ? gidx[j] : -1;
    if (g >= 0 && rep[j] == j) {
      n = 0.0;
      for (int q = gptr[g]; q < gptr[g + 1]; q++) n += U[(size_t)CNP * CNP * gmem[q] + (CNP + 1) * r];
    } else if (g >= 0) {
      n = coeff;
    }
  } else {
    const int i = (t - nA) / 3, q = (t - nA) % 3;
    n = PV[9 * (size_t)i + (q == 0 ? 0 : q == 1 ? 3 : 5)];
  }
  D[t] = damp_diag(n, dmin, dmax);
}

// per try, camera-major (one wave per unit): Y_a = W_a (V_i + mu I)^-1 stored once, and the unit's part of
// sum_a Y_a g_b,i (the e_a term of camera j), reduced over the lanes by a shuffle tree.  Y by L D L^T and
// substitution: the closed-form inverse loses the points seen once at a small mu
template <class T>
__global__ __launch_bounds__(64) void k_free_Y(const double *W, const double *PV, const int *iidx, const int *cam_obs,
                                               const int4 *cam_units, double *Y, double *eapart, double mu, FreeDamp dm,
                                               int *status, int try_id) {
  constexpr int CNP = T::CNP;
  const int lane = threadIdx.x;
  const int4 u = cam_units[blockIdx.x];
  double t[CNP];
#pragma unroll
  for (int r = 0; r < CNP; r++) t[r] = 0.0;
  if (lane < u.z - u.y) {
    const int a = cam_obs[u.y + lane];
    const double *pv = PV + 9 * (size_t)iidx[a];
    double v[6], vi[6];
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = pv[k];
    if (dm.D) {
      damp_point_block(v, mu, dm.dmin, dm.dmax);
    } else {
      v[0] += mu;
      v[3] += mu;
      v[5] += mu;
    }
    if (sym3_inverse(v, vi)) status[0] = try_id;  // (the singular flag as on the other routes; Y by substitution)
    const Sym3Ldl f = sym3_ldl(v);
    const double g0 = pv[6], g1 = pv[7], g2 = pv[8];
    const double *w = W + 3 * CNP * (size_t)a;
    double *y = Y + 3 * CNP * (size_t)a;
#pragma unroll
    for (int r = 0; r < CNP; r++) {
      double y0, y1, y2;
      sym3_ldl_solve(f, w[3 * r], w[3 * r + 1], w[3 * r + 2], y0, y1, y2);
      y[3 * r] = y0;
      y[3 * r + 1] = y1;
      y[3 * r + 2] = y2;
      t[r] = y0 * g0 + y1 * g1 + y2 * g2;
    }
  }
#pragma unroll
  for (int r = 0; r < CNP; r++) {
    const double s = free_wave_sum(t[r]);
    if (lane == 0) eapart[CNP * (size_t)blockIdx.x + r] = s;
  }
}

// S assembly: one wave per segment of a block's product list, one MFMA per product (A = Y_a, B = W_b^T, K = 3 of 4).
// The only segment of a block stores -sum straight into S; the others store partial tiles (CNP x CNP each).
// LIST (PSBA_SOLVER_SPARSE): S is the list of stored blocks, blocks[b].x the slot of the plan's block b, and the
// destination is S + CNP^2 slot with row stride CNP; the dense instantiation is the code as it was
template <class T, bool LIST = false>
__global__ __launch_bounds__(256) void k_free_schur(const double *Y, const double *W, const int2 *prods, const int4 *segs,
                                                    const int2 *blocks, int nsegs, double *S, int ld, double *tiles) {
  constexpr int CNP = T::CNP, WB = 3 * CNP;
  const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nsegs) return;
  const int lane = threadIdx.x & 63, col = lane & 15, k = lane >> 4;
  const bool live = CNP == 16 || col < CNP;  // (a lane outside the block reads entry 0 of the record and supplies 0.0)
  const bool zero = k == 3 || !live;
  const int4 s = segs[seg];
  const int off = live ? 3 * col + (k < 3 ? k : 0) : 0;
  kd4 acc = {0.0, 0.0, 0.0, 0.0};
  int p = s.y;
  for (; p + 4 <= s.z; p += 4) {  // four products' loads in flight before the first MFMA
    double y[4], w[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int2 ab = prods[p + q];
      y[q] = Y[WB * (size_t)ab.x + off];
      w[q] = W[WB * (size_t)ab.y + off];
      if (zero) y[q] = w[q] = 0.0;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(y[q], w[q], acc, 0, 0, 0);
  }
  for (; p < s.z; p++) {
    const int2 ab = prods[p];
    double y = Y[WB * (size_t)ab.x + off], w = W[WB * (size_t)ab.y + off];
    if (zero) y = w = 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(y, w, acc, 0, 0, 0);
  }
  if (s.w < 0) {
    const int2 b = blocks[s.x];
    double *dst = LIST ? S + (size_t)(CNP * CNP) * b.x : S + (size_t)(CNP * b.x) * ld + CNP * b.y;
    const size_t rs = LIST ? (size_t)CNP : (size_t)ld;
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (live && (CNP == 16 || k + 4 * r < CNP)) dst[(size_t)(k + 4 * r) * rs + col] = -acc[r];
  } else {
    double *dst = tiles + CNP * CNP * (size_t)s.w;
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (live && (CNP == 16 || k + 4 * r < CNP)) dst[CNP * (k + 4 * r) + col] = acc[r];
  }
}

// the blocks with several segments: their partial tiles in segment order (LIST: multi[].x is the block's slot)
template <class T, bool LIST = false>
__global__ __launch_bounds__(256) void k_free_combine(const int4 *multi, const double *tiles, double *S, int ld) {
  constexpr int CNP = T::CNP;
  const int4 m = multi[blockIdx.x];
  const int e = threadIdx.x;
  if (CNP < 16 && e >= CNP * CNP) return;
  double s = 0.0;
  for (int t = 0; t < m.w; t++) s += tiles[CNP * CNP * (size_t)(m.z + t) + e];
  if (LIST)
    S[(size_t)(CNP * CNP) * m.x + e] = -s;
  else
    S[(size_t)(CNP * m.x + e / CNP) * ld + CNP * m.y + e % CNP] = -s;
}

// S += blockdiag(U) + mu I (mu D with D set) on the lower block triangle, mirrored to the upper; e_a = g_a - the
// units' sums in unit order; identity padding; the accumulators of the try's back-substitution zeroed, the try stamp set
template <class T>
__global__ __launch_bounds__(256) void k_free_finalize(double *S, double *ea, const double *U, const double *ga,
                                                       const double *eapart, const int *cuptr, double mu, const double *D,
                                                       int nA, int n32, double *scal, int *status, int try_id) {
  constexpr int CNP = T::CNP;
  if (blockIdx.x == 0 && threadIdx.x < 4 * SC_NPART) scal[SC_PART + threadIdx.x] = 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 64) status[3] = try_id;
  const size_t n2 = (size_t)nA * nA;
  const size_t gtid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gsize = (size_t)gridDim.x * blockDim.x;
  for (size_t t = gtid; t < n2; t += gsize) {
    const int r = (int)(t / nA), c = (int)(t % nA);
    const int kb = r / CNP, lb = c / CNP;
    const size_t at = (size_t)r * n32 + c;
    if (lb > kb) {
      S[at] = S[(size_t)c * n32 + r];
    } else if (lb == kb) {
      double v = S[at] + U[(size_t)CNP * CNP * kb + CNP * (r - CNP * kb) + (c - CNP * lb)];
      if (r == c) v += D ? mu * D[r] : mu;
      S[at] = v;
    }
  }
  for (size_t t = gtid; t < (size_t)nA; t += gsize) {
    const int j = (int)(t / CNP), r = (int)(t % CNP);
    double s = 0.0;
    for (int u = cuptr[j]; u < cuptr[j + 1]; u++) s += eapart[CNP * (size_t)u + r];
    ea[t] = ga[t] - s;
  }
  write_padding(S, nA, n32, 1.0, gtid, gsize);
}

// back-substitution, thread per point: e_b,i = g_b,i - sum_j W_ij^T dpa_j, V*_i dpb_i = e_b,i (L D L^T), proposed
// point, then the residuals of its observations at the proposal; the try's four sums as per-workgroup partials in
// red (row 0: the camera terms), added in workgroup order by k_free_sum_columns
struct FreeBackArgs {
  const double *W, *PV, *camconst, *cams, *pts, *impts, *ga;
  const int *jidx, *ptr;
  double *dp, *newcams, *newpts, *scal, *red;
  const int *status;
  double mu;
  FreeDamp dm;
  unsigned mask;
  int nA, nP;
  const unsigned char *held_pose, *held_pt;  // read by the HELD instantiations only
  FreePriors pr;                             // read by the PRIOR instantiations only
  const double *isig;                        // read by the WGT instantiations only
  RobustLoss rl;
  const unsigned short *cmask;               // per-camera masks, null: none (kd_free_bits)
};
// the camera priors' cost at the proposal, from the newcams this workgroup has just written (behind a barrier): the
// try's `new cost` slot, thread per coordinate r: d_r (sum_c L[r][c] d[c])
template <int CNP>
__device__ __forceinline__ double free_prior_newcost(const FreeBackArgs &p) {
  __threadfence_block();
  __syncthreads();
  double v = 0.0;
  for (int t = threadIdx.x; t < p.nA; t += blockDim.x) {
    const int j = t / CNP, r = t % CNP, k = p.pr.cidx[j];
    if (k < 0) continue;
    const double *rec = p.pr.crec + (size_t)(CNP + CNP * CNP) * k;
    v += (rec[r] - p.newcams[t]) * prior_row<CNP>(rec, p.newcams + (size_t)CNP * j, r);
  }
  return v;
}
__device__ __forceinline__ void free_block_sums4(double *v4, double (*sRed)[4], double *dst) {
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const double v = free_wave_sum(v4[q]);
    if ((threadIdx.x & 63) == 0) sRed[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) dst[threadIdx.x] = ((sRed[threadIdx.x][0] + sRed[threadIdx.x][1]) + sRed[threadIdx.x][2]) + sRed[threadIdx.x][3];
}
template <class T, bool HELD, bool PRIOR>
__global__ __launch_bounds__(256) void k_free_backsub_cams(FreeBackArgs p) {  // one workgroup, launched first: proposal cams
  __shared__ double sRed[4][4];
  double v4[4] = {0.0, 0.0, 0.0, 0.0};  // dp_l2, gain_den, (new cost: the point kernel's), newp_l2
  if (threadIdx.x == 0) {
    p.scal[SC_STATUS_V] = (p.status[0] == p.status[3]) ? 1.0 : 0.0;
    p.scal[SC_STATUS_SPD] = (p.status[1] == p.status[3]) ? 1.0 : 0.0;
  }
  for (int t = threadIdx.x; t < p.nA; t += blockDim.x) {
    const int r = t % T::CNP;
    const bool hp = HELD && r >= T::NI && p.held_pose[t / T::CNP];
    const bool held = hp || (r < T::NI && !((kd_free_bits(p.mask, p.cmask, t / T::CNP) >> r) & 1u));
    double d = p.dp[t];
    if (held) p.dp[t] = d = 0.0;  // (already zero to rounding: S decouples the entry; exactly zero by definition)
    const double c = hp ? p.cams[t] : p.cams[t] + d;  // (a held pose keeps its bits: -0.0 + 0.0 would be +0.0)
    p.newcams[t] = c;
    v4[0] += d * d;
    const double mud = p.dm.D ? p.mu * p.dm.D[t] : p.mu;
    v4[1] += d * (mud * d + p.ga[t]);
    v4[3] += c * c;
  }
  if (PRIOR) v4[2] = free_prior_newcost<T::CNP>(p);
  free_block_sums4(v4, sRed, p.red);
}
template <class T, bool HELD, bool PRIOR, bool WGT>
__global__ __launch_bounds__(256) void k_free_backsub_pts(FreeBackArgs p) {
  constexpr int CNP = T::CNP;
  __shared__ double sRed[4][4];
  double v4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.nP; i += gridDim.x * blockDim.x) {
    const double *pv = p.PV + 9 * (size_t)i;
    const int o0 = p.ptr[i], o1 = p.ptr[i + 1];
    double e0 = pv[6], e1 = pv[7], e2 = pv[8];
    for (int a = o0; a < o1; a++) {
      const double *w = p.W + 3 * CNP * (size_t)a;
      const double *da = p.dp + CNP * (size_t)p.jidx[a];
#pragma unroll
      for (int k = 0; k < CNP; k++) {
        e0 -= w[3 * k] * da[k];
        e1 -= w[3 * k + 1] * da[k];
        e2 -= w[3 * k + 2] * da[k];
      }
    }
    double v[6], d[3];
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = pv[k];
    double mud[3] = {p.mu, p.mu, p.mu};
    if (p.dm.D) {
      mud[0] = p.mu * damp_diag(v[0], p.dm.dmin, p.dm.dmax);
      mud[1] = p.mu * damp_diag(v[3], p.dm.dmin, p.dm.dmax);
      mud[2] = p.mu * damp_diag(v[5], p.dm.dmin, p.dm.dmax);
      damp_point_block(v, p.mu, p.dm.dmin, p.dm.dmax);
    } else {
      v[0] += p.mu;
      v[3] += p.mu;
      v[5] += p.mu;
    }
    sym3_ldl_solve(sym3_ldl(v), e0, e1, e2, d[0], d[1], d[2]);
    const bool hq = HELD && p.held_pt[i];  // a held point: dp exactly 0, the proposal takes the current bits
    double n3[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const double cur = p.pts[3 * (size_t)i + q];
      if (hq) d[q] = 0.0;
      n3[q] = hq ? cur : cur + d[q];
      p.dp[p.nA + 3 * (size_t)i + q] = d[q];
      p.newpts[3 * (size_t)i + q] = n3[q];
      v4[0] += d[q] * d[q];
      v4[1] += d[q] * (mud[q] * d[q] + pv[6 + q]);
      v4[3] += n3[q] * n3[q];
    }
    for (int a = o0; a < o1; a++) {  // (newcams: written by k_free_backsub_cams, launched before this kernel)
      const int j = p.jidx[a];
      double cam[CNP], q0[4], r0, r1;
#pragma unroll
      for (int k = 0; k < CNP; k++) cam[k] = p.newcams[CNP * (size_t)j + k];
#pragma unroll
      for (int k = 0; k < 4; k++) q0[k] = p.camconst[9 * (size_t)j + 5 + k];
      const double2 m = reinterpret_cast<const double2 *>(p.impts)[a];
      T::residual(cam, q0, n3, m.x, m.y, r0, r1);
      if (WGT) {  // rho(|e / sigma_a|^2) at the proposal
        double s, rho, om;
        free_weight(p.rl, p.isig[a], r0, r1, s, rho, om);
        v4[2] += rho;
      } else {
        v4[2] += r0 * r0 + r1 * r1;
      }
    }
    if (PRIOR) {  // the point's prior at its proposal, behind its observations
      const int k = p.pr.pidx[i];
      if (k >= 0) v4[2] += prior_quad<3>(p.pr.prec + 12 * (size_t)k, n3);
    }
  }
  free_block_sums4(v4, sRed, p.red + 4 * (size_t)(1 + blockIdx.x));
}

// ---- intrinsics shared between cameras (psba_set_intrinsics_groups) ----
// A free intrinsic coordinate k < 10 of a camera that is not the representative (lowest member) of its group is
// "folded away": its row and column are added to the representative's and it is left as a masked coordinate is.
// The kernels below are for blocks of 16 only and run only on a handle with groups; every sum goes over the members in ascending camera order.
// k_free_finalize without the damping and with the whole square symmetric entry by entry (the diagonal blocks of
// -sum Y_a W_a^T are symmetric only to rounding: their lower triangle is the matrix), so that the fold may read any
// entry: S = blockdiag(U) - sum Y W^T, e_a, identity padding, the accumulators zeroed, the try stamp set
__global__ __launch_bounds__(256) void k_kd_finalize_sym(double *S, double *ea, const double *U, const double *ga,
                                                         const double *eapart, const int *cuptr, int nA, int n32,
                                                         double *scal, int *status, int try_id) {
  if (blockIdx.x == 0 && threadIdx.x < 4 * SC_NPART) scal[SC_PART + threadIdx.x] = 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 64) status[3] = try_id;
  const size_t n2 = (size_t)nA * nA;
  const size_t gtid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gsize = (size_t)gridDim.x * blockDim.x;
  for (size_t t = gtid; t < n2; t += gsize) {
    const int r = (int)(t / nA), c = (int)(t % nA);
    const int kb = r / KD_CNP, lb = c / KD_CNP;
    const size_t at = (size_t)r * n32 + c;
    if (lb > kb) {
      S[at] = S[(size_t)c * n32 + r];
    } else if (lb == kb && r >= c) {  // (the entries above the diagonal of a diagonal block: written from below)
      const double v = S[at] + U[(size_t)KD_CNP * KD_CNP * kb + KD_CNP * (r - KD_CNP * kb) + (c - KD_CNP * lb)];
      S[at] = v;
      if (r > c) S[(size_t)c * n32 + r] = v;
    }
  }
  for (size_t t = gtid; t < (size_t)nA; t += gsize) {
    const int j = (int)(t / KD_CNP), r = (int)(t % KD_CNP);
    double s = 0.0;
    for (int u = cuptr[j]; u < cuptr[j + 1]; u++) s += eapart[KD_CNP * (size_t)u + r];
    ea[t] = ga[t] - s;
  }
  write_padding(S, nA, n32, 1.0, gtid, gsize);
}

// row pass: thread = (group, intrinsic k, column c) owns S[(m, k)][c] of every member m; the representative's row
// becomes the sum of the members' rows (the other rows are left for k_kd_fold_finish to clear)
__global__ __launch_bounds__(256) void k_kd_fold_rows(double *S, KdGroups G, int nA, int n32) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)G.nmg * 10 * nA) return;
  const int c = (int)(t % nA), gk = (int)(t / nA);
  const int g = gk / 10, k = gk % 10;
  const int m0 = G.gptr[g], m1 = G.gptr[g + 1];
  if (!((kd_free_bits(G.mask, G.cmask, G.gmem[m0]) >> k) & 1u)) return;  // (the members carry equal rows)
  double s = 0.0;
  for (int q = m0; q < m1; q++) s += S[(size_t)(KD_CNP * G.gmem[q] + k) * n32 + c];
  S[(size_t)(KD_CNP * G.gmem[m0] + k) * n32 + c] = s;
}

// column pass, a launch of its own behind the row pass: thread = (group, row r, intrinsic k) owns S[r][(m, k)] of
// every member m.  Row nA stands for the e_a row of the reduce buffer (row n32)
__global__ __launch_bounds__(256) void k_kd_fold_cols(double *S, KdGroups G, int nA, int n32) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)G.nmg * (nA + 1) * 10) return;
  const int k = (int)(t % 10);
  const size_t u = t / 10;
  const int r = (int)(u % (nA + 1)), g = (int)(u / (nA + 1));
  const int m0 = G.gptr[g], m1 = G.gptr[g + 1];
  if (!((kd_free_bits(G.mask, G.cmask, G.gmem[m0]) >> k) & 1u)) return;
  double *row = S + (size_t)(r == nA ? n32 : r) * n32;
  double s = 0.0;
  for (int q = m0; q < m1; q++) s += row[KD_CNP * G.gmem[q] + k];
  row[KD_CNP * G.gmem[m0] + k] = s;
}

// behind the column pass: the folded-away coordinates cleared to what a masked coordinate is (zero row and column,
// coeff + mu on the diagonal, e_a = 0), mu added once to the other diagonal entries, the upper triangle an exact
// copy of the lower (the two passes sum a mirrored pair in different orders).  D set: mu D_r in the place of mu (D of
// a representative's shared coordinate is the clamp of the folded diagonal, that of a folded-away one clamp(coeff))
__global__ __launch_bounds__(256) void k_kd_fold_finish(double *S, double *ea, KdGroups G, double coeff, double mu,
                                                        const double *D, int nA, int n32) {
  const size_t n2 = (size_t)nA * nA;
  const size_t gtid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gsize = (size_t)gridDim.x * blockDim.x;
  for (size_t t = gtid; t < n2; t += gsize) {
    const int r = (int)(t / nA), c = (int)(t % nA);
    const size_t at = (size_t)r * n32 + c;
    const double mud = (D && r == c) ? mu * D[r] : mu;
    if (kd_folded(G, r) || kd_folded(G, c))
      S[at] = r == c ? coeff + mud : 0.0;
    else if (r == c)
      S[at] += mud;
    else if (r < c)
      S[at] = S[(size_t)c * n32 + r];  // (below the diagonal a kept entry is not written by this kernel)
  }
  for (size_t t = gtid; t < (size_t)nA; t += gsize)
    if (kd_folded(G, (int)t)) ea[t] = 0.0;
}

// k_free_max_diag over the folded diagonal of U: a shared free coordinate counts once, with the sum over its group
template <bool HELD>
__global__ __launch_bounds__(1024) void k_kd_max_diag_groups(const double *U, const double *PV, int nC, int nP, KdGroups G,
                                                             const unsigned char *held_pose, const unsigned char *held_pt,
                                                             double *out) {
  __shared__ double sRed[16];
  double m = 0.0;
  for (int t = threadIdx.x; t < KD_CNP * nC; t += blockDim.x) {
    const int j = t / KD_CNP, r = t % KD_CNP;
    if (r < 10 && !((kd_free_bits(G.mask, G.cmask, j) >> r) & 1u)) continue;
    if (HELD && r >= 10 && held_pose[j]) continue;
    const int g = r < 10 ? G.gidx[j] : -1;
    if (g < 0) {
      m = fmax(m, U[(size_t)KD_CNP * KD_CNP * j + (KD_CNP + 1) * r]);
    } else if (G.rep[j] == j) {
      double s = 0.0;
      for (int q = G.gptr[g]; q < G.gptr[g + 1]; q++) s += U[(size_t)KD_CNP * KD_CNP * G.gmem[q] + (KD_CNP + 1) * r];
      m = fmax(m, s);
    }
  }
  for (int i = threadIdx.x; i < nP; i += blockDim.x) {
    if (HELD && held_pt[i]) continue;
    const double *v = PV + 9 * (size_t)i;
    m = fmax(m, fmax(v[0], fmax(v[3], v[5])));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
  if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; w++) m = fmax(m, sRed[w]);
    *out = m;
  }
}

// k_free_backsub_cams with the step expanded: a folded-away entry reads its representative's dp (which the
// representative's own thread leaves as solved) and writes only its own; dp_l2, mu dp^2 and newp_l2 count a shared
// parameter once, dp g goes over every entry (sum_all dp g = dp_shared P^T g)
template <bool HELD, bool PRIOR>
__global__ __launch_bounds__(256) void k_kd_backsub_cams_groups(FreeBackArgs p, const int *rep) {
  __shared__ double sRed[4][4];
  double v4[4] = {0.0, 0.0, 0.0, 0.0};
  if (threadIdx.x == 0) {
    p.scal[SC_STATUS_V] = (p.status[0] == p.status[3]) ? 1.0 : 0.0;
    p.scal[SC_STATUS_SPD] = (p.status[1] == p.status[3]) ? 1.0 : 0.0;
  }
  for (int t = threadIdx.x; t < p.nA; t += blockDim.x) {
    const int j = t / KD_CNP, r = t % KD_CNP;
    const bool hp = HELD && r >= 10 && p.held_pose[j];
    const bool held = hp || (r < 10 && !((kd_free_bits(p.mask, p.cmask, j) >> r) & 1u));
    const bool copy = r < 10 && !held && rep[j] != j;
    double d = copy ? p.dp[KD_CNP * (size_t)rep[j] + r] : p.dp[t];
    if (held) d = 0.0;
    if (held || copy) p.dp[t] = d;
    const double c = hp ? p.cams[t] : p.cams[t] + d;  // (a held pose keeps its bits, as in k_free_backsub_cams)
    p.newcams[t] = c;
    if (!copy) {
      const double mud = p.dm.D ? p.mu * p.dm.D[t] : p.mu;
      v4[0] += d * d;
      v4[1] += d * (mud * d + p.ga[t]);
      v4[3] += c * c;
    } else {
      v4[1] += d * p.ga[t];
    }
  }
  if (PRIOR) v4[2] = free_prior_newcost<KD_CNP>(p);  // (per camera: every member's own prior at the expanded proposal)
  free_block_sums4(v4, sRed, p.red);
}

// (kd_mask and kd_rep are what the setters left: they refuse blocks of 11, which so keep all free and no groups)
static FreeArgs free_args(psba_ctx *h, int set) {
  FreeArgs a;
  a.camconst = h->camconst;
  a.cams = h->cams[set];
  a.pts = h->pts[set];
  a.impts = h->impts;
  a.iidx = h->iidx;
  a.jidx = h->jidx;
  a.ptr = h->ptr;
  a.cam_obs = h->cam_obs;
  a.cam_units = h->cam_units;
  a.held_pose = h->held_poses;
  a.held_pt = h->held_pts;
  a.W = nullptr;
  a.Be = h->free_Be;
  a.upart = h->free_upart;
  a.coeff = h->coeff;
  a.mask = h->kd_mask;
  a.nO = h->d.nO;
  a.pub_src = h->scal;
  a.pub_dst = nullptr;
  a.pub_stamp = 0.0;
  a.isig = h->obs_isig;
  a.rl = make_robust_loss(h->wgt_kind, h->wgt_c);
  a.cmask = h->kd_cmask;
  return a;
}
static FreePriors free_priors(psba_ctx *h) {
  FreePriors pr;
  pr.cidx = h->prior_cidx;
  pr.pidx = h->prior_pidx;
  pr.crec = h->prior_crec;
  pr.prec = h->prior_prec;
  return pr;
}
static int free_grid(long long n, int cap) {
  const long long g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

template <class T, bool HELD, bool PRIOR, bool WGT>
static int linearize_free(psba_ctx *h, bool ahead, bool publish) {
  const Dims &d = h->d;
  const int set = ahead ? 1 - h->cur : h->cur;
  FreeArgs a = free_args(h, set);
  a.W = ahead ? h->W_alt : h->W;
  double *PVo = ahead ? h->PV_alt : h->PV;
  a.pub_dst = publish ? h->h_scal_dev : nullptr;
  a.pub_stamp = h->pub_seq;
  h->coeff_w = h->coeff;
  double *Uo = ahead ? h->U_alt : h->U, *gao = ahead ? h->ga_alt : h->ga;
  ProfScope ps(h, PSBA_K_LINEARIZE);
  hipLaunchKernelGGL((k_free_linearize<T, HELD, WGT>), dim3(h->nCamUnits), dim3(64), 0, h->stream, a);
  const long long nfin = (long long)d.nC * (T::CNP * T::CNP + T::CNP);
  const FreePriors pr = free_priors(h);
  hipLaunchKernelGGL((k_free_finish_cams<T, HELD, PRIOR>), dim3((unsigned)((nfin + 255) / 256)), dim3(256), 0, h->stream,
                     h->free_upart, h->free_cuptr, d.nC, h->coeff, h->coeff_g, h->kd_mask, a.cmask, a.held_pose, Uo, gao, pr,
                     a.cams);
  hipLaunchKernelGGL((k_free_point_sums<HELD, PRIOR>), dim3((unsigned)((d.nP + 255) / 256)), dim3(256), 0, h->stream,
                     h->free_Be, h->ptr, d.nP, h->coeff, h->coeff_g, a.held_pt, PVo, pr, a.pts);
  if (h->damp_kind == PSBA_DAMPING_MARQUARDT)  // D of this set, behind the two kernels whose sums it reads
    hipLaunchKernelGGL(k_free_damp_diag<T>, dim3((unsigned)((d.nT + 255) / 256)), dim3(256), 0, h->stream, (const double *)Uo,
                       (const double *)PVo, (const int *)h->kd_rep, (const int *)h->kd_gidx, (const int *)h->kd_gptr,
                       (const int *)h->kd_gmem, h->kd_mask, a.cmask, h->coeff, d.nA, d.nT, h->damp_dmin, h->damp_dmax,
                       (double *)(ahead ? h->damp_D_alt : h->damp_D));
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

// the priors' per-workgroup partial sums at (cams, pts): cameras then points, written to part; returns how many (at
// most 512), ncam: those of the cameras
template <class T>
static int prior_cost_parts(psba_ctx *h, const double *cams, const double *pts, double *part, int *ncam) {
  const int gc = h->n_cam_priors ? free_grid(h->n_cam_priors, 256) : 0, gp = h->n_pt_priors ? free_grid(h->n_pt_priors, 256) : 0;
  if (gc)
    hipLaunchKernelGGL(k_free_prior_cost<T::CNP>, dim3(gc), dim3(256), 0, h->stream, (const int *)h->prior_clist,
                       (const int *)h->prior_cidx, (const double *)h->prior_crec, cams, h->n_cam_priors, part);
  if (gp)
    hipLaunchKernelGGL(k_free_prior_cost<3>, dim3(gp), dim3(256), 0, h->stream, (const int *)h->prior_plist,
                       (const int *)h->prior_pidx, (const double *)h->prior_prec, pts, h->n_pt_priors, part + gc);
  if (ncam) *ncam = gc;
  return gc + gp;
}

// psba_prior_cost: the two prior sums on their own, out2 (device) = (cameras, points)
template <class T>
static int prior_cost_free(psba_ctx *h, int which, double *out2) {
  const int set = which == PSBA_PARAMS_NEW ? 1 - h->cur : h->cur;
  int gc = 0;
  const int rows = prior_cost_parts<T>(h, h->cams[set], h->pts[set], h->free_red, &gc);
  hipLaunchKernelGGL(k_free_sum_columns, dim3(1), dim3(64), 0, h->stream, (const double *)nullptr, (const double *)h->free_red,
                     gc, 1, out2);
  hipLaunchKernelGGL(k_free_sum_columns, dim3(1), dim3(64), 0, h->stream, (const double *)nullptr,
                     (const double *)h->free_red + gc, rows - gc, 1, out2 + 1);
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

template <class T, bool WGT>
static int residual_free(psba_ctx *h, int which) {
  const int set = which == PSBA_PARAMS_NEW ? 1 - h->cur : h->cur;
  FreeArgs a = free_args(h, set);
  const int grid = free_grid(h->d.nO, 256);
  ProfScope ps(h, PSBA_K_RESIDUAL);
  hipLaunchKernelGGL((k_free_residual<T, WGT>), dim3(grid), dim3(256), 0, h->stream, a, h->free_red);
  // F: the observations' partials, then the camera priors', then the point priors' (none without priors)
  const int rows = grid + prior_cost_parts<T>(h, a.cams, a.pts, h->free_red + grid, nullptr);
  hipLaunchKernelGGL(k_free_sum_columns, dim3(1), dim3(64), 0, h->stream, (const double *)nullptr, h->free_red, rows, 1,
                     h->scal + SC_COST);
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

template <class T, bool HELD>
static int max_diag_free(psba_ctx *h) {
  const unsigned char *hp = h->held_poses, *hq = h->held_pts;
  if (T::CNP == KD_CNP && h->kd_rep)
    hipLaunchKernelGGL(k_kd_max_diag_groups<HELD>, dim3(1), dim3(1024), 0, h->stream, h->U, h->PV, h->d.nC, h->d.nP,
                       kd_groups(h), hp, hq, h->scal + SC_MAXDIAG);
  else
    hipLaunchKernelGGL((k_free_max_diag<T, HELD>), dim3(1), dim3(1024), 0, h->stream, h->U, h->PV, h->d.nC, h->d.nP,
                       h->kd_mask, (const unsigned short *)h->kd_cmask, hp, hq, h->scal + SC_MAXDIAG);
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

// the rule of the tries on the current linearization
static FreeDamp free_damp(psba_ctx *h) {
  FreeDamp dm;
  dm.D = h->damp_kind == PSBA_DAMPING_MARQUARDT ? (const double *)h->damp_D : nullptr;
  dm.dmin = h->damp_dmin;
  dm.dmax = h->damp_dmax;
  return dm;
}

template <class T>
static int schur_free(psba_ctx *h, double mu) {
  const Dims &d = h->d;
  const FreeDamp dm = free_damp(h);
  h->try_id++;  // (the status words are generation stamps, as in launch_schur)
  h->diag_done = false;
  if (h->solver == PSBA_SOLVER_PCG) {  // PSBA_SOLVER_SPARSE: the same two kernels into the list of stored blocks
    ProfScope ps(h, PSBA_K_SCHUR);
    hipLaunchKernelGGL(k_free_Y<T>, dim3(h->nCamUnits), dim3(64), 0, h->stream, h->W, h->PV, h->iidx, h->cam_obs, h->cam_units,
                       h->free_Y, h->free_eapart, mu, dm, h->status, h->try_id);
    hipLaunchKernelGGL((k_free_schur<T, true>), dim3((unsigned)((h->free_nsegs + 3) / 4)), dim3(256), 0, h->stream, h->free_Y,
                       h->W, h->free_prods, h->free_segs, h->free_blocks, h->free_nsegs, h->bs_val, T::CNP, h->free_tiles);
    if (h->free_nmulti)
      hipLaunchKernelGGL((k_free_combine<T, true>), dim3(h->free_nmulti), dim3(256), 0, h->stream, h->free_multi,
                         h->free_tiles, h->bs_val, T::CNP);
    PSBA_HIP(h, hipGetLastError());
    h->packed_pending = false;
    return launch_fbsr_finalize(h, mu, dm.D);
  }
  double *S = h->red, *ea = h->red + (size_t)h->n32 * h->n32;
  PSBA_HIP(h, hipMemsetAsync(h->red, 0, sizeof(double) * (size_t)(h->n32 + 1) * h->n32, h->stream));
  {
    ProfScope ps(h, PSBA_K_SCHUR);
    hipLaunchKernelGGL(k_free_Y<T>, dim3(h->nCamUnits), dim3(64), 0, h->stream, h->W, h->PV, h->iidx, h->cam_obs, h->cam_units,
                       h->free_Y, h->free_eapart, mu, dm, h->status, h->try_id);
    hipLaunchKernelGGL(k_free_schur<T>, dim3((unsigned)((h->free_nsegs + 3) / 4)), dim3(256), 0, h->stream, h->free_Y, h->W,
                       h->free_prods, h->free_segs, h->free_blocks, h->free_nsegs, S, h->n32, h->free_tiles);
    if (h->free_nmulti)
      hipLaunchKernelGGL(k_free_combine<T>, dim3(h->free_nmulti), dim3(256), 0, h->stream, h->free_multi, h->free_tiles, S,
                         h->n32);
    const size_t n2 = (size_t)d.nA * d.nA;
    const int fgrid = (int)((n2 + 255) / 256 > 4096 ? 4096 : (n2 + 255) / 256);
    if (T::CNP == KD_CNP && h->kd_rep) {  // shared intrinsics: the undamped symmetric square, the fold in two passes, then mu and the mirror
      const KdGroups G = kd_groups(h);
      const size_t nrow = (size_t)G.nmg * 10 * d.nA, ncol = (size_t)G.nmg * 10 * (d.nA + 1);
      hipLaunchKernelGGL(k_kd_finalize_sym, dim3(fgrid), dim3(256), 0, h->stream, S, ea, h->U, h->ga, h->free_eapart,
                         h->free_cuptr, d.nA, h->n32, h->scal, h->status, h->try_id);
      hipLaunchKernelGGL(k_kd_fold_rows, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, h->stream, S, G, d.nA, h->n32);
      hipLaunchKernelGGL(k_kd_fold_cols, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, h->stream, S, G, d.nA, h->n32);
      hipLaunchKernelGGL(k_kd_fold_finish, dim3(fgrid), dim3(256), 0, h->stream, S, ea, G, h->coeff, mu, dm.D, d.nA, h->n32);
    } else {
      hipLaunchKernelGGL(k_free_finalize<T>, dim3(fgrid), dim3(256), 0, h->stream, S, ea, h->U, h->ga, h->free_eapart,
                         h->free_cuptr, mu, dm.D, d.nA, h->n32, h->scal, h->status, h->try_id);
    }
  }
  h->packed_pending = false;
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

template <class T, bool HELD, bool PRIOR, bool WGT>
static int backsub_free(psba_ctx *h, double mu) {
  const Dims &d = h->d;
  FreeBackArgs a;
  a.W = h->W;
  a.PV = h->PV;
  a.camconst = h->camconst;
  a.cams = h->cams[h->cur];
  a.pts = h->pts[h->cur];
  a.impts = h->impts;
  a.ga = h->ga;
  a.jidx = h->jidx;
  a.ptr = h->ptr;
  a.held_pose = h->held_poses;
  a.held_pt = h->held_pts;
  a.pr = free_priors(h);
  a.isig = h->obs_isig;
  a.rl = make_robust_loss(h->wgt_kind, h->wgt_c);
  a.dp = h->dp;
  a.newcams = h->cams[1 - h->cur];
  a.newpts = h->pts[1 - h->cur];
  a.scal = h->scal;
  a.red = h->free_red;
  a.status = h->status;
  a.mu = mu;
  a.dm = free_damp(h);
  a.mask = h->kd_mask;
  a.cmask = h->kd_cmask;
  a.nA = d.nA;
  a.nP = d.nP;
  const int grid = free_grid(d.nP, KD_RED / 4 - 8);
  ProfScope ps(h, PSBA_K_BACKSUB);
  if (T::CNP == KD_CNP && h->kd_rep)
    hipLaunchKernelGGL((k_kd_backsub_cams_groups<HELD, PRIOR>), dim3(1), dim3(256), 0, h->stream, a, (const int *)h->kd_rep);
  else
    hipLaunchKernelGGL((k_free_backsub_cams<T, HELD, PRIOR>), dim3(1), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL((k_free_backsub_pts<T, HELD, PRIOR, WGT>), dim3(grid), dim3(256), 0, h->stream, a);
  // set 0 of the SC_NPART partial sets carries the whole sums (k_free_finalize zeroed the others)
  hipLaunchKernelGGL(k_free_sum_columns, dim3(1), dim3(64), 0, h->stream, (const double *)h->free_red,
                     (const double *)h->free_red + 4, grid, 4, h->scal + SC_PART);
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

// psba_get_obs_weights: s and w (device, [nO] each) at a parameter set
template <class T>
static int obs_weights_free(psba_ctx *h, int which, double *s_dev, double *w_dev) {
  const int set = which == PSBA_PARAMS_NEW ? 1 - h->cur : h->cur;
  FreeArgs a = free_args(h, set);
  hipLaunchKernelGGL(k_free_obs_weights<T>, dim3((unsigned)((h->d.nO + 255) / 256)), dim3(256), 0, h->stream, a, s_dev, w_dev);
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

// one dispatch on the camera block per launcher; the launchers whose kernels read the held masks also on has_held,
// those whose kernels read the priors also on has_prior, those whose kernels see observations also on has_weighting
#define FREE_DISPATCH(fn, ...) (h->cnp == KD_CNP ? fn<FreeKD>(__VA_ARGS__) : fn<FreeK>(__VA_ARGS__))
#define FREE_DISPATCH_HELD(fn, ...)                                                                        \
  (h->cnp == KD_CNP ? (h->has_held ? fn<FreeKD, true>(__VA_ARGS__) : fn<FreeKD, false>(__VA_ARGS__)) \
                    : (h->has_held ? fn<FreeK, true>(__VA_ARGS__) : fn<FreeK, false>(__VA_ARGS__)))
#define FREE_DISPATCH_W(fn, ...)                                                                                   \
  (h->cnp == KD_CNP ? (h->has_weighting ? fn<FreeKD, true>(__VA_ARGS__) : fn<FreeKD, false>(__VA_ARGS__)) \
                    : (h->has_weighting ? fn<FreeK, true>(__VA_ARGS__) : fn<FreeK, false>(__VA_ARGS__)))
#define FREE_DISPATCH_HPW2(T, H, fn, ...)                                                                                  \
  (h->has_prior ? (h->has_weighting ? fn<T, H, true, true>(__VA_ARGS__) : fn<T, H, true, false>(__VA_ARGS__)) \
                : (h->has_weighting ? fn<T, H, false, true>(__VA_ARGS__) : fn<T, H, false, false>(__VA_ARGS__)))
#define FREE_DISPATCH_HPW1(T, fn, ...) (h->has_held ? FREE_DISPATCH_HPW2(T, true, fn, __VA_ARGS__) : FREE_DISPATCH_HPW2(T, false, fn, __VA_ARGS__))
#define FREE_DISPATCH_HPW(fn, ...) (h->cnp == KD_CNP ? FREE_DISPATCH_HPW1(FreeKD, fn, __VA_ARGS__) : FREE_DISPATCH_HPW1(FreeK, fn, __VA_ARGS__))
int launch_linearize_free(psba_ctx *h, bool ahead, bool publish) { return FREE_DISPATCH_HPW(linearize_free, h, ahead, publish); }
int launch_obs_weights_free(psba_ctx *h, int which, double *s_dev, double *w_dev) { return FREE_DISPATCH(obs_weights_free, h, which, s_dev, w_dev); }
int launch_prior_cost_free(psba_ctx *h, int which, double *out2_dev) { return FREE_DISPATCH(prior_cost_free, h, which, out2_dev); }
int launch_residual_free(psba_ctx *h, int which) { return FREE_DISPATCH_W(residual_free, h, which); }
int launch_max_diag_free(psba_ctx *h) { return FREE_DISPATCH_HELD(max_diag_free, h); }
int launch_schur_free(psba_ctx *h, double mu) { return FREE_DISPATCH(schur_free, h, mu); }
int launch_backsub_free(psba_ctx *h, double mu) { return FREE_DISPATCH_HPW(backsub_free, h, mu); }

}  // namespace psba
