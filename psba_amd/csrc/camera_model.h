// camera_model.h -- projection, residual and analytic Jacobian of one observation (fp64).
//
// Model (reference: CL_files/compute_exQT.cl:36-69, compute_jacobiQT.cl:113-140; restated
// from the mathematics in SURVEY.md Appendix B, not from the Maple expression list):
//   q_l = (sqrt(1-|v|^2), v),  q = q_l (x) q0  (Hamilton product, local rotation on the left)
//   P   = R'(q) M + t,  R'(q) = 2 u u^T + (s^2 - |u|^2) I + 2 s [u]x   (q = (s,u); the
//         quaternion sandwich q (0,M) q*, equal to the rotation matrix for unit q)
//   x   = (fu Px + sk Py + u0 Pz)/Pz,  y = (fu ar Py + v0 Pz)/Pz,  K = (fu,u0,v0,ar,sk)
//   e   = measured - (x,y);  A = d(x,y)/d(v,t) (2x6 row-major),  B = d(x,y)/dM (2x3 row-major)
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace psba {

#define PSBA_HD __host__ __device__ __forceinline__

// Every function of the per-observation model pins how its a * b + c contract: within one expression, as written, and
// never across statements (the compiler's default for device code fuses across statements wherever the inlined
// context allows, so two kernels that inline the same text rounded it differently: k_jmul's A against the dumping
// K1's on 54cams differed by 2.4e-12 |A| in an entry (v0 - y) / Pz that cancels, 2.7 times what the suites allow
// between instantiations).  With the contraction pinned, every kernel that evaluates the model on the same inputs
// gets the same bits: the blocks K3, k_cam_sums and k_jmul recompute are the ones K1 formed, and the robust weight
// is the same everywhere (below).  First statement of the function body.
#define PSBA_FP_PINNED _Pragma("clang fp contract(on)")

struct Quat {
  double s, u0, u1, u2;
};

PSBA_HD Quat compose_quat(const double *q0, double v0, double v1, double v2, double &sl) {
  PSBA_FP_PINNED;
  sl = sqrt(1.0 - v0 * v0 - v1 * v1 - v2 * v2);
  const double s0 = q0[0], a0 = q0[1], a1 = q0[2], a2 = q0[3];
  Quat q;
  q.s = sl * s0 - (a0 * v0 + a1 * v1 + a2 * v2);
  q.u0 = s0 * v0 + sl * a0 + a2 * v1 - a1 * v2;
  q.u1 = s0 * v1 + sl * a1 + a0 * v2 - a2 * v0;
  q.u2 = s0 * v2 + sl * a2 + a1 * v0 - a0 * v1;
  return q;
}

// R'(q), row-major
PSBA_HD void quat_matrix(const Quat &q, double *R) {
  PSBA_FP_PINNED;
  const double ss = q.s * q.s, x = q.u0, y = q.u1, z = q.u2;
  const double xx = x * x, yy = y * y, zz = z * z;
  R[0] = ss + xx - yy - zz;
  R[4] = ss - xx + yy - zz;
  R[8] = ss - xx - yy + zz;
  const double xy = x * y, xz = x * z, yz = y * z, sx = q.s * x, sy = q.s * y, sz = q.s * z;
  R[1] = 2.0 * (xy - sz);
  R[2] = 2.0 * (xz + sy);
  R[3] = 2.0 * (xy + sz);
  R[5] = 2.0 * (yz - sx);
  R[6] = 2.0 * (xz - sy);
  R[7] = 2.0 * (yz + sx);
}

// residual only.  cam = (v0,v1,v2,t0,t1,t2)
PSBA_HD void residual_obs(const double *K, const double *q0, const double *cam, const double *M,
                          double mx, double my, double &e0, double &e1) {
  PSBA_FP_PINNED;
  double sl, R[9];
  const Quat q = compose_quat(q0, cam[0], cam[1], cam[2], sl);
  quat_matrix(q, R);
  const double Px = R[0] * M[0] + R[1] * M[1] + R[2] * M[2] + cam[3];
  const double Py = R[3] * M[0] + R[4] * M[1] + R[5] * M[2] + cam[4];
  const double Pz = R[6] * M[0] + R[7] * M[1] + R[8] * M[2] + cam[5];
  const double inv = 1.0 / Pz;
  e0 = mx - (K[0] * Px + K[4] * Py + K[1] * Pz) * inv;
  e1 = my - (K[0] * K[3] * Py + K[2] * Pz) * inv;
}

// residual + Jacobian blocks
// xn: (optional) the normalised image coordinates (Px / Pz, Py / Pz): what d(x, y) / dK needs
PSBA_HD void linearize_obs(const double *K, const double *q0, const double *cam, const double *M,
                           double mx, double my, double *e, double *A, double *B, double *xn = nullptr) {
  PSBA_FP_PINNED;
  double sl, R[9];
  const Quat q = compose_quat(q0, cam[0], cam[1], cam[2], sl);
  quat_matrix(q, R);
  const double Px = R[0] * M[0] + R[1] * M[1] + R[2] * M[2] + cam[3];
  const double Py = R[3] * M[0] + R[4] * M[1] + R[5] * M[2] + cam[4];
  const double Pz = R[6] * M[0] + R[7] * M[1] + R[8] * M[2] + cam[5];
  const double inv = 1.0 / Pz;
  const double x = (K[0] * Px + K[4] * Py + K[1] * Pz) * inv;
  const double y = (K[0] * K[3] * Py + K[2] * Pz) * inv;
  e[0] = mx - x;
  e[1] = my - y;
  if (xn) {
    xn[0] = Px * inv;
    xn[1] = Py * inv;
  }
  // D = d(x,y)/dP
  const double d00 = K[0] * inv, d01 = K[4] * inv, d02 = (K[1] - x) * inv;
  const double d11 = K[0] * K[3] * inv, d12 = (K[2] - y) * inv;
  // translation columns
  A[3] = d00;
  A[4] = d01;
  A[5] = d02;
  A[9] = 0.0;
  A[10] = d11;
  A[11] = d12;
  // B = D R'
  B[0] = d00 * R[0] + d01 * R[3] + d02 * R[6];
  B[1] = d00 * R[1] + d01 * R[4] + d02 * R[7];
  B[2] = d00 * R[2] + d01 * R[5] + d02 * R[8];
  B[3] = d11 * R[3] + d12 * R[6];
  B[4] = d11 * R[4] + d12 * R[7];
  B[5] = d11 * R[5] + d12 * R[8];
  // rotation columns: dq_l/dv_k = (-v_k/s_l, e_k), dq = dq_l (x) q0 = (ds, du);
  // dP = 2 du (u.M) + 2 u (du.M) + 2 (s ds - u.du) M + 2 ds (u x M) + 2 s (du x M)
  const double s0 = q0[0], a0 = q0[1], a1 = q0[2], a2 = q0[3];
  const double isl = 1.0 / sl;
  const double udM = q.u0 * M[0] + q.u1 * M[1] + q.u2 * M[2];
  const double c0 = q.u1 * M[2] - q.u2 * M[1];  // u x M
  const double c1 = q.u2 * M[0] - q.u0 * M[2];
  const double c2 = q.u0 * M[1] - q.u1 * M[0];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double dsl = -cam[k] * isl;
    const double ak = (k == 0) ? a0 : (k == 1 ? a1 : a2);
    const double ds = dsl * s0 - ak;
    // e_k x a
    const double x0 = (k == 0) ? 0.0 : (k == 1 ? a2 : -a1);
    const double x1 = (k == 0) ? -a2 : (k == 1 ? 0.0 : a0);
    const double x2 = (k == 0) ? a1 : (k == 1 ? -a0 : 0.0);
    const double du0 = ((k == 0) ? s0 : 0.0) + dsl * a0 + x0;
    const double du1 = ((k == 1) ? s0 : 0.0) + dsl * a1 + x1;
    const double du2 = ((k == 2) ? s0 : 0.0) + dsl * a2 + x2;
    const double dudM = du0 * M[0] + du1 * M[1] + du2 * M[2];
    const double udu = q.u0 * du0 + q.u1 * du1 + q.u2 * du2;
    const double g = q.s * ds - udu;
    const double m0 = du1 * M[2] - du2 * M[1];  // du x M
    const double m1 = du2 * M[0] - du0 * M[2];
    const double m2 = du0 * M[1] - du1 * M[0];
    const double dP0 = 2.0 * (du0 * udM + q.u0 * dudM + g * M[0] + ds * c0 + q.s * m0);
    const double dP1 = 2.0 * (du1 * udM + q.u1 * dudM + g * M[1] + ds * c1 + q.s * m1);
    const double dP2 = 2.0 * (du2 * udM + q.u2 * dudM + g * M[2] + ds * c2 + q.s * m2);
    A[k] = d00 * dP0 + d01 * dP1 + d02 * dP2;
    A[6 + k] = d11 * dP1 + d12 * dP2;
  }
}

// Free intrinsics (the reference reads 11 parameters per camera, PSBA/main.cpp:73,140-149, and never
// optimises the first five, CL_files/PSBA.cl:5-7): camera block p = (fu, u0, v0, ar, s | v0, v1, v2 | t0, t1, t2).
// x = fu xn + s yn + u0, y = fu ar yn + v0 with (xn, yn) = (Px, Py) / Pz, so
//   d(x, y) / d(fu, u0, v0, ar, s) = [ xn, 1, 0, 0, yn ;  ar yn, 0, 1, fu yn, 0 ]
// and the other six columns are those of the fixed-K Jacobian.  A is 2 x 11 row-major.
constexpr int FK_CNP = 11;
PSBA_HD void linearize_obs_freek(const double *p, const double *q0, const double *M, double mx, double my, double *e,
                                 double *A, double *B) {
  PSBA_FP_PINNED;
  double A6[12], xn[2];
  linearize_obs(p, q0, p + 5, M, mx, my, e, A6, B, xn);
  A[0] = xn[0];
  A[1] = 1.0;
  A[2] = 0.0;
  A[3] = 0.0;
  A[4] = xn[1];
  A[FK_CNP + 0] = p[3] * xn[1];
  A[FK_CNP + 1] = 0.0;
  A[FK_CNP + 2] = 1.0;
  A[FK_CNP + 3] = p[0] * xn[1];
  A[FK_CNP + 4] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    A[5 + k] = A6[k];
    A[FK_CNP + 5 + k] = A6[6 + k];
  }
}

// ---- lens distortion and per-observation covariances (the reference reads both and never uses them) ----
// With (x, y) = (Px, Py) / Pz, r2 = x^2 + y^2 and kc = (k1, k2, k3, k4, k5) (Camera Calibration Toolbox order, the
// column order of the 17-column sba cams files):
//   radial = 1 + k1 r2 + k2 r2^2 + k5 r2^3
//   xd = radial x + 2 k3 x y + k4 (r2 + 2 x^2),   yd = radial y + k3 (r2 + 2 y^2) + 2 k4 x y
//   u = fu xd + s yd + u0,   v = fu ar yd + v0,   e = m - (u, v)
// Covariances: observation a has an SPD 2x2 Sigma_a; the host factors Sigma_a^-1 = L_a^T L_a with L_a upper
// triangular, stored (l00, l01, l11, 0).  The kernels whiten right after the projection (e <- L e, A <- L A,
// B <- L B), so the cost is sum e^T Sigma^-1 e and everything downstream is the same normal equations.
// The lens model of a kernel instantiation: bit 0 distortion, bit 1 covariances, bit 2 robust loss (below).
// Bit 3 (LENS_FIXED, below): some parameter blocks are held constant; set only at the launch sites of the kernels
// that form Jacobian blocks or finish a step (lens_dispatch_fixed), never in psba_ctx::lens.
enum { LENS_PLAIN = 0, LENS_DIST = 1, LENS_COV = 2, LENS_BOTH = 3, LENS_ROBUST = 4, LENS_MODELS = 8, LENS_FIXED = 8 };
constexpr int LENS_WSTRIDE = 4;  // doubles per observation of the whitening factors (l00, l01, l11, pad)

// (xd, yd) and, when J is given, d(xd, yd) / d(x, y) row-major
PSBA_HD void distort(const double *kc, double x, double y, double &xd, double &yd, double *J = nullptr) {
  PSBA_FP_PINNED;
  const double r2 = x * x + y * y;
  const double radial = 1.0 + r2 * (kc[0] + r2 * (kc[1] + r2 * kc[4]));
  const double xy = x * y;
  xd = radial * x + 2.0 * kc[2] * xy + kc[3] * (r2 + 2.0 * x * x);
  yd = radial * y + kc[2] * (r2 + 2.0 * y * y) + 2.0 * kc[3] * xy;
  if (J) {
    const double dr = kc[0] + r2 * (2.0 * kc[1] + 3.0 * kc[4] * r2);  // d radial / d r2
    J[0] = radial + 2.0 * x * x * dr + 2.0 * kc[2] * y + 6.0 * kc[3] * x;
    J[1] = 2.0 * xy * dr + 2.0 * kc[2] * x + 2.0 * kc[3] * y;
    J[2] = 2.0 * xy * dr + 2.0 * kc[2] * x + 2.0 * kc[3] * y;
    J[3] = radial + 2.0 * y * y * dr + 6.0 * kc[2] * y + 2.0 * kc[3] * x;
  }
}

PSBA_HD void residual_obs_dist(const double *K, const double *q0, const double *cam, const double *M, const double *kc,
                               double mx, double my, double &e0, double &e1) {
  PSBA_FP_PINNED;
  double sl, R[9];
  const Quat q = compose_quat(q0, cam[0], cam[1], cam[2], sl);
  quat_matrix(q, R);
  const double Px = R[0] * M[0] + R[1] * M[1] + R[2] * M[2] + cam[3];
  const double Py = R[3] * M[0] + R[4] * M[1] + R[5] * M[2] + cam[4];
  const double Pz = R[6] * M[0] + R[7] * M[1] + R[8] * M[2] + cam[5];
  const double inv = 1.0 / Pz;
  double xd, yd;
  distort(kc, Px * inv, Py * inv, xd, yd);
  e0 = mx - (K[0] * xd + K[4] * yd + K[1]);
  e1 = my - (K[0] * K[3] * yd + K[2]);
}

// residual + Jacobian blocks with distortion.  D = d(u, v) / dP = Kmat d(xd, yd) / d(x, y) d(x, y) / dP is a
// full 2 x 3 matrix (d10 != 0), so A[9] and the R[0..2] terms of B[3..5] are not the zeros of linearize_obs.
PSBA_HD void linearize_obs_dist(const double *K, const double *q0, const double *cam, const double *M, const double *kc,
                                double mx, double my, double *e, double *A, double *B) {
  PSBA_FP_PINNED;
  double sl, R[9];
  const Quat q = compose_quat(q0, cam[0], cam[1], cam[2], sl);
  quat_matrix(q, R);
  const double Px = R[0] * M[0] + R[1] * M[1] + R[2] * M[2] + cam[3];
  const double Py = R[3] * M[0] + R[4] * M[1] + R[5] * M[2] + cam[4];
  const double Pz = R[6] * M[0] + R[7] * M[1] + R[8] * M[2] + cam[5];
  const double inv = 1.0 / Pz;
  const double x = Px * inv, y = Py * inv;
  double xd, yd, J[4];
  distort(kc, x, y, xd, yd, J);
  e[0] = mx - (K[0] * xd + K[4] * yd + K[1]);
  e[1] = my - (K[0] * K[3] * yd + K[2]);
  // G = Kmat J, Kmat = [fu s; 0 fu ar]; d(x, y) / dP = [1 0 -x; 0 1 -y] / Pz
  const double fa = K[0] * K[3];
  const double g00 = K[0] * J[0] + K[4] * J[2], g01 = K[0] * J[1] + K[4] * J[3];
  const double g10 = fa * J[2], g11 = fa * J[3];
  double D[6];
  D[0] = g00 * inv;
  D[1] = g01 * inv;
  D[2] = -(g00 * x + g01 * y) * inv;
  D[3] = g10 * inv;
  D[4] = g11 * inv;
  D[5] = -(g10 * x + g11 * y) * inv;
#pragma unroll
  for (int r = 0; r < 2; r++) {
    A[6 * r + 3] = D[3 * r];
    A[6 * r + 4] = D[3 * r + 1];
    A[6 * r + 5] = D[3 * r + 2];
#pragma unroll
    for (int c = 0; c < 3; c++) B[3 * r + c] = D[3 * r] * R[c] + D[3 * r + 1] * R[3 + c] + D[3 * r + 2] * R[6 + c];
  }
  // rotation columns: dP / dv_k as in linearize_obs
  const double s0 = q0[0], a0 = q0[1], a1 = q0[2], a2 = q0[3];
  const double isl = 1.0 / sl;
  const double udM = q.u0 * M[0] + q.u1 * M[1] + q.u2 * M[2];
  const double c0 = q.u1 * M[2] - q.u2 * M[1];
  const double c1 = q.u2 * M[0] - q.u0 * M[2];
  const double c2 = q.u0 * M[1] - q.u1 * M[0];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double dsl = -cam[k] * isl;
    const double ak = (k == 0) ? a0 : (k == 1 ? a1 : a2);
    const double ds = dsl * s0 - ak;
    const double x0 = (k == 0) ? 0.0 : (k == 1 ? a2 : -a1);
    const double x1 = (k == 0) ? -a2 : (k == 1 ? 0.0 : a0);
    const double x2 = (k == 0) ? a1 : (k == 1 ? -a0 : 0.0);
    const double du0 = ((k == 0) ? s0 : 0.0) + dsl * a0 + x0;
    const double du1 = ((k == 1) ? s0 : 0.0) + dsl * a1 + x1;
    const double du2 = ((k == 2) ? s0 : 0.0) + dsl * a2 + x2;
    const double dudM = du0 * M[0] + du1 * M[1] + du2 * M[2];
    const double udu = q.u0 * du0 + q.u1 * du1 + q.u2 * du2;
    const double g = q.s * ds - udu;
    const double m0 = du1 * M[2] - du2 * M[1];
    const double m1 = du2 * M[0] - du0 * M[2];
    const double m2 = du0 * M[1] - du1 * M[0];
    const double dP0 = 2.0 * (du0 * udM + q.u0 * dudM + g * M[0] + ds * c0 + q.s * m0);
    const double dP1 = 2.0 * (du1 * udM + q.u1 * dudM + g * M[1] + ds * c1 + q.s * m1);
    const double dP2 = 2.0 * (du2 * udM + q.u2 * dudM + g * M[2] + ds * c2 + q.s * m2);
    A[k] = D[0] * dP0 + D[1] * dP1 + D[2] * dP2;
    A[6 + k] = D[3] * dP0 + D[4] * dP1 + D[5] * dP2;
  }
}

// Free intrinsics with distortion (PSBA_CAMERA_FREE_KD; the same model in include/psba_hip.h and DESIGN 7d): camera
// block p = (fu, u0, v0, ar, s | k1, k2, k3, k4, k5 | v0, v1, v2 | t0, t1, t2), kc = p + 5 in the order of distort().
// With (x, y) the normalised point, r2 = x^2 + y^2 and (xd, yd) = distort(kc, x, y):
//   d(u, v) / d(fu, u0, v0, ar, s) = [ xd, 1, 0, 0, yd ;  ar yd, 0, 1, fu yd, 0 ]
//   d xd / d(k1..k5) = (r2 x, r2^2 x, 2 x y, r2 + 2 x^2, r2^3 x)
//   d yd / d(k1..k5) = (r2 y, r2^2 y, r2 + 2 y^2, 2 x y, r2^3 y)
//   d u / dk = fu d xd + s d yd,   d v / dk = fu ar d yd
// and the six extrinsic columns and B are those of linearize_obs_dist.  A is 2 x 16 row-major.
// free_mask: bit k set = intrinsic k (k < 10) is optimised; a cleared bit zeroes that column of A (psba_set_intrinsics_mask).
constexpr int KD_CNP = 16;
constexpr unsigned KD_ALL_FREE = 0x3FFu;
PSBA_HD void linearize_obs_freekd(const double *p, const double *q0, const double *M, double mx, double my, double *e,
                                  double *A, double *B, unsigned free_mask = KD_ALL_FREE) {
  PSBA_FP_PINNED;
  double A6[12];
  linearize_obs_dist(p, q0, p + 10, M, p + 5, mx, my, e, A6, B);
  // the normalised point once more (three products: cheaper than widening linearize_obs_dist's interface)
  double sl, R[9];
  const Quat q = compose_quat(q0, p[10], p[11], p[12], sl);
  quat_matrix(q, R);
  const double Px = R[0] * M[0] + R[1] * M[1] + R[2] * M[2] + p[13];
  const double Py = R[3] * M[0] + R[4] * M[1] + R[5] * M[2] + p[14];
  const double Pz = R[6] * M[0] + R[7] * M[1] + R[8] * M[2] + p[15];
  const double inv = 1.0 / Pz;
  const double x = Px * inv, y = Py * inv;
  double xd, yd;
  distort(p + 5, x, y, xd, yd);
  const double r2 = x * x + y * y, xy2 = 2.0 * x * y;
  const double dxd[5] = {r2 * x, r2 * r2 * x, xy2, r2 + 2.0 * x * x, r2 * r2 * r2 * x};
  const double dyd[5] = {r2 * y, r2 * r2 * y, r2 + 2.0 * y * y, xy2, r2 * r2 * r2 * y};
  const double fa = p[0] * p[3];
  A[0] = xd;
  A[1] = 1.0;
  A[2] = 0.0;
  A[3] = 0.0;
  A[4] = yd;
  A[KD_CNP + 0] = p[3] * yd;
  A[KD_CNP + 1] = 0.0;
  A[KD_CNP + 2] = 1.0;
  A[KD_CNP + 3] = p[0] * yd;
  A[KD_CNP + 4] = 0.0;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    A[5 + k] = p[0] * dxd[k] + p[4] * dyd[k];
    A[KD_CNP + 5 + k] = fa * dyd[k];
  }
#pragma unroll
  for (int k = 0; k < 10; k++) {
    const bool fr = (free_mask >> k) & 1u;
    A[k] = fr ? A[k] : 0.0;
    A[KD_CNP + k] = fr ? A[KD_CNP + k] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) {
    A[10 + k] = A6[k];
    A[KD_CNP + 10 + k] = A6[6 + k];
  }
}

// e <- L e, A <- L A, B <- L B with L = [l00 l01; 0 l11] (w = (l00, l01, l11))
PSBA_HD void whiten2(const double *w, double &e0, double &e1) {
  PSBA_FP_PINNED;
  const double t = w[0] * e0 + w[1] * e1;
  e1 = w[2] * e1;
  e0 = t;
}
PSBA_HD void whiten_obs(const double *w, double *e, double *A, double *B) {
  whiten2(w, e[0], e[1]);
#pragma unroll
  for (int k = 0; k < 6; k++) whiten2(w, A[k], A[6 + k]);
#pragma unroll
  for (int k = 0; k < 3; k++) whiten2(w, B[k], B[3 + k]);
}

// ---- robust losses (the same model in include/psba_hip.h and DESIGN 7b) ----
// s_a = ||L_a e_a||^2 is the whitened squared residual (L_a = I without covariances); the cost is F = sum_a rho(s_a)
// with a scale c > 0 in whitened units (pixels when Sigma = I), c2 = c^2:
//   NONE     rho = s                            rho' = 1
//   HUBER    rho = s (s <= c2), 2 c sqrt(s) - c2  rho' = 1, c / sqrt(s)
//   CAUCHY   rho = c2 log(1 + s / c2)            rho' = 1 / (1 + s / c2)
//   SOFT_L1  rho = 2 c2 (sqrt(1 + s / c2) - 1)   rho' = 1 / sqrt(1 + s / c2)
// rho(0) = 0 and rho'(0) = 1 for all four (no 1/2: the reference's convention).  The normal equations are those of
// weighted Gauss-Newton (IRLS): w = sqrt(rho'(s)) after the whitening, e <- w e, A <- w A, B <- w B, so that
// A~^T e~ is the gradient of F (halved, in the sign convention of g).  The rho'' term of the Hessian is left out:
// it is negative for these three losses and would break positive definiteness.
// The kind is uniform over a launch (no divergence within a wave); w is recomputed wherever the Jacobian blocks
// are (K1, K3, k_jmul) from the same inputs, so every kernel sees the same w bit for bit and none is stored.
enum { LOSS_NONE = 0, LOSS_HUBER = 1, LOSS_CAUCHY = 2, LOSS_SOFT_L1 = 3 };
struct RobustLoss {
  double c, c2, ic2;  // scale, c^2, 1 / c^2
  int kind;
};
inline RobustLoss make_robust_loss(int kind, double c) {
  RobustLoss r;
  r.c = c;
  r.c2 = c * c;
  r.ic2 = 1.0 / r.c2;
  r.kind = kind;
  return r;
}
// rho(s) and w = sqrt(rho'(s)).  Huber's two branches are a select (both sides are finite or unused: c / 0 = inf
// only where s <= c2 picks 1); soft-L1's rho is written as 2 s / (sqrt(1 + s / c2) + 1), the same value without the
// cancellation of sqrt(1 + s / c2) - 1 at s << c2.
PSBA_HD void robust_eval(const RobustLoss &rl, double s, double &rho, double &w) {
  PSBA_FP_PINNED;
  switch (rl.kind) {
    case LOSS_HUBER: {
      const double r = sqrt(s);
      const bool in = s <= rl.c2;
      rho = in ? s : 2.0 * rl.c * r - rl.c2;
      w = in ? 1.0 : sqrt(rl.c / r);
      break;
    }
    case LOSS_CAUCHY: {
      const double u = 1.0 + s * rl.ic2;
      rho = rl.c2 * log1p(s * rl.ic2);
      w = 1.0 / sqrt(u);
      break;
    }
    case LOSS_SOFT_L1: {
      const double r = sqrt(1.0 + s * rl.ic2);
      rho = 2.0 * s / (r + 1.0);
      w = 1.0 / sqrt(r);
      break;
    }
    default:
      rho = s;
      w = 1.0;
      break;
  }
}
// e <- w e, A <- w A, B <- w B with w of s = |e|^2 (e already whitened)
PSBA_HD void robust_scale(const RobustLoss &rl, double *e, double *A, double *B) {
  PSBA_FP_PINNED;
  double rho, w;
  robust_eval(rl, e[0] * e[0] + e[1] * e[1], rho, w);
  e[0] *= w;
  e[1] *= w;
#pragma unroll
  for (int k = 0; k < 12; k++) A[k] *= w;
#pragma unroll
  for (int k = 0; k < 6; k++) B[k] *= w;
}

// ---- fixed parameter blocks (the same model in include/psba_hip.h and DESIGN 7c) ----
// psba_set_fixed marks cameras and points that are held constant.  The problem solved is the reduced one: the
// columns of J that belong to fixed blocks are deleted and the fixed values enter the residual as constants.  It is
// stored embedded in the full-size system: A_ij = 0 for a fixed camera j and B_ij = 0 for a fixed point i (applied
// after the whitening and the loss weight: zeroing commutes with both), hence W_ij = 0 if either is fixed,
// g_a,j = 0 and g_b,i = 0 exactly; the stored diagonal block of a fixed camera (U_j) or point (V_i) is the
// placeholder coeff I, which keeps V_i + mu I and S positive definite at mu = 0; dp is exactly 0 on fixed entries.
// The residual e and the cost are untouched: every observation counts.
// The mask is two byte arrays on the device (non-zero = fixed), read only by the LENS_FIXED instantiations: the
// kernels' last argument, behind the robust loss, so that every other argument keeps its offset.
struct FixedMask {
  const unsigned char *cams, *pts;  // [nC], [nP]; either may be null (none of that kind)
};
enum { FIX_CAM = 1, FIX_PT = 2 };
// which of observation (i, j)'s two blocks are fixed (0 without the bit: no load)
template <int LM>
PSBA_HD int fix_load(const FixedMask &fm, size_t i, size_t j) {
  if constexpr ((LM & LENS_FIXED) != 0)
    return ((fm.cams && fm.cams[j]) ? FIX_CAM : 0) | ((fm.pts && fm.pts[i]) ? FIX_PT : 0);
  else
    return 0;
}
template <int LM>
PSBA_HD bool fix_cam(const FixedMask &fm, size_t j) {
  if constexpr ((LM & LENS_FIXED) != 0)
    return fm.cams && fm.cams[j];
  else
    return false;
}
template <int LM>
PSBA_HD bool fix_pt(const FixedMask &fm, size_t i) {
  if constexpr ((LM & LENS_FIXED) != 0)
    return fm.pts && fm.pts[i];
  else
    return false;
}
// A <- 0 under FIX_CAM, B <- 0 under FIX_PT (selects: no divergence)
template <int LM>
PSBA_HD void fix_mask(int fx, double *A, double *B) {
  if constexpr ((LM & LENS_FIXED) != 0) {
    const bool fc = (fx & FIX_CAM) != 0, fp = (fx & FIX_PT) != 0;
#pragma unroll
    for (int k = 0; k < 12; k++) A[k] = fc ? 0.0 : A[k];
#pragma unroll
    for (int k = 0; k < 6; k++) B[k] = fp ? 0.0 : B[k];
  }
}

// an entry of W_ij = coeff A^T B under the mask: +0.0 when either block is fixed.  The product of the zeroed block is a
// zero already, but 0 * x keeps x's sign, and the stored W of a fixed block is +0.0 like g and dp (a select)
template <int LM>
PSBA_HD double fix_w(int fx, double w) {
  if constexpr ((LM & LENS_FIXED) != 0)
    return fx ? 0.0 : w;
  else
    return w;
}

// loads of camera j's kc and observation a's whitening factors (nothing under a model without them)
template <int LM>
PSBA_HD void lens_load_kc(const double *src, size_t j, double *kc) {
  if constexpr ((LM & LENS_DIST) != 0) {
#pragma unroll
    for (int k = 0; k < 5; k++) kc[k] = src[5 * j + k];
  }
}
template <int LM>
PSBA_HD void lens_load_w(const double *src, size_t a, double *w) {
  if constexpr ((LM & LENS_COV) != 0) {
    const double2 w01 = reinterpret_cast<const double2 *>(src)[2 * a];
    w[0] = w01.x;
    w[1] = w01.y;
    w[2] = src[LENS_WSTRIDE * a + 2];
  }
}

// the per-observation entry points of the fixed-intrinsics kernels: LM = LENS_PLAIN is exactly linearize_obs /
// residual_obs (kc, w and rl are not read)
template <int LM>
PSBA_HD void lens_linearize(const double *cc, const double *cam, const double *M, const double *kc, const double *w,
                            const RobustLoss &rl, double mx, double my, double *e, double *A, double *B) {
  if constexpr ((LM & LENS_DIST) != 0)
    linearize_obs_dist(cc, cc + 5, cam, M, kc, mx, my, e, A, B);
  else
    linearize_obs(cc, cc + 5, cam, M, mx, my, e, A, B);
  if constexpr ((LM & LENS_COV) != 0) whiten_obs(w, e, A, B);
  if constexpr ((LM & LENS_ROBUST) != 0) robust_scale(rl, e, A, B);
}
template <int LM>
PSBA_HD void lens_residual(const double *cc, const double *cam, const double *M, const double *kc, const double *w,
                           double mx, double my, double &e0, double &e1) {
  if constexpr ((LM & LENS_DIST) != 0)
    residual_obs_dist(cc, cc + 5, cam, M, kc, mx, my, e0, e1);
  else
    residual_obs(cc, cc + 5, cam, M, mx, my, e0, e1);
  if constexpr ((LM & LENS_COV) != 0) whiten2(w, e0, e1);
}
// the cost term of one observation from its whitened residual (lens_residual): s = |e|^2, or rho(s) under the robust
// bit, which also scales e <- w e (the residual the normal equations see) and stores s to *s_out when given
template <int LM>
PSBA_HD double lens_cost(const RobustLoss &rl, double &e0, double &e1, double *s_out = nullptr) {
  PSBA_FP_PINNED;
  const double s = e0 * e0 + e1 * e1;
  if constexpr ((LM & LENS_ROBUST) != 0) {
    double rho, w;
    robust_eval(rl, s, rho, w);
    e0 *= w;
    e1 *= w;
    if (s_out) *s_out = s;
    return rho;
  } else {
    return s;
  }
}

// calls f(std::integral_constant<int, LM>()) for the lens model lm of a handle (the launch sites' dispatch)
template <class F>
void lens_dispatch(int lm, F &&f) {
  switch (lm) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 6: f(std::integral_constant<int, 6>()); break;
    case 7: f(std::integral_constant<int, 7>()); break;
    default: f(std::integral_constant<int, 0>()); break;
  }
}

// the same with the LENS_FIXED bit on top (lm = psba_ctx::lens, fixed = a mask is set): the launch sites of K1, K3,
// k_cam_sums and k_jmul.  A handle without a mask runs the instantiations lens_dispatch picks.
template <class F>
void lens_dispatch_fixed(int lm, bool fixed, F &&f) {
  if (!fixed) return lens_dispatch(lm, f);
  switch (lm) {
    case 1: f(std::integral_constant<int, LENS_FIXED | 1>()); break;
    case 2: f(std::integral_constant<int, LENS_FIXED | 2>()); break;
    case 3: f(std::integral_constant<int, LENS_FIXED | 3>()); break;
    case 4: f(std::integral_constant<int, LENS_FIXED | 4>()); break;
    case 5: f(std::integral_constant<int, LENS_FIXED | 5>()); break;
    case 6: f(std::integral_constant<int, LENS_FIXED | 6>()); break;
    case 7: f(std::integral_constant<int, LENS_FIXED | 7>()); break;
    default: f(std::integral_constant<int, LENS_FIXED | 0>()); break;
  }
}

// symmetric 3x3 inverse by the closed form the reference uses (T = -det,
// CL_files/compute_Vinv.cl:29,76-86).  v = (v00,v01,v02,v11,v12,v22) -> same packing.
// Returns true when |T| < 1e-16 (the reference's singular flag).
PSBA_HD bool sym3_inverse(const double *v, double *o) {
  const double a11 = v[0], a12 = v[1], a13 = v[2], a22 = v[3], a23 = v[4], a33 = v[5];
  const double T = (a33 * a12 * a12 - 2.0 * a12 * a13 * a23 + a22 * a13 * a13 + a11 * a23 * a23 -
                    a11 * a22 * a33);
  const double iT = -1.0 / T;
  o[0] = (a22 * a33 - a23 * a23) * iT;
  o[1] = (a13 * a23 - a12 * a33) * iT;
  o[2] = (a12 * a23 - a13 * a22) * iT;
  o[3] = (a11 * a33 - a13 * a13) * iT;
  o[4] = (a12 * a13 - a11 * a23) * iT;
  o[5] = (a11 * a22 - a12 * a12) * iT;
  return fabs(T) < 1e-16;
}

// V y = w for a symmetric positive definite 3x3 V (same packing) by L D L^T and substitution.  Unlike a product
// with the explicit inverse this is backward stable per right-hand side, which is what keeps Y_a W_b^T accurate when
// V_i + mu I is nearly singular (a point seen once and a small mu: V_i has rank 2 and W, g_b carry no component along
// its null direction -- an unstructured error of the inverse would be amplified by the condition number).
struct Sym3Ldl {
  double l10, l20, l21, i0, i1, i2;  // unit lower factor, reciprocals of D
};
PSBA_HD Sym3Ldl sym3_ldl(const double *v) {
  Sym3Ldl f;
  f.i0 = 1.0 / v[0];
  f.l10 = v[1] * f.i0;
  f.l20 = v[2] * f.i0;
  const double d1 = v[3] - f.l10 * v[1];
  f.i1 = 1.0 / d1;
  f.l21 = (v[4] - f.l20 * v[1]) * f.i1;
  f.i2 = 1.0 / (v[5] - f.l20 * v[2] - f.l21 * f.l21 * d1);
  return f;
}
PSBA_HD void sym3_ldl_solve(const Sym3Ldl &f, double w0, double w1, double w2, double &y0, double &y1, double &y2) {
  const double z1 = w1 - f.l10 * w0, z2 = w2 - f.l20 * w0 - f.l21 * z1;
  y2 = z2 * f.i2;
  y1 = z1 * f.i1 - f.l21 * y2;
  y0 = w0 * f.i0 - f.l10 * y1 - f.l20 * y2;
}

// Marquardt's scaling of the damping (psba_set_damping): D_k from the stored diagonal entry N_kk of the
// linearization -- the one place the clamps are applied, for cameras, points, held and folded-away coordinates alike
PSBA_HD double damp_diag(double nkk, double dmin, double dmax) { return fmin(fmax(nkk, dmin), dmax); }
// V_i + mu diag(D_i) in place (v = sym6 packing), D_i formed from V_i's own diagonal in registers.  k_free_Y and
// k_free_backsub_pts both come through here, with an explicit fma, so that the back-substitution solves against the
// very bits Y was made with
PSBA_HD void damp_point_block(double *v, double mu, double dmin, double dmax) {
  v[0] = fma(mu, damp_diag(v[0], dmin, dmax), v[0]);
  v[3] = fma(mu, damp_diag(v[3], dmin, dmax), v[3]);
  v[5] = fma(mu, damp_diag(v[5], dmin, dmax), v[5]);
}

}  // namespace psba
