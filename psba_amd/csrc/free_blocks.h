// free_blocks.h -- what the kernel files that serve the free-intrinsics route share (kernels_free.hip, kernels_cov.hip):
// the two camera blocks the kernels are templated on, and the groups' tables with the predicate of a folded-away
// coordinate, and the free bits of a camera under the per-camera masks.
#pragma once
#include "camera_model.h"
#include "psba_internal.h"

namespace psba {

typedef double kd4 __attribute__((ext_vector_type(4)));

// the camera block: CNP parameters, the first NI of them intrinsics (the mask's bits); linearization and residual
struct FreeK {
  static constexpr int CNP = FK_CNP, NI = 5;
  static __device__ __forceinline__ void linearize(const double *cam, const double *q0, const double *M, double mx,
                                                   double my, double *e, double *A, double *B, unsigned) {
    linearize_obs_freek(cam, q0, M, mx, my, e, A, B);  // (no mask: all five intrinsics are free)
  }
  static __device__ __forceinline__ void residual(const double *cam, const double *q0, const double *M, double mx,
                                                  double my, double &e0, double &e1) {
    residual_obs(cam, q0, cam + 5, M, mx, my, e0, e1);
  }
};
struct FreeKD {
  static constexpr int CNP = KD_CNP, NI = 10;
  static __device__ __forceinline__ void linearize(const double *cam, const double *q0, const double *M, double mx,
                                                   double my, double *e, double *A, double *B, unsigned mask) {
    linearize_obs_freekd(cam, q0, M, mx, my, e, A, B, mask);
  }
  static __device__ __forceinline__ void residual(const double *cam, const double *q0, const double *M, double mx,
                                                  double my, double &e0, double &e1) {
    residual_obs_dist(cam, q0, cam + 10, M, cam + 5, mx, my, e0, e1);
  }
};
// ---- per-camera masks (psba_set_camera_masks) ----
// cmask [nC]: one word per camera, bit k set = row j of the table frees intrinsic k.  Null: no table, and the branch
// (uniform: the pointer is a kernel argument) leaves the global mask as it is, with no load -- the idiom of FreeDamp::D.
// Every kernel that asks "is intrinsic k of camera j optimised" asks these bits; a coordinate they mask is what a
// coordinate masked by psba_set_intrinsics_mask is.  The members of a group carry equal rows (the setters see to it),
// so the kernels of the groups take the bits of any member for the group.
__device__ __forceinline__ unsigned kd_free_bits(unsigned mask, const unsigned short *cmask, int j) {
  return cmask ? mask & cmask[j] : mask;
}

// ---- intrinsics shared between cameras (psba_set_intrinsics_groups): the tables of the groups ----
struct KdGroups {
  const int *rep;   // [nC] representative of each camera
  const int *gidx;  // [nC] the camera's group among those with several members, -1: alone
  const int *gptr;  // [nmg + 1] CSR over gmem
  const int *gmem;  // members, ascending; the first of a group is its representative
  int nmg;
  unsigned mask;
  const unsigned short *cmask;  // [nC] per-camera masks, null: none (kd_free_bits)
};
__device__ __forceinline__ bool kd_folded(const KdGroups &G, int t) {  // t: coordinate of the camera part
  const int k = t % KD_CNP;
  return k < 10 && ((kd_free_bits(G.mask, G.cmask, t / KD_CNP) >> k) & 1u) && G.rep[t / KD_CNP] != t / KD_CNP;
}
// the handle's tables as a kernel argument
inline KdGroups kd_groups(const psba_ctx *h) {
  KdGroups G;
  G.rep = h->kd_rep;
  G.gidx = h->kd_gidx;
  G.gptr = h->kd_gptr;
  G.gmem = h->kd_gmem;
  G.nmg = h->kd_nmg;
  G.mask = h->kd_mask;
  G.cmask = h->kd_cmask;
  return G;
}

}  // namespace psba
