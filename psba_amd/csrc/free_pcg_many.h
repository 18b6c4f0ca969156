// free_pcg_many.h -- what the two files of the multi-column conjugate gradients share (kernels_free_pcg_many.hip: unit
// right-hand sides of chosen cameras; kernels_free_pcg_points.hip: the Y right-hand sides of chosen points,
// DESIGN 7p): the layout of a panel's scalar block and the two fixed-order sums over it.
#pragma once
#include "psba_internal.h"

namespace psba {

// the scalar block of one panel (doubles, device): sixteen of each of k_fpcg's scalars, one per column, then the partial
// sums [slot][workgroup][16].  p.Sp, r.r and r.z of iteration `it` live in slot it % 4 (r.z of the next iteration in
// slot (it + 1) % 4), as in kernels_free_pcg.hip.  With unit right-hand sides b.b (1) and the first r.z (the diagonal
// entry of the block inverse) are written by the start kernel itself; with general ones (kernels_free_pcg_points.hip)
// they are sums, whose partials the start kernel leaves in the r.r partials of slot 3 and the r.z partials of slot 0
enum { MF_BB = 0, MF_FAIL = 16, MF_DONE = 32, MF_RRFIN = 48, MF_DEAD = 64, MF_ACT = 80, MF_RR = 96, MF_RZ = 160, MF_N = 224,
       MF_PQP = MF_N, MF_RRP = MF_N + 64 * FPCG_CAP, MF_RZP = MF_N + 128 * FPCG_CAP, MF_ALL = MF_N + 192 * FPCG_CAP };

// the workgroup's 256 values are 16 strands (threadIdx.x >> 4) of 16 columns (threadIdx.x & 15): sOut[col] = the
// strands' sum in ascending order
__device__ __forceinline__ void fpcgm_block_sums(double v, double *sW, double *sOut) {
  sW[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x < 16) {
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < 16; g++) s += sW[16 * g + threadIdx.x];
    sOut[threadIdx.x] = s;
  }
  __syncthreads();
}
// the sums of n <= FPCG_CAP partials [n][16]: strand g adds the partials g, g + 16, ... of its column in ascending
// order.  Every workgroup that calls this gets the same bits
__device__ __forceinline__ void fpcgm_sum_partials(const double *part, int n, double *sW, double *sOut) {
  double v = 0.0;
  for (int i = threadIdx.x >> 4; i < n; i += 16) v += part[16 * i + (threadIdx.x & 15)];
  fpcgm_block_sums(v, sW, sOut);
}

// kernels_free_pcg_many.hip, for kernels_free_pcg_points.hip: the vector kernels' grid, the verbs' buffers, and
// iterations it0 .. it0 + burst - 1 of the multi-column solve on the first np panels of those buffers (k_fpcgm_spmm,
// k_fpcgm_update, k_fpcgm_direction as psba_sparse_camera_covariance launches them)
int fcm_vec_grid(int n);
int fcm_buffers(psba_ctx *h, int panels);
int launch_fpcgm_burst(psba_ctx *h, int np, int it0, int burst);

}  // namespace psba
