// kernels_backsub.hip -- K3: point back-substitution, proposal and its cost in one pass.
//
// Replaces kern_compute_eb, kern_compute_dpb, kern_compute_newp, the second
// kern_compute_exQT of a damping try and the host-side compute_L2_sq / compute_rho sums
// (reference CL_files/compute_eb.cl:6-41, compute_dpb.cl:6-35, compute_newp.cl:6-26,
// compute_exQT.cl:18-71; PSBA/sba_func.cpp:1001-1213; PSBA/levmar.cpp:151-195,271-280;
// PSBA/misc.cpp:151-157).  The reference copies dp (nT doubles) and ex (2 nO doubles) to the
// host on every try; here only four scalars leave the device.
//
// Per tile of whole points: thread per observation forms W_ij^T dpa_j; thread per point
// finishes e_b,i, applies V*_i^-1, writes dpb_i and the proposed point; thread per
// observation then evaluates the residual at the proposal.
#include <cstdlib>

#include "camera_model.h"
#include "psba_internal.h"

namespace psba {

struct BackArgs {
  const double *W, *PV, *camconst, *cams, *pts, *impts, *ga;
  const int *iidx, *jidx, *ptr;
  const int4 *tile_desc;
  double *dp;          // [nA] dpa (in) | [nB] dpb (out)
  double *newcams, *newpts;
  double *scal;        // the four sums accumulate in scal[SC_PART ...]
  double *dbg_eb;
  const int *status;   // [0] singular-V stamp, [1] not-SPD stamp, [3] this try's stamp
  double mu;
  double coeff;        // W_ij = coeff A_ij^T B_ij (the coefficient of the linearization W came from)
  int nC, nA, nTiles;
  int cam_terms;       // 1 on the rank that owns the camera terms of the scalar sums
  int mode;            // development ablation (PSBA_BACK_MODE): 1 no residual pass, 2 no W^T dpa pass
  const double *kc, *wl;  // lens model (camera_model.h): read only by the LENS_DIST / LENS_COV instantiations
};  // (the robust loss is the kernels' last argument, read only by the LENS_ROBUST instantiations)

// RECOMP: W_ij^T dpa_j = coeff B_ij^T (A_ij dpa_j) from the Jacobian blocks recomputed at the current
// parameters (~300 flop per observation) instead of from the stored W (144 bytes per observation:
// 50 of the kernel's 66 MB at venice size); the camera constants and parameters loaded for it are
// the ones the residual pass needs anyway.  (PSBA_BACK_READ_W=1: the W-reading form.)
template <bool DUMP, bool RECOMP, int LM>
__global__ __launch_bounds__(TILE_OBS) void k_backsub(BackArgs p, RobustLoss rl, FixedMask fm) {
  __shared__ double sT[TILE_OBS][3];   // W_a^T dpa_j per observation
  __shared__ double sNP[TILE_OBS][3];  // proposed point per point of the tile
  __shared__ double sRed[4][4];
  const int tid = threadIdx.x;
  double s_dp = 0.0, s_den = 0.0, s_cost = 0.0, s_np = 0.0;

  // camera part (once): proposal cams + dpa and the camera terms of the scalar sums.
  // g_a here is this rank's partial; the sum over ranks of dpa.g_a is the full term.
  if (blockIdx.x == 0) {
    // the try's status as summable flags right behind the partial sums, so that
    // one all-reduce (sum) over ranks covers scalars and status
    if (tid == 0) {
      p.scal[SC_STATUS_V] = (p.status[0] == p.status[3]) ? 1.0 : 0.0;
      p.scal[SC_STATUS_SPD] = (p.status[1] == p.status[3]) ? 1.0 : 0.0;
    }
    for (int t = tid; t < p.nA; t += TILE_OBS) {
      // a fixed camera: dpa_j is zero whatever the solver returned, and the proposal is the current block bit for bit
      // (every other reader of dpa in this kernel masks it the same way, so the store below races with nothing)
      const bool fc = fix_cam<LM>(fm, t / 6);
      const double d = fc ? 0.0 : p.dp[t], c = fc ? p.cams[t] : p.cams[t] + d;
      if (fc) p.dp[t] = 0.0;
      p.newcams[t] = c;
      s_den += d * p.ga[t];
      if (p.cam_terms) {
        s_dp += d * d;
        s_den += p.mu * d * d;
        s_np += c * c;
      }
    }
  }

  // the dependent index loads of a tile (descriptor -> observation indices -> point CSR) are
  // issued one tile ahead
  int tile = blockIdx.x;
  int4 dsc = tile < p.nTiles ? p.tile_desc[tile] : make_int4(0, 0, 0, 0);
  int i = 0, j = 0;
  if (dsc.z + tid < dsc.w) {
    i = p.iidx[dsc.z + tid];
    j = p.jidx[dsc.z + tid];
  }
  for (; tile < p.nTiles; tile += gridDim.x) {
    const int p0 = dsc.x, p1 = dsc.y, o0 = dsc.z, o1 = dsc.w;
    const int a = o0 + tid;
    const int tn = tile + gridDim.x;
    const int4 dn = tn < p.nTiles ? p.tile_desc[tn] : make_int4(0, 0, 0, 0);
    int pb0 = 0, pb1 = 0;  // CSR bounds of this thread's point
    if (p0 + tid < p1) {
      pb0 = p.ptr[p0 + tid] - o0;
      pb1 = p.ptr[p0 + tid + 1] - o0;
    }
    __syncthreads();
    double cc[9], cam[6], da[6], kc[5], wl[3];
    // a robust loss scales A and B by w(s) of the residual at the current parameters, so the recomputed blocks need
    // the real measurement (K1's inputs, hence K1's w bit for bit); without the bit the measurement is 0 (e unused)
    constexpr bool MEAS = RECOMP && (LM & LENS_ROBUST) != 0;
    double2 m = make_double2(0.0, 0.0);
    const int fx = a < o1 ? fix_load<LM>(fm, i, j) : 0;
    if (RECOMP && a < o1) {
#pragma unroll
      for (int k = 0; k < 9; k++) cc[k] = p.camconst[9 * j + k];
      lens_load_kc<LM>(p.kc, j, kc);
      lens_load_w<LM>(p.wl, a, wl);
      if (MEAS) m = reinterpret_cast<const double2 *>(p.impts)[a];
#pragma unroll
      for (int k = 0; k < 6; k++) {
        cam[k] = p.cams[6 * j + k];
        da[k] = (fx & FIX_CAM) ? 0.0 : p.dp[6 * j + k];
      }
    }
    if (a < o1 && p.mode != 2) {
      double t0 = 0.0, t1 = 0.0, t2 = 0.0;
      if (RECOMP) {
        double M[3], e[2], A[12], B[6];
#pragma unroll
        for (int k = 0; k < 3; k++) M[k] = p.pts[3 * (size_t)i + k];
        lens_linearize<LM>(cc, cam, M, kc, wl, rl, m.x, m.y, e, A, B);
        fix_mask<LM>(fx, A, B);
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) {
          s0 += A[k] * da[k];
          s1 += A[6 + k] * da[k];
        }
        t0 = p.coeff * (B[0] * s0 + B[3] * s1);
        t1 = p.coeff * (B[1] * s0 + B[4] * s1);
        t2 = p.coeff * (B[2] * s0 + B[5] * s1);
      } else {
        const double *w = p.W + 18 * (size_t)a;
        const double *dw = p.dp + 6 * j;
#pragma unroll
        for (int k = 0; k < 6; k++) {
          const double dk = (fx & FIX_CAM) ? 0.0 : dw[k];
          t0 += w[3 * k] * dk;
          t1 += w[3 * k + 1] * dk;
          t2 += w[3 * k + 2] * dk;
        }
      }
      sT[tid][0] = t0;
      sT[tid][1] = t1;
      sT[tid][2] = t2;
    }
    __syncthreads();
    if (p0 + tid < p1) {
      const int ip = p0 + tid;
      const double *pv = p.PV + 9 * (size_t)ip;
      const int b0 = pb0, b1 = pb1;
      const double g0 = pv[6], g1 = pv[7], g2 = pv[8];
      double e0 = 0.0, e1 = 0.0, e2 = 0.0;
      for (int b = b0; b < b1; b++) {
        e0 += sT[b][0];
        e1 += sT[b][1];
        e2 += sT[b][2];
      }
      e0 = g0 - e0;
      e1 = g1 - e1;
      e2 = g2 - e2;
      if (DUMP) {
        p.dbg_eb[3 * (size_t)ip] = e0;
        p.dbg_eb[3 * (size_t)ip + 1] = e1;
        p.dbg_eb[3 * (size_t)ip + 2] = e2;
      }
      double v[6], vi[6];
#pragma unroll
      for (int k = 0; k < 6; k++) v[k] = pv[k];
      v[0] += p.mu;
      v[3] += p.mu;
      v[5] += p.mu;
      sym3_inverse(v, vi);
      // a fixed point: dpb_i = 0 and the proposal is the current point bit for bit (its W_ij^T dpa_j terms and g_b,i are
      // zero under the mask already; the select does not rely on it)
      const bool fp = fix_pt<LM>(fm, ip);
      const double d0 = fp ? 0.0 : vi[0] * e0 + vi[1] * e1 + vi[2] * e2;
      const double d1 = fp ? 0.0 : vi[1] * e0 + vi[3] * e1 + vi[4] * e2;
      const double d2 = fp ? 0.0 : vi[2] * e0 + vi[4] * e1 + vi[5] * e2;
      double *dpb = p.dp + p.nA + 3 * (size_t)ip;
      dpb[0] = d0;
      dpb[1] = d1;
      dpb[2] = d2;
      const double *M = p.pts + 3 * (size_t)ip;
      const double n0 = fp ? M[0] : M[0] + d0, n1 = fp ? M[1] : M[1] + d1, n2 = fp ? M[2] : M[2] + d2;
      double *np = p.newpts + 3 * (size_t)ip;
      np[0] = n0;
      np[1] = n1;
      np[2] = n2;
      sNP[tid][0] = n0;
      sNP[tid][1] = n1;
      sNP[tid][2] = n2;
      s_dp += d0 * d0 + d1 * d1 + d2 * d2;
      s_den += d0 * (p.mu * d0 + g0) + d1 * (p.mu * d1 + g1) + d2 * (p.mu * d2 + g2);
      s_np += n0 * n0 + n1 * n1 + n2 * n2;
    }
    __syncthreads();
    if (a < o1 && p.mode != 1) {
      double e0, e1;
      if (!RECOMP) {
#pragma unroll
        for (int k = 0; k < 9; k++) cc[k] = p.camconst[9 * j + k];
#pragma unroll
        for (int k = 0; k < 6; k++) cam[k] = (fx & FIX_CAM) ? p.cams[6 * j + k] : p.cams[6 * j + k] + p.dp[6 * j + k];
        lens_load_kc<LM>(p.kc, j, kc);
        lens_load_w<LM>(p.wl, a, wl);
      } else {
#pragma unroll
        for (int k = 0; k < 6; k++) cam[k] = (fx & FIX_CAM) ? cam[k] : cam[k] + da[k];
      }
      if (!MEAS) m = reinterpret_cast<const double2 *>(p.impts)[a];
      lens_residual<LM>(cc, cam, sNP[i - p0], kc, wl, m.x, m.y, e0, e1);
      s_cost += lens_cost<LM>(rl, e0, e1);
    }
    dsc = dn;
    i = j = 0;
    if (dsc.z + tid < dsc.w) {
      i = p.iidx[dsc.z + tid];
      j = p.jidx[dsc.z + tid];
    }
  }
  // workgroup reduction of the four sums, one atomic each
  double v4[4] = {s_dp, s_den, s_cost, s_np};
#pragma unroll
  for (int q = 0; q < 4; q++) {
    double v = v4[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((tid & 63) == 0) sRed[q][tid >> 6] = v;
  }
  __syncthreads();
  // one wave-instruction with four lanes: same-address atomics serialise at ~13 ns per
  // request, so the requests are spread over SC_NPART partial sets (summed on the host)
  if (tid < 4) {
    const double v = sRed[tid][0] + sRed[tid][1] + sRed[tid][2] + sRed[tid][3];
    atomicAdd(&p.scal[SC_PART + 4 * (blockIdx.x % SC_NPART) + tid], v);
  }
}

// A point seen by more than TILE_OBS cameras (compute_eb.cl:28-37 loops over all cameras): one
// workgroup walks its observations twice, TILE_OBS at a time -- sum of W_ij^T dpa_j (from the
// stored W), then dpb_i and the proposed point by one thread, then the residuals at the proposal.
template <bool DUMP, int LM>
__global__ __launch_bounds__(TILE_OBS) void k_backsub_long(BackArgs p, const int *long_pts, RobustLoss rl, FixedMask fm) {
  __shared__ double sRed[TILE_OBS / 64][4];
  __shared__ double sNP[3];
  const int tid = threadIdx.x, i = long_pts[blockIdx.x];
  const int o0 = p.ptr[i], o1 = p.ptr[i + 1];
  double t3[3] = {0.0, 0.0, 0.0};
  for (int a = o0 + tid; a < o1; a += TILE_OBS) {
    const double *w = p.W + 18 * (size_t)a;
    const double *dw = p.dp + 6 * (size_t)p.jidx[a];
    const bool fc = fix_cam<LM>(fm, p.jidx[a]);
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double dk = fc ? 0.0 : dw[k];
      t3[0] += w[3 * k] * dk;
      t3[1] += w[3 * k + 1] * dk;
      t3[2] += w[3 * k + 2] * dk;
    }
  }
#pragma unroll
  for (int q = 0; q < 3; q++) {
    double v = t3[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((tid & 63) == 0) sRed[tid >> 6][q] = v;
  }
  __syncthreads();
  double s_dp = 0.0, s_den = 0.0, s_cost = 0.0, s_np = 0.0;
  if (tid == 0) {
    const double *pv = p.PV + 9 * (size_t)i;
    double e[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      double v = 0.0;
      for (int w2 = 0; w2 < TILE_OBS / 64; w2++) v += sRed[w2][q];
      e[q] = pv[6 + q] - v;
      if (DUMP) p.dbg_eb[3 * (size_t)i + q] = e[q];
    }
    double v[6], vi[6];
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = pv[k];
    v[0] += p.mu;
    v[3] += p.mu;
    v[5] += p.mu;
    sym3_inverse(v, vi);
    const bool fp = fix_pt<LM>(fm, i);
    const double d[3] = {fp ? 0.0 : vi[0] * e[0] + vi[1] * e[1] + vi[2] * e[2], fp ? 0.0 : vi[1] * e[0] + vi[3] * e[1] + vi[4] * e[2],
                         fp ? 0.0 : vi[2] * e[0] + vi[4] * e[1] + vi[5] * e[2]};
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const double n = fp ? p.pts[3 * (size_t)i + q] : p.pts[3 * (size_t)i + q] + d[q];
      p.dp[p.nA + 3 * (size_t)i + q] = d[q];
      p.newpts[3 * (size_t)i + q] = n;
      sNP[q] = n;
      s_dp += d[q] * d[q];
      s_den += d[q] * (p.mu * d[q] + pv[6 + q]);
      s_np += n * n;
    }
  }
  __syncthreads();
  for (int a = o0 + tid; a < o1; a += TILE_OBS) {
    const int j = p.jidx[a];
    double cc[9], cam[6], e0, e1, kc[5], wl[3];
#pragma unroll
    for (int k = 0; k < 9; k++) cc[k] = p.camconst[9 * (size_t)j + k];
#pragma unroll
    for (int k = 0; k < 6; k++)
      cam[k] = fix_cam<LM>(fm, j) ? p.cams[6 * (size_t)j + k] : p.cams[6 * (size_t)j + k] + p.dp[6 * (size_t)j + k];
    lens_load_kc<LM>(p.kc, j, kc);
    lens_load_w<LM>(p.wl, a, wl);
    const double2 m = reinterpret_cast<const double2 *>(p.impts)[a];
    lens_residual<LM>(cc, cam, sNP, kc, wl, m.x, m.y, e0, e1);
    s_cost += lens_cost<LM>(rl, e0, e1);
  }
  __syncthreads();
  {
    double v = s_cost;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((tid & 63) == 0) sRed[tid >> 6][3] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double c = 0.0;
    for (int w2 = 0; w2 < TILE_OBS / 64; w2++) c += sRed[w2][3];
    double *dst = p.scal + SC_PART + 4 * (blockIdx.x % SC_NPART);
    atomicAdd(&dst[0], s_dp);
    atomicAdd(&dst[1], s_den);
    atomicAdd(&dst[2], c);
    atomicAdd(&dst[3], s_np);
  }
}

// the try's scalar block into pinned host memory: one small kernel instead of the runtime's
// 768-byte device-to-host copy (3.9 us on the stream in front of the linearization queued ahead)
// (the block, a fresh stamp and the check word, as the linearization queued ahead writes them: scal_publish.h -- the
// host waits for this route's event and does not need them, but the pinned block has one format)
__global__ __launch_bounds__(128) void k_publish_scal(const double *scal, double *host, double stamp) {
  scal_publish(scal, host, stamp);
}

int launch_publish_scal(psba_ctx *h, hipStream_t s) {
  h->pub_seq += 1.0;
  hipLaunchKernelGGL(k_publish_scal, dim3(1), dim3(128), 0, s, h->scal, h->h_scal_dev, h->pub_seq);
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

// psba_test_publish: nothing but the shared prologue, in a workgroup of 64, 128 or 256 threads
__global__ __launch_bounds__(256) void k_test_publish(const double *scal, double *host, double stamp) {
  scal_publish(scal, host, stamp);
}

int launch_test_publish(psba_ctx *h, int threads) {
  h->pub_seq += 1.0;
  hipLaunchKernelGGL(k_test_publish, dim3(1), dim3(threads), 0, h->stream, h->scal, h->h_scal_dev, h->pub_seq);
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

// Structure-only try (every camera fixed, psba_set_fixed): there is no coupled system, dpa = 0 and K3's point part is
// the whole solve, dpb_i = (V_i + mu I)^-1 g_b,i.  This kernel stands in for K2, the S-reduce and the factorization:
// it zeroes dpa and the try's partial sums, stamps the try (status[3]) and flags a singular V_i + mu I (status[0]) as
// K2 would have.
__global__ __launch_bounds__(256) void k_struct_only_begin(const double *PV, double mu, int nA, int nP, double *dp, double *scal,
                                                           int *status, int try_id) {
  const int gtid = blockIdx.x * blockDim.x + threadIdx.x, gsize = gridDim.x * blockDim.x;
  if (blockIdx.x == 0 && threadIdx.x < 4 * SC_NPART) scal[SC_PART + threadIdx.x] = 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 64) status[3] = try_id;
  for (int t = gtid; t < nA; t += gsize) dp[t] = 0.0;
  for (int i = gtid; i < nP; i += gsize) {
    double v[6], vi[6];
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = PV[9 * (size_t)i + k];
    v[0] += mu;
    v[3] += mu;
    v[5] += mu;
    if (sym3_inverse(v, vi)) status[0] = try_id;
  }
}

int launch_struct_only_try(psba_ctx *h, double mu) {
  h->try_id++;
  h->diag_done = false;
  h->packed_pending = false;
  int grid = (h->d.nP + 255) / 256;
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(k_struct_only_begin, dim3(grid), dim3(256), 0, h->stream, h->PV, mu, h->d.nA, h->d.nP, h->dp, h->scal,
                     h->status, h->try_id);
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

// K3 for lens model LM (psba_ctx::lens)
template <int LM>
static void enqueue_backsub(psba_ctx *h, const BackArgs &a, const RobustLoss &rl, const FixedMask &fm, int grid, bool dump, bool read_w) {
  if (dump && read_w)
    hipLaunchKernelGGL((k_backsub<true, false, LM>), dim3(grid), dim3(TILE_OBS), 0, h->stream, a, rl, fm);
  else if (dump)
    hipLaunchKernelGGL((k_backsub<true, true, LM>), dim3(grid), dim3(TILE_OBS), 0, h->stream, a, rl, fm);
  else if (read_w)
    hipLaunchKernelGGL((k_backsub<false, false, LM>), dim3(grid), dim3(TILE_OBS), 0, h->stream, a, rl, fm);
  else
    hipLaunchKernelGGL((k_backsub<false, true, LM>), dim3(grid), dim3(TILE_OBS), 0, h->stream, a, rl, fm);
  if (h->nLong) {  // points seen by more cameras than a tile holds
    if (dump)
      hipLaunchKernelGGL((k_backsub_long<true, LM>), dim3(h->nLong), dim3(TILE_OBS), 0, h->stream, a, h->long_pts, rl, fm);
    else
      hipLaunchKernelGGL((k_backsub_long<false, LM>), dim3(h->nLong), dim3(TILE_OBS), 0, h->stream, a, h->long_pts, rl, fm);
  }
}

int launch_backsub(psba_ctx *h, double mu, bool dump) {
  if (h->cnp != 6) return dump ? mirror_refused(h) : launch_backsub_free(h, mu);
  const Dims &d = h->d;
  BackArgs a;
  a.W = h->W;
  a.PV = h->PV;
  a.camconst = h->camconst;
  a.cams = h->cams[h->cur];
  a.pts = h->pts[h->cur];
  a.impts = h->impts;
  a.ga = h->ga;
  a.iidx = h->iidx;
  a.jidx = h->jidx;
  a.ptr = h->ptr;
  a.tile_desc = h->tile_desc;
  a.dp = h->dp;
  a.newcams = h->cams[1 - h->cur];
  a.newpts = h->pts[1 - h->cur];
  a.scal = h->scal;
  a.dbg_eb = h->dbg_eb;
  a.status = h->status;
  a.mu = mu;
  a.coeff = h->coeff_w;
  a.nC = d.nC;
  a.nA = d.nA;
  a.nTiles = d.nTiles;
  a.cam_terms = h->rank == 0 ? 1 : 0;
  a.kc = h->lens_kc;
  a.wl = h->lens_w;
  const RobustLoss rl = make_robust_loss(h->loss_kind, h->loss_c);
  {
    const char *m = getenv("PSBA_BACK_MODE");
    a.mode = m ? atoi(m) : 0;
  }
  // the fused path's accumulators are zeroed by this try's k_schur_reduce; the sba_func.h mirror
  // may run K3 more than once per assembly, so it zeroes them here
  if (dump) PSBA_HIP(h, hipMemsetAsync(h->scal + SC_PART, 0, 4 * SC_NPART * sizeof(double), h->stream));
  // persistent workgroups, three per CU (venice-shaped, 1350 tiles, K3 in us by grid: 512 18.7, 640 17.7,
  // 768 16.6, 896 18.8, 1024 18.2, 1350 17.8)
  int grid = d.nTiles < 768 ? d.nTiles : 768;
  if (const char *e = getenv("PSBA_BACK_GRID")) grid = atoi(e) > 0 && atoi(e) < grid ? atoi(e) : grid;
  {
    ProfScope ps(h, PSBA_K_BACKSUB);
    const bool read_w = getenv("PSBA_BACK_READ_W") != nullptr;
    const FixedMask fm = {h->fix_cams, h->fix_pts};
    lens_dispatch_fixed(h->lens, h->has_fixed, [&](auto m) { enqueue_backsub<decltype(m)::value>(h, a, rl, fm, grid, dump, read_w); });
  }
  PSBA_HIP(h, hipGetLastError());
  return PSBA_OK;
}

}  // namespace psba
