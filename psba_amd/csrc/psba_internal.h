// psba_internal.h -- the handle behind include/psba_hip.h and the kernel launch prototypes.
// Takes the place of PSBA_struct (reference PSBA/cl_psba.h:9-89) and the 31 cl_mem
// allocations of setup_cl (PSBA/cl_psba.cpp:40-84).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <string>
#include <vector>

#include "../../include/psba_hip.h"
#include "dev_buf.h"
#include "scal_publish.h"

namespace psba {

constexpr int TILE_OBS = 256;   // observations per point-aligned tile (= threads per workgroup)
constexpr int TILE_PTS = 128;   // points per tile (bounds the per-point LDS rows)
constexpr int MAX_GROUPS = 128; // row-aligned groups of the LDS-resident S partition (K2) are tried up to this count, then ranges of blocks
constexpr int CAM_ACC = 27;     // per-camera accumulators: 21 (sym U) + 6 (g_a)
constexpr int LEAN_REC = 20;    // doubles of an observation's record in the lean form: A (2 x 6) | B (2 x 3) | e (2); 160 bytes
constexpr int NSCAL = 104;      // device scalar block (doubles)
static_assert(NSCAL == PUB_WORDS, "scal_publish.h states the block's length");
constexpr int SC_NPART = 16;    // K3's four sums arrive in 16 partial sets (same-address atomics serialise)

// slots of the device scalar block
enum {
  SC_COST = 0,      // ||e||^2 of psba_residual
  SC_DP_L2 = 1,
  SC_GAIN_DEN = 2,
  SC_NEW_COST = 3,
  SC_NEWP_L2 = 4,
  SC_MAXDIAG = 7,
  // [8..9] alias the status words (ints)
  SC_PART = 16,      // K3: [SC_NPART][4] partial (dp_l2, gain_den, new_cost, newp_l2), summed on the host
  SC_STATUS_V = 80,  // K3: 1.0 when some V_i was singular in this try (summable over ranks)
  SC_STATUS_SPD = 81,  // K3: 1.0 when the Cholesky of this try failed
  SC_TR_DOTS = 84,     // trust-region operators: (Jx1.Jx1, Jx1.Jx2, Jx2.Jx2)
  SC_CHOLMOD = 88,     // modified Cholesky: lambda, delta, beta, block columns on the one-column route
  SC_SUMS = 96,        // psba_allreduce_scalars: up to 8 host scalars summed over the ranks
};

struct Dims {
  int nC = 0, nP = 0, nO = 0;
  int nA = 0, nB = 0, nT = 0;
  int nTiles = 0;     // tiles of the tile kernels (K1, K3): the long points' tiles are not among their descriptors
  int nTilesAll = 0;  // tiles of the contiguous partition tile_pt (incl. one per long point)
  int maxTrack = 0;
};

// one workgroup of k_schur_lds: a range of work items of one group of blocks
// item = (a - obs0) | (i - pt0) << 24 | (a - b) << 46 | position << 54: observation (24 bits), point
// (22 bits), distance to the partner observation of the same point (8 bits: a point has at most
// TILE_OBS = 256 observations), block position in the partition (10 bits)
constexpr int ITEM_OBS_BITS = 24, ITEM_PT_BITS = 22, ITEM_BOFF_BITS = 8, ITEM_POS_BITS = 10;
struct SchurWg {
  int group, nblk;      // group of blocks; blocks in its LDS partition
  int obs0, pt0;        // the items' observation / point numbers are relative to these
  long long item0, item1;
  unsigned long long slab_off;  // where this workgroup's partition goes in psba_ctx::slab
  long long itemD;      // [item0, itemD): pair items (one a-side, two partners, see PAIR_*_BITS); [itemD, item1): one product each
};
// a pair item: one observation a and its partners a - boff and a - boff + 1 of the same point (W_a, V*^-1, Y_a and
// the e_a terms are formed once for two products): a - obs0, i - pt0, boff >= 1, the two block positions
constexpr int PAIR_OBS_BITS = 18, PAIR_PT_BITS = 16;  // (+ ITEM_BOFF_BITS + 2 * ITEM_POS_BITS = 62 bits)
constexpr unsigned long long SCHUR_NULL_ITEM = ~0ull;
// what k_schur_reduce needs to know about the group a run of 16 partition positions belongs to
struct ReduceGroup {
  int nwg, nblk;            // slabs of the group, blocks in its partition
  long long pos0;           // first (global) position of the group
  unsigned long long slab;  // first double of the group's slabs
  unsigned long long pad;
};

// K2's route for many cameras (no LDS partition can hold a useful part of S): one thread per
// unit = (block of the lower block triangle, a segment of that block's product list); the
// thread accumulates its 6x6 (and, for a diagonal block, e_a) in registers.  Units are sorted
// by length; the 64 units of a wave read their products from an ELL-style table
// prod[(row0 + t) * 64 + lane] (-1 padded), so the list loads are coalesced.
struct OwnerWave {
  long long row0;  // first ELL row of this wave
  int len;         // rows (= longest unit of the wave)
  int pad;
};
struct OwnerUnit {
  int j, k;        // block (j, k), k <= j
  int multi;       // 1: the block has several units -> atomic adds into the zeroed S; 0: plain stores
  int slot;        // index of the block in the block-sparse list (psba_set_solver PSBA_SOLVER_PCG); -1: idle lane of the last wave
};
struct OwnerPlanHost {
  std::vector<int2> prod;          // (a, b) observation indices; a = -1: padding
  std::vector<OwnerWave> waves;
  std::vector<OwnerUnit> units;    // 64 per wave
  std::vector<int2> blocks;        // the non-empty blocks (j, k), k <= j, plus every diagonal block: canonical order
  std::vector<int> diag_slot;      // [nC] index of block (j, j) in `blocks`
  long long products = 0;
};
#ifdef PSBA_BUILD_EXPERIMENTS
// ---- K2 ring route (few cameras), an experiment of round 3 that lost: schur_ring_plan.cpp /
// kernels_schur_ring.hip, compiled only with PSBA_BUILD_EXPERIMENTS=1 (psba_amd/build.py) ----
constexpr int RING_LANES = 256;      // consumer lanes of a workgroup (4 waves); every lane owns one 6x6 block
constexpr int RING_MOVERS = 4;       // waves that stream W records into the LDS ring with LDS-DMA
constexpr int RING_PREPPERS = 4;     // waves that form Y_a = W_a V*^-1 (two lanes per job)
constexpr int RING_PREP_JOBS = 32;   // jobs per prepper wave and step
constexpr int RING_PAGE = 7;         // W records per page load at most: one LDS-DMA instruction moves up to 63 x 16 B, contiguous in W and in LDS
constexpr int RING_SLOTS = 992;      // 144-byte LDS slots in all: W records first, Y behind them
constexpr int RING_MAXOPS = 16;      // page loads per mover wave and step at most
constexpr unsigned RING_NULL_ENTRY = 0xFFFFFFFFu;
struct RingStep { int op_begin, op_end, job_begin, job_end; };  // the page loads and jobs of a step (relative to the workgroup's lists)
struct RingJob {
  int obs, point;   // the a-side observation and its point
  int slots;        // slot of W_a | Y slot << 16
  int earow;        // row (relative to the workgroup's first) whose e_a this job feeds, -1: not here
};
struct RingWg {
  int blk0, nblk;   // blocks [blk0, blk0 + nblk) of the canonical order tri(j) + k
  int row0, nrows;  // camera rows those blocks lie in
  int copy, nsteps; // which copy of the packed triangle the sums go to; steps (even)
  int nwslots, pad; // W slots of this workgroup's LDS; the Y slots follow them
  long long step0, ent0, op0, job0, lane0, bl0;  // first entry of this workgroup in the plan's lists
};
struct RingPlanHost {
  int nR = 0, nS = 0, nWg = 0, lat = 2;
  std::vector<int> rb;              // block range r = [rb[r], rb[r+1])
  std::vector<RingWg> wgs;          // range-major: index r * nS + s
  std::vector<RingStep> steps;
  std::vector<unsigned> entries;    // [step][RING_LANES]: partner slot | Y slot << 16, or RING_NULL_ENTRY
  std::vector<int> ops;             // [op][2]: first observation of the run of records, first slot | records << 16
  std::vector<RingJob> jobs;
  std::vector<int> lane_blk;        // [wg][RING_LANES] lane -> local block (-1: idle)
  std::vector<int> blk_lane0;       // [wg][nblk + 1] first lane of each local block
  long long products = 0, slots = 0, loaded_recs = 0;
};
#endif  // PSBA_BUILD_EXPERIMENTS
struct SchurPlanHost {
  std::vector<unsigned long long> items;
  std::vector<SchurWg> wgs;
  std::vector<int> blockpos;   // block (j,k) -> position in its group's partition
  std::vector<int> posblock;   // inverse, groups concatenated: (j << 16) | k, -1 = padding
  size_t slab_doubles = 0;
  long long real_items = 0;
  // runs layout (clustered tracks, see build_schur_plan): a workgroup's items as [turn][RUN_THREADS], every
  // thread's consecutive items grouped into runs of one block position; tasks = number of such runs
  bool runs = false;
  long long tasks = 0;
  long long pair_items = 0;  // rows layout: items that carry two products of one observation (SchurWg::itemD)
};
// ---- the camera blocks of 11 and 16 (free intrinsics, kernels_free.hip): the products Y_a W_b^T, b <= a of one
// point, sorted by block (j_a, j_b) of the lower block triangle and inside a block by point; every block's list cut
// into segments of at most seg_len products (one wave each).  blockprod_plan.cpp, host only
struct BlockProdPlanHost {
  std::vector<int2> blocks;  // (j, k), k <= j, ascending by (j, k): the blocks with at least one product
  std::vector<int4> segs;    // (block, first product, end product, partial tile or -1: the block's only segment)
  std::vector<int2> prods;   // (a, b) observation indices
  std::vector<int4> multi;   // the blocks with several segments: (j, k, first partial tile, tiles)
  int ntiles = 0;            // partial tiles (a camera block squared each)
  int seg_len = 0;
};
// the block-sparse S of these camera blocks (PSBA_SOLVER_SPARSE, kernels_free_pcg.hip): the plan's blocks plus a
// diagonal block for every camera without a product, ascending by (j, k), and the symmetric row walk of the product
struct BlockRowsHost {
  std::vector<int2> jk;        // the stored blocks
  std::vector<int> slot_of;    // [plan.blocks] slot of each of the plan's blocks in jk
  std::vector<int> diag_slot;  // [nC] slot of block (j, j)
  std::vector<char> added;     // [nC] 1: no product stores block (j, j)
  std::vector<int> rowptr;     // [nC + 1]
  std::vector<int2> rowent;    // (slot, other camera | how << 28), how as in bs_rowent; a row ascending by slot
  long long nadded = 0;
};
void build_block_rows(int nCams, const BlockProdPlanHost &plan, BlockRowsHost &out);  // blockprod_plan.cpp
constexpr int FBSR_ADDED = 1 << 30;  // flag in bs_diag on this route
constexpr int FPCG_CAP = 128;        // workgroups of the persistent grids = partial sums per inner product
inline int fpcg_vec_grid(int n) { return (n + 255) / 256 < FPCG_CAP ? (n + 255) / 256 : FPCG_CAP; }  // by unknowns
inline int fpcg_row_grid(int nC) { return (nC + 3) / 4 < FPCG_CAP ? (nC + 3) / 4 : FPCG_CAP; }       // by block rows, four a workgroup
constexpr int FCOVM_PANELS = 8;      // panels of 16 columns of a batch of psba_sparse_camera_covariance (kernels_free_pcg_many.hip)
constexpr int KD_UNIT = 64;        // observations of a camera unit on this route: one wave, one observation per lane
constexpr int KD_SEG_DEFAULT = 64; // products per segment (PSBA_FKD_SEG overrides)
constexpr int KD_RED = 4 * 520;    // doubles of the reduction scratch: camera terms | up to 512 workgroups x 4 sums
constexpr int RUN_THREADS = 512;  // threads of a workgroup of k_schur_lds_runs: 192 VGPRs with the 36 accumulators, two waves per SIMD (768 threads = 168 VGPRs spill 27 registers: 85 against 59 us)
constexpr int RUN_MAX = 32;       // products a lane sums in registers before it touches the LDS at the latest
}  // namespace psba

// ---- the handle's state, split by lifetime ----
// ProblemState: everything an upload creates or invalidates -- the problem's buffers and schedules, the settings that
// belong to a problem (lens model, loss, fixed blocks) and the state of the try in flight.  A new upload and
// psba_destroy replace it by a default-constructed one: its members release what they own and every scalar is back
// at its initial value.  A new per-problem field goes here, with its initial value, and nothing else has to be updated;
// a new derived-state flag (one that says "this was computed for the current model and parameters") is cleared in
// model_changed (problem_options.cpp), and nowhere else.
struct ProblemState {
  psba::Dims d;
  // ---- device memory ----
  psba::DevBuf<double> camconst;  // [nC][9]  K5 | q0(4)               (Kparas_buffer, initcams_buffer)
  psba::DevBuf<double> cams[2];   // [nC][6] cur / proposed            (cams_buffer, newCams_buffer)
  psba::DevBuf<double> pts[2];    // [nP][3] cur / proposed            (pts3D_buffer, newPts3D_buffer)
  psba::DevBuf<double> params0;   // [nT] the parameters as uploaded (psba_reset_params)
  psba::DevBuf<double> impts;     // [nO][2]                           (impts_buffer)
  // lens model (psba_set_distortion / psba_set_obs_covariance / psba_set_robust_loss; camera_model.h): the launch
  // sites pick the kernel instantiation from `lens` (bit 0 distortion, bit 1 covariances, bit 2 a robust loss other
  // than none); an upload resets it to none
  int lens = 0;
  int loss_kind = 0;            // PSBA_LOSS_* and its scale (whitened units)
  double loss_c = 1.0;
  psba::DevBuf<double> obs_s;    // [nO] psba_obs_sq_residuals' device output, allocated on first use
  psba::DevBuf<double> lens_kc;  // [nC][5] k1..k5, allocated while distortion is set
  psba::DevBuf<double> lens_w;   // [nO][4] (l00, l01, l11, 0): L^T L = Sigma^-1, allocated while covariances are set
  // fixed parameter blocks (psba_set_fixed; camera_model.h FixedMask): byte masks on the device, allocated while a
  // mask of that kind with a non-zero entry is set; an upload resets them to none.  has_fixed selects the LENS_FIXED
  // kernel instantiations at the launch sites (lens_dispatch_fixed); struct_only = every camera is fixed
  psba::DevBuf<unsigned char> fix_cams, fix_pts;  // [nC], [nP]
  int n_fix_cams = 0, n_fix_pts = 0;
  bool has_fixed = false, struct_only = false;
  bool try_shortcut = false;    // this try took the structure-only shortcut: nothing was assembled or factored
  psba::DevBuf<int> iidx;       // [nO] point of each observation    (iidx_buffer)
  psba::DevBuf<int> jidx;       // [nO] camera of each observation   (jidx_buffer)
  psba::DevBuf<int> ptr;        // [nP+1] point CSR over observations (replaces blkIdx_buffer)
  psba::DevBuf<int> tile_pt;    // [nTiles+1] first point of each tile
  psba::DevBuf<int> long_pts;   // [nLong] points seen by more than TILE_OBS cameras (tiles of their own, handled by the *_long kernels)
  int nLong = 0;
  psba::DevBuf<int4> tile_desc;  // [nTiles] (first point, end point, first observation, end observation): one load instead of a chain
  psba::DevBuf<double> W;        // [nO][18] W_ij = coeff A^T B        (W_buffer)
  psba::DevBuf<double> PV;       // [nP][9]  V_i sym6 | g_b,i          (V_buffer + g_buffer tail)
  psba::DevBuf<double> U;        // [nC][36]                           (U_buffer)
  psba::DevBuf<double> ga;       // [nA]                               (g_buffer head)
  // second set of linearization outputs, written by psba_linearize_ahead for the proposed
  // parameters while the host decides about the step; psba_accept swaps the sets
  psba::DevBuf<double> W_alt, PV_alt, U_alt, ga_alt;
  // the lean form of a linearization (psba_levmar's look-ahead linearizations on an eligible handle):
  // K1 stores one record (A | B | e) per observation instead of W, U and g_a, and K2 and its reduce form S, e_a and g_a
  // from the records.  A set written lean holds PV and R; its W and U are stale.  lean_ok: decided at upload (the
  // record buffers come with the first use, lean_prepare); lean_cur / lean_alt: the form of the current set and of the one queued ahead (written by
  // launch_linearize, swapped by psba_accept); lm_lean: the last psba_levmar queued lean linearizations
  psba::DevBuf<double> R, R_alt;  // [nO][LEAN_REC]
  bool lean_ok = false, lean_cur = false, lean_alt = false, lm_lean = false;
  bool ahead = false;           // the alternate set holds the linearization at the proposed parameters
  bool lin_is_ahead = false;    // the current set was computed ahead: the next psba_linearize is a no-op
  bool scal_side = false;       // side-stream work the main stream has not been ordered behind yet
  psba::DevBuf<double> campart;  // [nPart][nC][27] per-workgroup camera partial sums
  int nPart = 0;
  // many cameras (the 27 per-camera accumulators no longer fit a workgroup's LDS): K1 adds its
  // camera sums with global fp64 atomics into camacc [nC][27] (zeroed per launch) instead
  bool cam_global = false;
  psba::DevBuf<double> camacc;
  // ... and those sums are formed by a camera-major pass: thread = (camera, segment of its
  // observations), 27 sums in registers, one set of atomic adds per segment
  psba::DevBuf<int> cam_obs;     // [nO] observation indices sorted by camera (stable: points ascending)
  psba::DevBuf<int4> cam_units;  // [nCamUnits] (camera, first, end in cam_obs, 0)
  int nCamUnits = 0;
  // padded reduce buffer Lw[(n32+16)][n32], n32 = nA rounded up to 32: rows < nA = S (row stride
  // n32), rows nA..n32-1 identity padding, row n32 = ea, rows above zero (S_buffer, eab_buffer)
  psba::DevBuf<double> red;
  int n32 = 0;
  // K2 (schur) static schedule, built once per problem by schur_plan.cpp
  int nGroups = 0;              // groups of blocks (one LDS partition each); 0: the owner route
  int nWg = 0;                  // workgroups of k_schur_lds
  std::vector<int> gblk0;       // group g owns the blocks [gblk0[g], gblk0[g+1]) of the canonical order tri(j) + k
  std::vector<int> gnwg;        // workgroups (= slabs) of group g
  std::vector<int> gnblk;       // blocks in group g's LDS partition (padded to 16)
  std::vector<size_t> gslab;    // first double of group g's slabs
  psba::DevBuf<psba::ReduceGroup> gtab;  // for k_schur_reduce: one entry per run of 16 partition positions
  psba::DevBuf<psba::SchurWg> wg;        // [nWg] ordered by position in the point sequence
  psba::DevBuf<unsigned long long> items;  // work items, one per product Y_a W_b^T (or null)
  bool schur_runs = false;      // K2's items are in the runs layout (k_schur_lds_runs)
  bool schur_pairs = false;     // K2's item lists begin with pair items (SchurWg::itemD)
  // single rank: the K2 workgroups add their copies of the 21 blocks of the first 32x32 diagonal
  // block into diag0 (global atomics) while flushing, and one extra workgroup of the S-reduce
  // kernel factors that block -- the first step of the Cholesky chain off the critical path
  psba::DevBuf<double> redp;    // with a communicator: the packed sums (slab order, lower block triangle + e_a) that are all-reduced
  size_t packed_doubles = 0;
  bool packed_pending = false;  // this try's sums sit in redp, not yet in red
  psba::DevBuf<double> diag0;   // [21 * 36], zero between tries
  int h_diagpos[21] = {0};      // partition positions of the blocks (j, k), j <= 5
  int h_diaggrp[21] = {0};      // and their groups (-1: no such camera)
  bool diag_done = false;       // this try's S-reduce kernel has factored the first diagonal block
  bool cholmod_factor = false;  // chol_L holds the factor of the last dense psba_cholmod_lambda (psba_get_cholmod_factor)
  psba::DevBuf<int> posblock;   // per group, per partition position: (j << 16) | k of the block there, -1 = padding
  psba::DevBuf<double> slab;    // per workgroup: its group's partition, 36 doubles per position
  size_t packedN = 0;           // 36 * nC (nC+1) / 2 doubles: packed lower block triangle of S
  int ring_nWg = 0, ring_nS = 0;  // (workgroups of the experimental ring route; 0 in the product build)
#ifdef PSBA_BUILD_EXPERIMENTS
  // K2 ring route (few cameras): see RingPlanHost
  psba::DevBuf<psba::RingWg> ring_wg;
  psba::DevBuf<psba::RingStep> ring_steps;
  psba::DevBuf<unsigned> ring_entries;
  psba::DevBuf<int> ring_ops;
  psba::DevBuf<psba::RingJob> ring_jobs;
  psba::DevBuf<int> ring_bl0;
  psba::DevBuf<int> ring_canon;    // [tri(nC)] (j << 16) | k of every block of the canonical order
  psba::DevBuf<double> ring_slab;  // [ring_nS][packedN] copies of the packed triangle
  psba::DevBuf<double> ring_pvi;   // [nP][9] (V_i + mu I)^-1 (sym6) | (V_i + mu I)^-1 g_b,i of the current try (k_schur_vinv)
  long long ring_products = 0, ring_slots = 0;
  size_t ring_loaded_recs = 0;
  psba::DevBuf<long long> chol_tim_ring;  // dev instrumentation (PSBA_RING_TIMING): per-step s_memtime stamps of two workgroups
#endif
  // block-sparse S + preconditioned CG (psba_set_solver, kernels_pcg.hip)
  int pcg_iters = 0;
  double pcg_relres = 0.0;
  bool pcg_exhausted = false;   // the last solve used up max_iter without reaching tol
  long long bs_nblk = 0;
  psba::DevBuf<double> bs_val;  // [bs_nblk][cnp^2] | e_a [nA] right behind (one all-reduce)
  double *bs_ea = nullptr;      // = bs_val + cnp^2 bs_nblk (not owned)
  psba::DevBuf<int2> bs_jk;     // [bs_nblk] (j, k)
  psba::DevBuf<int> bs_diag;    // [nC] index of block (j, j) (PSBA_SOLVER_SPARSE on blocks of 11 / 16: | FBSR_ADDED where
                                // no product stores the block and k_fbsr_finalize writes it whole)
  // the full symmetric pattern by block row, for the product S p without atomics: row j's entries
  // [bs_rowptr[j], bs_rowptr[j + 1]) = (slot of the stored block, other camera | how to read it << 28:
  // 0 as stored (j is the block's row), 1 transposed (j is its column), 2 the diagonal block)
  psba::DevBuf<int> bs_rowptr;
  psba::DevBuf<int2> bs_rowent;
  psba::DevBuf<double> pcg_vec;   // r | z | p | q, nA each
  psba::DevBuf<double> pcg_minv;  // [nC][cnp^2] inverses of the diagonal blocks
  psba::DevBuf<double> pcg_scal;  // device scalars (their pinned mirror pcg_host lives with the handle)
  // psba_sparse_camera_covariance / psba_sparse_S_times_many (kernels_free_pcg_many.hip): buffers of their own,
  // allocated at first use -- the solve's dp, pcg_vec and pcg_scal are not touched
  psba::DevBuf<double> fcm_vec;   // [6][fcm_cap][nA][16] x | r | z | p | q | r's second buffer
  int fcm_cap = 0;                // panels fcm_vec holds (<= FCOVM_PANELS)
  psba::DevBuf<double> fcm_scal;  // [FCOVM_PANELS] scalar blocks of the panels | 16 doubles of k_fbsr_diag_inverse
  psba::DevBuf<int> fcm_status;   // [4] the status words k_fbsr_diag_inverse reports into
  psba::PinnedBuf<double> fcm_host;  // pinned mirror of the panels' scalars
  // K2 owner route (many cameras): see OwnerPlanHost
  psba::DevBuf<int2> own_prod;
  psba::DevBuf<psba::OwnerWave> own_waves;
  psba::DevBuf<psba::OwnerUnit> own_units;
  int own_nwaves = 0;
  long long own_products = 0;
  // the camera blocks of cnp = 11 and 16 (free intrinsics, kernels_free.hip): no floating-point atomics on this route
  psba::DevBuf<int> free_cuptr;      // [nC+1] the units cam_units[free_cuptr[j] .. free_cuptr[j+1]) of camera j
  psba::DevBuf<double> free_Be;      // [nO][8] B (2 x 3) | e of the linearization in flight (read by the per-point pass)
  psba::DevBuf<double> free_upart;   // [nCamUnits][cnp^2 + cnp] per-unit sums A^T A (cnp x cnp) | A^T e
  psba::DevBuf<double> free_Y;       // [nO][3 cnp] Y_a = W_a (V_i + mu I)^-1 of the try
  psba::DevBuf<double> free_eapart;  // [nCamUnits][cnp] per-unit sums Y_a g_b,i
  psba::DevBuf<int2> free_blocks, free_prods;  // BlockProdPlanHost on the device
  psba::DevBuf<int4> free_segs, free_multi;
  psba::DevBuf<double> free_tiles;   // [ntiles][cnp^2] partial tiles of the blocks with several segments
  int free_nsegs = 0, free_nmulti = 0;
  psba::DevBuf<double> free_red;     // [KD_RED] per-workgroup partial sums (cost; the try's four sums)
  // blocks of 16 only (the setters refuse the others, which so keep every intrinsic free and no groups)
  unsigned kd_mask = 0x3FFu;       // psba_set_intrinsics_mask: bit k set = intrinsic k is optimised
  // per-camera masks (psba_set_camera_masks): one word per camera, bit k set = the camera's row frees
  // intrinsic k; the free bits of camera j are kd_mask & kd_cmask[j].  Empty / null = no table (a table without a
  // zero entry is none): the kernels then read kd_mask alone, with no load; an upload resets to none
  std::vector<unsigned short> kd_cmask_h;
  psba::DevBuf<unsigned short> kd_cmask;  // [nC] kd_cmask_h on the device
  // shared intrinsics (psba_set_intrinsics_groups): empty / null = no grouping, the ungrouped launches
  std::vector<int> kd_rep_h;       // [nC] representative (lowest member) of each camera's group; empty: none
  int kd_ngroups = 0;              // groups in all (singletons included) while kd_rep_h is set
  psba::DevBuf<int> kd_rep;        // [nC] kd_rep_h on the device
  psba::DevBuf<int> kd_gidx;       // [nC] index of the camera's group among those with several members, -1: alone
  psba::DevBuf<int> kd_gptr;       // [kd_nmg + 1] CSR over kd_gmem of the groups with several members
  psba::DevBuf<int> kd_gmem;       // their members in ascending camera order (the first is the representative)
  int kd_nmg = 0;
  // ... under PSBA_SOLVER_SPARSE (psba_set_sparse_intrinsics_groups; kernels_free_pcg.hip): the list keeps the
  // unfolded, undamped blocks and the solve folds -- the folded diagonal blocks of the preconditioner are built into
  // buffers of their own, allocated with the tables
  int kd_nmem = 0;                 // entries of kd_gmem
  psba::DevBuf<double> fg_part;    // [kd_nmem][10][16] each member's share of the intrinsic rows of its group's folded block
  psba::DevBuf<double> fg_blk;     // [kd_nmg][256] the folded diagonal block of each representative, mu D added
  double bs_mu = 0.0;              // mu and D (null: I) of the last k_fbsr_finalize: what the grouped solve adds after the fold
  const double *bs_D = nullptr;    // (not owned)
  bool precond_ok = false;         // pcg_minv holds the block inverses of the last psba_schur_solve (psba_get_sparse_precond)
  // held poses and points of this route (psba_set_held): byte masks on the device, both allocated while
  // either has a non-zero entry (has_held: the HELD kernel instantiations), none otherwise; an upload resets to none
  psba::DevBuf<unsigned char> held_poses, held_pts;  // [nC], [nP]
  int n_held_poses = 0, n_held_pts = 0;
  bool has_held = false;
  // Gaussian priors of this route (psba_set_priors), compacted: the record of each block (-1: no prior),
  // the records mean | information of the blocks that have one, and the list of those blocks.  All six are allocated
  // while any block has a prior (has_prior: the PRIOR kernel instantiations), none otherwise; an upload resets to none
  psba::DevBuf<int> prior_cidx, prior_pidx;      // [nC], [nP]
  psba::DevBuf<int> prior_clist, prior_plist;    // [n_cam_priors], [n_pt_priors] (at least one element)
  psba::DevBuf<double> prior_crec, prior_prec;   // [n_cam_priors][cnp + cnp^2], [n_pt_priors][12]
  psba::DevBuf<double> prior_out;                // [2] psba_prior_cost's device output, allocated on first use
  int n_cam_priors = 0, n_pt_priors = 0;
  bool has_prior = false;
  // observation weighting of this route (psba_set_obs_weighting): a loss (kind, scale) and 1 / sigma per
  // observation.  has_weighting (the WGT kernel instantiations) = a loss other than none or sigmas; the table is then
  // allocated (ones when only a loss is set), none otherwise; an upload resets to (none, 1, no sigmas)
  int wgt_kind = 0;
  double wgt_c = 1.0;
  bool wgt_sigma = false, has_weighting = false;
  psba::DevBuf<double> obs_isig;   // [nO] 1 / sigma_a
  psba::DevBuf<double> obs_sw;     // [2 nO] psba_get_obs_weights' device output s | w, allocated on first use
  // the damping rule of this route (psba_set_damping): N + mu I, or N + mu D with Marquardt's
  // D_k = min(max(N_kk, dmin), dmax).  damp_D [nT] belongs to the current linearization, damp_D_alt to the one queued
  // ahead (psba_accept swaps them with the rest); both are allocated by the first switch to Marquardt
  int damp_kind = PSBA_DAMPING_IDENTITY;
  double damp_dmin = 1e-6, damp_dmax = 1e32;
  psba::DevBuf<double> damp_D, damp_D_alt;
  bool damp_ok = false;           // damp_D is that of the current parameters and model (psba_get_damping_diag)
  psba::DevBuf<double> dp;        // [nT] dpa | dpb                     (dp_buffer)
  psba::DevBuf<double> trv[2];    // [nT] each: vectors of the trust-region operators (allocated on first use)
  psba::DevBuf<double> jmul_out;  // [2 nO] J x of psba_compute_Jmultiply (allocated on first use)
  psba::GraphExec chol_graph[2];  // captured panel chain of kernels_chol_graph.hip, with / without its first step
  int chol_graph_n32[2] = {0, 0};
  double *chol_graph_red[2] = {nullptr, nullptr};  // (the reduce buffer the graph was captured for: compared, not owned)
  psba::DevBuf<long long> chol_tim;  // dev instrumentation: per-phase s_memtime ticks of the last solve (PSBA_CHOL_TIMING)
  psba::DevBuf<double> chol_L;    // [(2 n32+16)][n32] panel chain: the Cholesky factor | forward-solved e_a row | L^-T
  psba::DevBuf<double> dist_buf;  // sharded factorization: packed column blocks of one super-panel (allocated on first use)
  psba::DevBuf<double> chol_ws;   // [ceil(nA/32)][32*32] inverses of the diagonal blocks of L (diagBlkAux_buffer)
  // covariance of the estimate (psba_covariance_compute and psba_free_covariance_compute; covariance.cpp,
  // kernels_cov.hip): one set of workspaces for every camera block, allocated on first use.  A handle
  // has one camera model for its life, so one pair of flags serves both verb families; each family's getters refuse
  // the other's handle by its camera block (cnp).  Y_ij of the points is cov_Y for blocks of 6, the route's free_Y else
  psba::DevBuf<double> cov_A;         // [n32][n32] over one compute: compacted S -> its Cholesky factor -> C_aa, the result
  psba::DevBuf<double> cov_X;         // [n32][n32] the lower triangle of the inverse (read by the finish alone)
  psba::DevBuf<int> cov_src;          // [nA] -1 fixed, masked or held | itself: live | the representative's coordinate: folded away
  psba::DevBuf<double> cov_dinv;      // [n32 / 16][256] inverses of the factor's diagonal tiles
  psba::DevBuf<double> cov_Y;         // [nO][18]
  psba::DevBuf<double> cov_pts;       // [nP][9]
  psba::DevBuf<int> cov_status;       // [2] not SPD, singular V
  bool cov_ok = false;                // cov_A is the camera covariance of the current parameters and model
  bool cov_pts_ok = false;            // ... and cov_pts the point blocks (not after reassemble = 0)
  double cov_ms[3] = {0.0, 0.0, 0.0}; // factor, inverse, points of the last compute (psba_covariance_times)
  // debug dumps for the sba_func.h mirror (allocated on first use)
  psba::DevBuf<double> dbg_ex, dbg_JA, dbg_JB, dbg_Y, dbg_Vinv, dbg_eb;

  // ---- state ----
  bool uploaded = false, linearized = false, assembled = false, solved = false, backsubbed = false;
  bool backsub_pending = false;  // psba_backsub_async issued, psba_backsub_wait not yet
  // free intrinsics: W and free_Be hold the blocks of one linearization at the current parameters
  // (psba_get_free_obs_blocks); a linearization queued ahead writes W_alt but the same free_Be
  bool free_obs = false;
  // the try's scalars travel to the host with the linearization queued ahead (its workgroup 0 copies
  // them and then writes a stamp the host polls) instead of through a kernel of their own between K3
  // and that linearization: publish_deferred = K3 queued, nothing published yet; publish_in_k1 = the
  // queued K1 carries them, the host takes the block once it carries the stamp pub_seq and its own check word
  // (scal_publish.h)
  bool publish_deferred = false, publish_in_k1 = false;
  int cur = 0;                  // index of the current parameter set in cams[]/pts[]
  double coeff = 1.0, coeff_g = 1.0, mu = 0.0;
  double coeff_w = 1.0;         // the coefficient the stored W was formed with (last K1 launch)
  bool mu_applied = false;      // update_UV called (fine-grained mirror only)
};

// what lives as long as the handle: the device and its streams and events, the scalar blocks, the communicator, the
// settings made before an upload (solver, camera block, block pattern), per-device flags, profiling -- and the
// generation stamps try_id and pub_seq, which are compared with device and pinned words that are never zeroed (a stamp
// that started again at zero would match a stale word)
struct psba_ctx : ProblemState {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  // multi-GPU
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;

  double *h_scal_dev = nullptr;     // device address of the pinned host block h_scal
  hipEvent_t scal_event = nullptr;  // recorded behind the scalar copy of psba_backsub_async
  hipStream_t stream2 = nullptr;    // with a communicator: the try's scalar all-reduce + copy run here
  hipEvent_t k3_event = nullptr;    // K3 done (main stream) -> side stream
  hipStream_t chol_side = nullptr;      // lowest-priority stream of the far updates (look-ahead of the blocked chain)
  std::vector<hipEvent_t> chol_events;  // the look-ahead of the blocked Cholesky chain (two per super-panel)

  int solver = 0;               // PSBA_SOLVER_* (block-sparse S + preconditioned CG: psba_set_solver, kernels_pcg.hip)
  // PSBA_SOLVER_SPARSE was asked for: stored as PSBA_SOLVER_PCG (with six-parameter blocks it is that mode), and on
  // blocks of 11 / 16 the upload takes the route of kernels_free_pcg.hip instead of refusing
  bool sparse_any_block = false;
  int cnp = 6;  // parameters per camera: 6 (fixed intrinsics, the reference's kernels), 11 (psba_set_camera_model: free intrinsics) or 16 (free intrinsics and distortion)
  double pcg_tol = 1e-10;
  int pcg_maxit = 500;
  psba::PinnedBuf<double> pcg_host;       // pinned mirror of the PCG's device scalars (allocated by the first PCG upload)
  std::vector<unsigned char> bs_pattern;  // sharded points without a communicator: the union of all ranks' blocks (psba_set_sparse_pattern)

  psba::DevBuf<double> scal;    // [NSCAL]
  // [4] generation stamps, never zeroed: [0] == try_id <=> some V_i singular in this try,
  // [1] == try_id <=> the Cholesky of this try failed; [3] = try_id as seen by the graph-replayed
  // Cholesky kernels (written by the K2 reduce kernel).  Lives in scal[8..9]
  int *status = nullptr;
  int try_id = 0;
  double pub_seq = 0.0;         // stamp of the last block a kernel published (scal_publish.h): h_scal[PUB_STAMP]
  psba::PinnedBuf<double> h_scal;  // pinned mirror of scal, then the stamp and the check word (PUB_RAW of NSCAL + 8 words)
  // psba_publish_stats: blocks psba_backsub_wait accepted from the linearization queued ahead, and tries among them
  // that met a torn reading (the wanted stamp over a block that fails its check) before
  long long pub_takes = 0, pub_torn = 0;
  int *h_status = nullptr;      // pinned mirror of status

  // kernels whose dynamic LDS exceeds 64 KiB need hipFuncSetAttribute once per device: kept per
  // handle (one handle = one device), not per process
  bool lds_attr_set = false, atomic_attr_set = false, chol_attr_set = false, lin_attr_set = false, ring_attr_set = false;

  // ---- profiling ----
  unsigned prof = 0;            // bit k set: time kernel class k with HIP events
  struct Span { hipEvent_t a, b; int kind; };
  std::vector<Span> spans;
  size_t spans_used = 0;
  double prof_ms[PSBA_K_COUNT] = {0};
  int prof_n[PSBA_K_COUNT] = {0};
};

namespace psba {

// error helpers (psba_api.cpp)
int fail(psba_ctx *h, int code, const char *fmt, ...);
// the lean form of the linearization, for psba_levmar (psba_api.cpp): may this handle take it now; psba_linearize_ahead
// in either form; and, before psba_levmar returns, a standard linearization in the place of every lean one a later
// verb could still reach
bool lean_eligible(psba_ctx *h);
bool lean_prepare(psba_ctx *h);  // lean_eligible, with the record buffers allocated on first use
int linearize_ahead(psba_ctx *h, bool lean);
int lean_restore(psba_ctx *h);
#define PSBA_HIP(h, call)                                                              \
  do {                                                                                 \
    hipError_t e__ = (call);                                                           \
    if (e__ != hipSuccess)                                                             \
      return psba::fail((h), PSBA_E_HIP, "%s failed: %s (%s:%d)", #call,               \
                        hipGetErrorString(e__), __FILE__, __LINE__);                   \
  } while (0)

struct ProfScope {
  psba_ctx *h;
  int idx = -1;
  ProfScope(psba_ctx *h, int kind);
  ~ProfScope();
};

// ---- kernel launchers (one per .hip file) ----
// kernels_linearize.hip
int launch_linearize(psba_ctx *h, bool dump, bool ahead = false, bool publish = false, bool lean = false);
int launch_residual(psba_ctx *h, int which, double *ex_out_dev, double *s_out_dev = nullptr);
int launch_max_diag(psba_ctx *h);
// kernels_schur.hip
int build_schur_plan(psba_ctx *h, int nCams, int nPts, int nObs, const int *iidx, const int *jidx,
                     const int *ptr, SchurPlanHost &out);
int build_owner_plan(int nCams, int nObs, const int *iidx, const int *jidx, const int *ptr, OwnerPlanHost &out,
                     const unsigned char *pattern = nullptr);
int sparse_pattern(int nCams, int nObs, const int *iidx, const int *jidx, const int *ptr, unsigned char *flags);
#ifdef PSBA_BUILD_EXPERIMENTS
int build_ring_plan(int nCams, int nPts, int nObs, const int *iidx, const int *jidx, const int *ptr, RingPlanHost &out,
                    bool force = false);
int launch_schur_ring(psba_ctx *h, double mu, bool dump);
struct SchurLdsArgs;
bool launch_schur_lds_mode(int mode, dim3 G, dim3 B, size_t lds, hipStream_t s, const SchurLdsArgs &a);  // kernels_schur_modes.hip
#endif
int launch_schur(psba_ctx *h, double mu, bool dump);
int launch_schur_expand(psba_ctx *h);
// kernels_chol.hip
int launch_chol_solve(psba_ctx *h);
int mirror_refused(psba_ctx *h);  // the sba_func.h mirror (dumps, per-observation outputs) asked of a block wider than 6
// kernels_free.hip: the camera blocks of 11 and 16 (free intrinsics; with distortion), MFMA sums in fixed order
int build_blockprod_plan(int nCams, int nObs, const int *iidx, const int *jidx, const int *ptr, int seg_len,
                         BlockProdPlanHost &out);  // blockprod_plan.cpp
int launch_linearize_free(psba_ctx *h, bool ahead, bool publish);
int launch_residual_free(psba_ctx *h, int which);
int launch_obs_weights_free(psba_ctx *h, int which, double *s_dev, double *w_dev);
int launch_prior_cost_free(psba_ctx *h, int which, double *out2_dev);
int launch_max_diag_free(psba_ctx *h);
int launch_schur_free(psba_ctx *h, double mu);
int launch_backsub_free(psba_ctx *h, double mu);
// kernels_pcg.hip
int launch_bsr_finalize(psba_ctx *h, double mu);
int launch_pcg_solve(psba_ctx *h);
int launch_bsr_gershgorin(psba_ctx *h, double *lambda, double *info3);
int launch_bsr_times(psba_ctx *h, const double *x_host, double *y_host);
// the same three on blocks of 11 / 16 (kernels_free_pcg.hip)
int launch_fbsr_finalize(psba_ctx *h, double mu, const double *D);
int launch_fpcg_solve(psba_ctx *h);
int launch_fbsr_times(psba_ctx *h, const double *x_host, double *y_host);
int launch_fbsr_diag_inverse(psba_ctx *h, double *minv, double *pc, int *status, int stamp);
int launch_fbsr_times_many(psba_ctx *h, int n_panels, const double *X, double *Y);  // kernels_free_pcg_many.hip
int launch_fcovm_compute(psba_ctx *h, double scale, int n_sel, const int *sel, double *C, double *cols, int *iters, double *relres);
int launch_fcovp_compute(psba_ctx *h, double mu, double scale, int n_sel, const int *sel, double *C, double *cols, int *iters,
                         double *relres);  // kernels_free_pcg_points.hip
// kernels_chol_graph.hip
int launch_chol_graph(psba_ctx *h);
int chol_dist_shape(psba_ctx *h, int *NB, int *blocked);
int chol_shape(psba_ctx *h, int *out8);
int chol_dist_exchange_plan(int n32, int NB, int nranks, int JE, long long (*out)[4], int cap);
int chol_dist_begin(psba_ctx *h);
int chol_dist_superpanel(psba_ctx *h, int J);
int chol_dist_block(psba_ctx *h, int B, double *buf_dev, int set);
int chol_dist_finish(psba_ctx *h);
// kernels_backsub.hip
int launch_backsub(psba_ctx *h, double mu, bool dump);
int launch_publish_scal(psba_ctx *h, hipStream_t s);
int launch_test_publish(psba_ctx *h, int threads);
int launch_struct_only_try(psba_ctx *h, double mu);
// kernels_cov.hip
int launch_cov_cameras(psba_ctx *h, double scale, hipEvent_t *ev);
int launch_cov_points(psba_ctx *h, double mu, double scale);
int launch_cov_gather(psba_ctx *h, const int2 *pairs_dev, int n_pairs, double *out_dev);
int launch_fcov_sigmas(psba_ctx *h, double *sigma_dev);
// kernels_tr.hip
int launch_jmul(psba_ctx *h, const double *x1_dev, const double *x2_dev, double *out1_dev, double *dots_dev);
int launch_pack_g(psba_ctx *h, double *g_dev);
int launch_newp(psba_ctx *h, double *dp_dev);
int launch_cholmod(psba_ctx *h, double *out4_dev);

}  // namespace psba
