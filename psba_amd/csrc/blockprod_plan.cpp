// blockprod_plan.cpp -- the S-assembly schedule of the free-intrinsics camera blocks (kernels_free.hip),
// built once per upload on the host: every product Y_a W_b^T (b <= a, both observations of one point) belongs to the
// block (camera of a, camera of b) of the lower block triangle.  The products are sorted by block, inside a block by
// point (the order the sums are formed in: fixed by the problem, not by the run), and every block's list is cut into
// segments of at most seg_len products -- one wave each; a block with several segments is summed from partial tiles
// in segment order.  Also the host-only test hook psba_blockprod_plan_*.
#include <algorithm>
#include <new>

#include "psba_internal.h"

namespace psba {

int build_blockprod_plan(int nCams, int nObs, const int *iidx, const int *jidx, const int *ptr, int seg_len,
                         BlockProdPlanHost &out) {
  if (seg_len < 1) seg_len = 1;
  out = BlockProdPlanHost();
  out.seg_len = seg_len;
  struct Rec {
    long long block;  // j * nCams + k: ascending = ascending (j, k)
    int a, b;
  };
  std::vector<Rec> recs;
  long long total = 0;
  for (int a = 0; a < nObs; a++) total += a - ptr[iidx[a]] + 1;
  if (total > 0x7fffffffLL) return PSBA_E_INVALID;  // the segments index the list with ints
  recs.reserve((size_t)total);
  // point-major input with ascending cameras inside a point: this enumeration is ascending by point, and b <= a means
  // camera(b) <= camera(a)
  for (int a = 0; a < nObs; a++)
    for (int b = ptr[iidx[a]]; b <= a; b++) recs.push_back(Rec{(long long)jidx[a] * nCams + jidx[b], a, b});
  std::stable_sort(recs.begin(), recs.end(), [](const Rec &x, const Rec &y) { return x.block < y.block; });
  out.prods.resize(recs.size());
  for (size_t t = 0; t < recs.size(); t++) out.prods[t] = make_int2(recs[t].a, recs[t].b);
  for (size_t f = 0; f < recs.size();) {
    size_t e = f;
    while (e < recs.size() && recs[e].block == recs[f].block) e++;
    const int blk = (int)out.blocks.size();
    const int j = (int)(recs[f].block / nCams), k = (int)(recs[f].block % nCams);
    out.blocks.push_back(make_int2(j, k));
    const int nseg = (int)((e - f + (size_t)seg_len - 1) / (size_t)seg_len);
    if (nseg > 1) out.multi.push_back(make_int4(j, k, out.ntiles, nseg));
    for (int s = 0; s < nseg; s++) {
      const size_t s0 = f + (size_t)s * seg_len, s1 = std::min(e, s0 + (size_t)seg_len);
      out.segs.push_back(make_int4(blk, (int)s0, (int)s1, nseg > 1 ? out.ntiles++ : -1));
    }
    f = e;
  }
  return PSBA_OK;
}

// the stored blocks of the block-sparse S: a merge of the plan's blocks (ascending) with the diagonal of every camera;
// then the row walk as upload_bsr_rows builds it for the blocks of 6 -- a block serves its row as stored and its
// column's row transposed, a diagonal block through its lower triangle; a row's entries ascend by slot
void build_block_rows(int nCams, const BlockProdPlanHost &plan, BlockRowsHost &out) {
  out = BlockRowsHost();
  out.diag_slot.assign((size_t)nCams, -1);
  out.added.assign((size_t)nCams, 0);
  out.slot_of.resize(plan.blocks.size());
  size_t b = 0;
  for (int j = 0; j < nCams; j++) {
    for (; b < plan.blocks.size() && plan.blocks[b].x == j; b++) {  // row j of the lower triangle ends with (j, j)
      if (plan.blocks[b].y == j) out.diag_slot[(size_t)j] = (int)out.jk.size();
      out.slot_of[b] = (int)out.jk.size();
      out.jk.push_back(plan.blocks[b]);
    }
    if (out.diag_slot[(size_t)j] < 0) {
      out.diag_slot[(size_t)j] = (int)out.jk.size();
      out.added[(size_t)j] = 1;
      out.nadded++;
      out.jk.push_back(make_int2(j, j));
    }
  }
  out.rowptr.assign((size_t)nCams + 1, 0);
  for (const int2 &e : out.jk) {
    out.rowptr[(size_t)e.x + 1]++;
    if (e.x != e.y) out.rowptr[(size_t)e.y + 1]++;
  }
  for (int j = 0; j < nCams; j++) out.rowptr[(size_t)j + 1] += out.rowptr[(size_t)j];
  out.rowent.resize((size_t)out.rowptr[(size_t)nCams]);
  std::vector<int> at(out.rowptr.begin(), out.rowptr.end() - 1);
  for (size_t sl = 0; sl < out.jk.size(); sl++) {
    const int2 e = out.jk[sl];
    if (e.x == e.y) {
      out.rowent[(size_t)at[(size_t)e.x]++] = make_int2((int)sl, e.x | (2 << 28));
    } else {
      out.rowent[(size_t)at[(size_t)e.x]++] = make_int2((int)sl, e.y);
      out.rowent[(size_t)at[(size_t)e.y]++] = make_int2((int)sl, e.x | (1 << 28));
    }
  }
}

}  // namespace psba

struct psba_blockprod_plan {
  psba::BlockProdPlanHost plan;
  psba::BlockRowsHost rows;
};

extern "C" {

psba_blockprod_plan_t psba_blockprod_plan_create(int nCams, int n3Dpts, int n2Dprojs, const int *iidx, const int *jidx,
                                                 int seg_len) {
  if (nCams <= 0 || n3Dpts <= 0 || n2Dprojs <= 0 || !iidx || !jidx || seg_len < 1) return nullptr;
  std::vector<int> ptr((size_t)n3Dpts + 1, 0);
  for (int a = 0; a < n2Dprojs; a++) {
    if (iidx[a] < 0 || iidx[a] >= n3Dpts || jidx[a] < 0 || jidx[a] >= nCams) return nullptr;
    // point-major, cameras ascending inside a point, as psba_upload_problem requires
    if (a && (iidx[a] < iidx[a - 1] || (iidx[a] == iidx[a - 1] && jidx[a] <= jidx[a - 1]))) return nullptr;
    ptr[(size_t)iidx[a] + 1]++;
  }
  for (int i = 0; i < n3Dpts; i++) ptr[(size_t)i + 1] += ptr[i];
  psba_blockprod_plan *p = new (std::nothrow) psba_blockprod_plan;
  if (!p) return nullptr;
  if (psba::build_blockprod_plan(nCams, n2Dprojs, iidx, jidx, ptr.data(), seg_len, p->plan) != PSBA_OK) {
    delete p;
    return nullptr;
  }
  psba::build_block_rows(nCams, p->plan, p->rows);
  return p;
}

int psba_blockprod_plan_rows_info(psba_blockprod_plan_t p, long long info[3]) {
  if (!p || !info) return PSBA_E_INVALID;
  info[0] = (long long)p->rows.jk.size();
  info[1] = p->rows.nadded;
  info[2] = (long long)p->rows.rowent.size();
  return PSBA_OK;
}

int psba_blockprod_plan_rows(psba_blockprod_plan_t p, int *jk, int *diag_slot, int *rowptr, int *rowent) {
  if (!p) return PSBA_E_INVALID;
  const psba::BlockRowsHost &r = p->rows;
  if (jk)
    for (size_t b = 0; b < r.jk.size(); b++) {
      jk[2 * b] = r.jk[b].x;
      jk[2 * b + 1] = r.jk[b].y;
    }
  if (diag_slot) std::copy(r.diag_slot.begin(), r.diag_slot.end(), diag_slot);
  if (rowptr) std::copy(r.rowptr.begin(), r.rowptr.end(), rowptr);
  if (rowent)
    for (size_t e = 0; e < r.rowent.size(); e++) {
      rowent[2 * e] = r.rowent[e].x;
      rowent[2 * e + 1] = r.rowent[e].y;
    }
  return PSBA_OK;
}

int psba_blockprod_plan_info(psba_blockprod_plan_t p, long long info[4]) {
  if (!p || !info) return PSBA_E_INVALID;
  info[0] = (long long)p->plan.blocks.size();
  info[1] = (long long)p->plan.segs.size();
  info[2] = (long long)p->plan.prods.size();
  info[3] = p->plan.ntiles;
  return PSBA_OK;
}

int psba_blockprod_plan_copy(psba_blockprod_plan_t p, int *blocks, int *segs, int *prods) {
  if (!p) return PSBA_E_INVALID;
  if (blocks)
    for (size_t b = 0; b < p->plan.blocks.size(); b++) {
      blocks[2 * b] = p->plan.blocks[b].x;
      blocks[2 * b + 1] = p->plan.blocks[b].y;
    }
  if (segs)
    for (size_t s = 0; s < p->plan.segs.size(); s++) {
      segs[3 * s] = p->plan.segs[s].x;
      segs[3 * s + 1] = p->plan.segs[s].y;
      segs[3 * s + 2] = p->plan.segs[s].z;
    }
  if (prods)
    for (size_t t = 0; t < p->plan.prods.size(); t++) {
      prods[2 * t] = p->plan.prods[t].x;
      prods[2 * t + 1] = p->plan.prods[t].y;
    }
  return PSBA_OK;
}

void psba_blockprod_plan_destroy(psba_blockprod_plan_t p) { delete p; }

}  // extern "C"
