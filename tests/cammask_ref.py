"""Host reference of the per-camera intrinsics masks on the 16-block route (psba_set_camera_masks; no GPU):
tests/test_cammask_ref.py applies it to plain fp64 evaluations and injected faults, tests/test_gpu_camera_masks.py to
the kernels.

Model.  table [nC, 10], row j = camera j, order (fu, u0, v0, ar, s, k1..k5), non-zero = optimised.  Intrinsic k of
camera j is optimised iff the global mask frees k AND row j frees k.  A coordinate that is not optimised is one more
held coordinate of the embedded system (held_ref.py's statement): its column of A is zero, the placeholder coeff is on
the diagonal, g, e_a and dp are exactly 0 there, the maximum of the diagonal skips it, the proposal carries the current
bits.  A camera with no free intrinsic and a held pose is a wholly fixed camera; nothing more is needed for one.

_CamMask is a mixin in the manner of held_ref._Held and sits in front of it: it zeroes the masked columns of A per
observation by j and extends `held` by the masked coordinates BEFORE the holds, the priors and the weighting derive
their own tables from it (held_all, free_all, free_c), so every judge of free_ref, shared_ref, held_ref, prior_ref,
weight_ref and freecov_ref applies unchanged with its own constants.  CamMaskRoute is weight_ref.WeightRoute with the
table (no priors and no weighting by default: those layers are then the identity); CamMaskSharedRoute is
held_ref.HeldSharedRoute with a table that is constant on every group.

Groups.  A coordinate masked for a group is masked on every member: it is not shared, not summed and not folded away,
so phi, away and keep are restated per camera here.  shared_ref.fold and fold_bound take (rep, free) and build the map
of the global mask, which would sum the members' placeholders of such a coordinate into n_g coeff at the
representative; fold() and fold_bound() below are the same sums over the route's own phi.

CamMaskTwin is held_ref.HeldTwin whose `keep` drops the masked columns as well: the dense LM of the reduced problem."""
import numpy as np

import assembly_ref as ar
import free_ref as fr
import held_ref as hr
import prior_ref as pr
import shared_ref as sr
import weight_ref as wr
from freekd_twin import CNP

LD = ar.LD
NONE = (0,) * 10
F_ONLY = (1, 0, 0, 0, 0, 0, 0, 0, 0, 0)
F_K1_K2 = (1, 0, 0, 0, 0, 1, 1, 0, 0, 0)
MIXED_ROWS = (fr.ALL, F_K1_K2, NONE, F_ONLY)        # by j % 4: all free; {f, k1, k2}; none; {f}


def mixed_table(nC):
    """[nC, 10] uint8 cycling by j % 4 through MIXED_ROWS"""
    return np.asarray(MIXED_ROWS, dtype=np.uint8)[np.arange(int(nC)) % 4].copy()


def constant_table(nC, row):
    return np.tile(np.asarray(row, dtype=np.uint8).reshape(1, 10), (int(nC), 1))


def group_table(labels, rows=MIXED_ROWS):
    """a table constant on each group and mixed across groups: the groups in the order of their representatives cycle
    through `rows`"""
    rep = sr.representatives(labels)
    order = {r: n for n, r in enumerate(np.unique(rep).tolist())}
    return np.asarray(rows, dtype=np.uint8)[[order[r] % len(rows) for r in rep.tolist()]].copy()


def as_table(table, nC):
    return np.ones((nC, 10), dtype=bool) if table is None else (np.asarray(table).reshape(nC, 10) != 0)


class _CamMask:
    """mixin in front of held_ref._Held over free_ref.Route (16 wide): `_table` is set before the base constructors
    run, and the hook is _hold, the first thing any layer above free_ref.Route does with `held`"""

    def _hold(self, poses, pts):
        assert self.cnp == CNP, "blocks of 11 have no mask"
        self.table = as_table(self._table, self.nC)
        self.cam_free = self.table & (np.asarray(self.free).reshape(1, 10) != 0)        # the free bits per camera
        self.held_global = self.held.copy()                  # what the global mask alone holds
        masked = (CNP * np.arange(self.nC)[:, None] + np.arange(10)[None, :])[~self.cam_free]
        self.held_table = np.setdiff1d(masked, self.held_global).astype(np.int64)       # ... and the table on top
        self.held = np.union1d(self.held, masked).astype(np.int64)
        super()._hold(poses, pts)
        self.fixed_cams = np.flatnonzero(~self.cam_free.any(axis=1) & self.held_poses)   # wholly fixed

    def blocks(self, fault=None):
        """the blocks below with the columns the table masks zeroed per observation.  Fault for test_cammask_ref.py:
        "masked-column" leaves the first table-masked column of the first camera that has one as it was."""
        e, A, B, proj = super().blocks(None if fault == "masked-column" else fault)
        A = A.copy()
        keep = A.copy()
        zero = ~self.cam_free[self.j]                        # [nO, 10]
        A[:, :, :10] = np.where(zero[:, None, :], 0.0, A[:, :, :10])
        if fault == "masked-column":
            t = int(self.held_table[0])
            rows = self.j == t // CNP
            assert rows.any() and np.any(keep[rows, :, t % CNP] != 0.0)
            A[rows, :, t % CNP] = keep[rows, :, t % CNP]
        return e, A, B, proj


class CamMaskRoute(_CamMask, wr.WeightRoute):
    """the 16-block route with a table, and optionally holds, priors and a weighting (none: those layers are the
    identity and weight_ref.sums / judge reduce to held_ref's and free_ref's)"""

    def __init__(self, p, table, free=None, poses=None, pts=None, pri=None, loss=(wr.NONE, 1.0), sigma=None):
        self._table = table
        pri = pr.Priors(int(p["nC"]), CNP, int(p["nP"])) if pri is None else pri
        super().__init__(p, CNP, pri, loss, sigma, free, poses, pts)


def _groups_carry_equal_rows(rep, table):
    bad = np.argwhere(table != table[rep])
    assert bad.size == 0, f"camera {bad[0][0]} and its representative differ in coordinate {bad[0][1]}"


class CamMaskSharedRoute(_CamMask, hr.HeldSharedRoute):
    """held_ref.HeldSharedRoute with a table constant on every group; phi, away and keep per camera"""

    def __init__(self, p, labels, table, free=None, kc=None, poses=None, pts=None):
        self._table = table
        super().__init__(p, labels, free, kc, poses, pts)
        _groups_carry_equal_rows(self.rep, self.table)
        k = np.tile(np.arange(CNP), self.nC)
        j = np.repeat(np.arange(self.nC), CNP)
        shared = np.c_[self.cam_free, np.zeros((self.nC, 6), dtype=bool)].reshape(-1)
        self.phi = np.where(shared, CNP * self.rep[j] + k, CNP * j + k)
        self.away = self.phi != np.arange(self.nA)
        self.keep = np.r_[~self.away, np.ones(self.nB, dtype=bool)]


# ---- the fold with a table ---------------------------------------------------------------------------------------------

def fold(S, ea, rt, mu, coeff=1.0, fault=None):
    """shared_ref.fold over the route's own map phi (per camera: a coordinate masked for a group is summed into
    itself), in the dtype of S: rows, then columns summed into the representatives', mu once, folded-away coordinates
    cleared to (zero, coeff + mu, e_a = 0).  Fault "fold-masked": the map of the global mask, which also sums the
    members' placeholders of a coordinate masked for the group"""
    dt = S.dtype.type
    phi = sr.fold_map(rt.rep, rt.free)[0] if fault == "fold-masked" else rt.phi
    nA = phi.size
    k = np.arange(nA)
    S0 = S.copy()
    S0[k, k] -= dt(mu)
    rows = np.zeros_like(S0)
    np.add.at(rows, phi, S0)
    out = np.zeros_like(S0)
    np.add.at(out.T, phi, rows.T)
    out[k, k] += dt(mu)
    away = phi != k
    out[away, away] = dt(coeff) + dt(mu)
    e = np.zeros_like(ea)
    np.add.at(e, phi, ea)
    return out, e


def fold_bound(M, rt, mu):
    """shared_ref.fold_bound over the route's own map: (exact [nA, nA] 80-bit, bound, exact e_a, bound e_a, away) of the
    fold of an UNFOLDED reduce buffer whose handle carries the table -- gamma(n_r n_c + 2) sum |terms|; a masked
    coordinate has one source entry, its own placeholder"""
    phi, away = rt.phi, rt.away
    nA = phi.size
    n32 = M.shape[1]
    L = np.tril(M[:nA, :nA])
    sym = L + np.tril(L, -1).T
    S, ea = fold(ar.ld(sym), ar.ld(M[n32, :nA]), rt, mu)
    terms = np.abs(sym)
    terms[np.arange(nA), np.arange(nA)] += abs(mu)

    def both(x):
        rows = np.zeros_like(x)
        np.add.at(rows, phi, x)
        out = np.zeros_like(x)
        np.add.at(out.T, phi, rows.T)
        return out
    mag, cnt = both(terms), both(np.ones((nA, nA)))
    bound = ar.gamma(cnt + 2) * mag
    aw = np.flatnonzero(away)
    bound[aw, aw] = ar.U * (1.0 + abs(mu))                  # the placeholder 1 + mu: one rounding (no source entry)
    cnt_e = np.bincount(phi, minlength=nA)
    mag_e = np.bincount(phi, weights=np.abs(M[n32, :nA]), minlength=nA)
    return S, bound, ea, ar.gamma(cnt_e + 2) * mag_e, away


def shared_schur_ref(rt, sm, mu, rule=fr.NO_RULE, fault=None):
    """held_ref.shared_schur_ref with the fold above: the point blocks damped, the fold of the undamped camera part,
    then mu D once on the diagonal"""
    D = sr.damp_ref(rt, sm, rule)[0]
    S, ea = fold(*fr.schur_blocks(rt, mu, D, camera=False), rt, 0.0, fault=fault)
    k = np.arange(rt.nA)
    S[k, k] += LD(mu) * ar.ld(D[:rt.nA])
    return S.astype(np.float64), ea.astype(np.float64)


# ---- the exact parts ----------------------------------------------------------------------------------------------------

def check_table_parts(rt, W, cams, newcams):
    """psba_get_free_obs_blocks' W has zero rows at the masked coordinates of each observation's camera, non-zero focal
    rows where the focal length is free; the proposal carries the current bits at every masked coordinate"""
    zero = ~rt.cam_free[rt.j]
    assert np.all(W[:, :10, :][zero] == 0.0), "a masked row of W is not zero"
    live = rt.cam_free[rt.j][:, 0] & ~rt.held_pts[rt.i]
    assert np.all(np.abs(W[live][:, 0, :]).sum(axis=1) > 0.0), "a free focal row of W is zero"
    a = np.ascontiguousarray(np.asarray(cams)[:, :10][~rt.cam_free])
    b = np.ascontiguousarray(np.asarray(newcams)[:, :10][~rt.cam_free])
    assert a.tobytes() == b.tobytes(), "the proposal moved a masked intrinsic"


# ---- plain fp64 evaluations with the faults the judges must reject -------------------------------------------------------

def plain_try(rt, mu, rule=fr.NO_RULE, fault=None):
    """One damping try of a CamMaskRoute in plain fp64 from free_ref's plain pieces (what the kernels compute), with g,
    max_diag and D, in the form weight_ref.judge reads.  Faults: "masked-column" (one masked column left in A),
    "no-placeholder" (the diagonal of one table-masked coordinate keeps its zero sum), "max-diag-masked" (the maximum
    also over the table-masked coordinates of the unmasked diagonal)."""
    e, A, B, _ = rt.blocks(fault if fault == "masked-column" else None)
    U, ga, V, gb, W = fr.plain_sums(rt, e, A, B)
    hq = np.flatnonzero(rt.held_pts)
    V[hq] = np.eye(3)
    gb[hq] = 0.0
    k, k3 = np.arange(rt.cnp), np.arange(3)
    dU = U[:, k, k].reshape(-1)
    dU[rt.held] = 1.0
    if fault == "no-placeholder":
        dU[rt.held_table[0]] = 0.0
    diag = np.concatenate([dU, V[:, k3, k3].reshape(-1)])
    max_diag = float(diag[rt.free_all].max())
    if fault == "max-diag-masked":
        _, A0, _, _ = rt.unheld_blocks()
        d0, _ = ar._segsum((A0 * A0).sum(axis=1), rt.j, rt.nC)
        max_diag = float(max(max_diag, d0.reshape(-1)[rt.held_table].max()))
    D = rule.clamp(diag) if rule.marquardt else np.ones(rt.nT)
    S, ea, Vs = fr.plain_scatter(rt, U, dU, ga, V, gb, W, mu, D)
    g = np.concatenate([ga.reshape(-1), gb.reshape(-1)])
    blk = np.arange(rt.nA) // rt.cnp
    upper = blk[:, None] < blk[None, :]
    S[upper] = S.T[upper]                                    # (the mirror of k_free_finalize)
    dpa = fr.plain_solve(S, ea, fallback=fault is not None)
    if fault is None:
        dpa[rt.held] = 0.0
    out = fr.plain_finish(rt, S, ea, dict(Vs=Vs, W=W, g=g), dpa, mu, D, hold_b=hq if fault is None else None)
    cams, pts = rt.current()
    return dict(out, g=g, cams=cams, pts=pts, D=D if rule.marquardt else None, max_diag=max_diag, W=W)


def plain_shared_system(rt, mu, fault=None):
    """S, e_a of a CamMaskSharedRoute in plain fp64 under the identity rule: free_ref.plain_schur (placeholders at
    every held coordinate) and the kernels' fold over the coordinates that are free for the group.  Fault
    "fold-masked": the fold also sums the coordinates masked for a group"""
    S1, ea1, pc = fr.plain_schur(rt, mu)
    phi = sr.fold_map(rt.rep, rt.free)[0] if fault == "fold-masked" else rt.phi
    nA = rt.nA
    k = np.arange(nA)
    S0 = np.tril(S1) + np.tril(S1, -1).T
    S0[k, k] -= mu
    rows = np.zeros_like(S0)
    np.add.at(rows, phi, S0)
    out = np.zeros_like(S0)
    np.add.at(out.T, phi, rows.T)
    out[k, k] += mu
    e = np.zeros_like(ea1)
    np.add.at(e, phi, ea1)
    away = phi != k
    out[away, :] = 0.0
    out[:, away] = 0.0
    out[away, away] = 1.0 + mu
    e[away] = 0.0
    return np.tril(out) + np.tril(out, -1).T, e


# ---- a dense LM with the table: HeldTwin.levmar with the masked columns deleted as well -----------------------------------

class CamMaskTwin(hr.HeldTwin):
    """HeldTwin whose `keep` also drops the columns the table masks"""

    def __init__(self, prob, table, kc=None, free=None, poses=None, pts=None):
        super().__init__(prob, kc, free, poses, pts)
        self.table = as_table(table, self.nC)
        fa = self.keep[:self.nA].reshape(self.nC, CNP).copy()
        fa[:, :10] &= self.table
        self.keep = np.r_[fa.reshape(-1), self.keep[self.nA:]]


RING_FREE_CAMS, RING_FIXED_CAMS = (1, 3, 5), (0, 2, 4)


def mixed_ring(seed=7):
    """held_ref.held_ring (poses 0 and 1 held) for the recovery: cameras 0, 2 and 4 start at their true K and kc with
    the row none, cameras 1, 3 and 5 from the scene's start with the row {f, k1, k2}.  Returns (start problem, start
    kc [6, 5], held pose flags, table, K_true, kc_true)"""
    from freekd_twin import ring_problem
    start, kc0, poses = hr.held_ring(seed)
    _, _, K_true, kc_true = ring_problem(seed)
    K = np.array(start["K"], dtype=np.float64).reshape(-1, 5)
    kc = np.array(kc0, dtype=np.float64).reshape(-1, 5)
    fixed = list(RING_FIXED_CAMS)
    K[fixed], kc[fixed] = K_true[fixed], kc_true[fixed]
    table = constant_table(6, F_K1_K2)
    table[fixed] = 0
    return dict(start, K=K), kc, poses, table, K_true, kc_true
