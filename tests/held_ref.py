"""Host reference of held poses and points on the free-intrinsics routes (psba_set_held; no GPU):
tests/test_held_ref.py applies it to plain fp64 evaluations and injected faults, tests/test_gpu_held.py to the kernels.

Two statements of the same problem.  REDUCED: the held columns of J are deleted, the normal equations of what is left
are solved, and the step is scattered back with zeros.  EMBEDDED (what the device stores): the full-size system with
the held columns of A and the held rows of B zeroed and the placeholder coeff on the held diagonal entries, so that a
held coordinate is what a coordinate held by psba_set_intrinsics_mask is.  A held pose is the last six coordinates of
a camera block; a held point its three coordinates.

HeldRoute is free_ref.Route with the zeroed blocks and `held` extended by the pose coordinates, so that every judge of
free_ref.py (sums, damp_ref, scale_diag, check_exact_parts, dpb_residual, scalars, solve_judge) applies unchanged with
its constants; HeldSharedRoute is the same on shared_ref.SharedRoute.  The point placeholders, which free_ref has no
notion of, are patched in by sums() below (V = coeff I, g_b = 0, zero envelopes; the diagonals `dampings` and damp_ref
read patched the same way).  schur_blocks IS free_ref.schur_blocks, which skips the points the route holds (their W is
zero: they contribute nothing, and at mu = 0 their V of the sums is singular) and serves both damping rules; plain_try
is assembled from free_ref's plain_sums, plain_scatter, plain_solve and plain_finish around its own fault switches; and
HeldTwin is TwinKD's LM loop with the solve of a step overridden."""
import numpy as np

import assembly_ref as ar
import free_ref as fr
import shared_ref as sr
from freekd_twin import CNP, TwinKD, cholesky_solve

LD = ar.LD


class _Held:
    """mixin over free_ref.Route: poses [nC] and pts [nP] flags, non-zero = held"""

    def _hold(self, poses, pts):
        hp = np.zeros(self.nC, dtype=bool) if poses is None else (np.asarray(poses).reshape(self.nC) != 0)
        hq = np.zeros(self.nP, dtype=bool) if pts is None else (np.asarray(pts).reshape(self.nP) != 0)
        self.held_poses, self.held_pts = hp, hq
        self.ni = self.cnp - 6
        self.held_mask = self.held.copy()                    # the coordinates the intrinsics mask holds
        pose = (self.cnp * np.flatnonzero(hp)[:, None] + self.ni + np.arange(6)[None, :]).reshape(-1)
        self.held_pose = pose
        self.held = np.union1d(self.held, pose).astype(np.int64)
        self.held_b = (3 * np.flatnonzero(hq)[:, None] + np.arange(3)[None, :]).reshape(-1)   # within the point part
        self.held_all = np.r_[self.held, self.nA + self.held_b].astype(np.int64)
        self.free_all = np.ones(self.nT, dtype=bool)
        self.free_all[self.held_all] = False

    def blocks(self, fault=None):
        """the twin's blocks with the held pose columns of A and the held points' B zeroed.  Faults for
        test_held_ref.py: "pose-column" leaves the first pose column of the first held camera as it was."""
        e, A, B, proj = super().blocks()
        A, B = A.copy(), B.copy()
        keep = A[:, :, self.ni].copy()
        A[self.held_poses[self.j], :, self.ni:] = 0.0
        if fault == "pose-column":
            rows = self.j == np.flatnonzero(self.held_poses)[0]
            A[rows, :, self.ni] = keep[rows]
        B[self.held_pts[self.i]] = 0.0
        return e, A, B, proj

    def unheld_blocks(self):
        """the route's blocks without the holds (the intrinsics mask applied): what the reduced statement deletes from"""
        return super().blocks()


class HeldRoute(_Held, fr.Route):
    def __init__(self, p, cnp, free=None, poses=None, pts=None):
        super().__init__(p, cnp, free)
        self._hold(poses, pts)


class HeldSharedRoute(_Held, sr.SharedRoute):
    def __init__(self, p, labels, free=None, kc=None, poses=None, pts=None):
        super().__init__(p, labels, free, kc)
        self._hold(poses, pts)


def largest_pose_camera(p, cnp, free=None):
    """the camera whose pose diagonal holds the largest entry of diag N of the route without holds (held, a max_diag
    that forgets the mask reports it), and whether that entry is the largest of the whole diagonal"""
    rt = fr.Route(p, cnp, free)
    sm = fr.sums(rt)
    dU = sm["diagU"].copy()
    dU[rt.held] = 0.0
    pose = dU.reshape(rt.nC, cnp)[:, cnp - 6:]
    return int(np.argmax(pose.max(axis=1))), bool(pose.max() >= max(dU.max(), sm["diagV"].max()))


def point_with_views(p, n=3, skip=0):
    """the (skip + 1)-th point seen by at least n cameras"""
    return int(np.flatnonzero(np.bincount(np.asarray(p["iidx"]), minlength=int(p["nP"])) >= n)[skip])


def flags(n, idx):
    m = np.zeros(n, dtype=np.uint8)
    m[np.asarray(idx, dtype=np.int64)] = 1
    return m


def sums(rt, coeff=1.0, coeff_g=1.0):
    """free_ref.sums of the held route with the point placeholders: V = coeff I, g_b = 0 and zero envelopes at held
    points, and the diagonal `dampings` and damp_ref read (diagV, diagVx, envdV) patched the same way"""
    sm = fr.sums(rt, coeff, coeff_g)
    hq, hb = np.flatnonzero(rt.held_pts), rt.held_b
    sm["V"][hq] = LD(coeff) * np.eye(3, dtype=LD)
    sm["envV"][hq] = 0.0
    sm["g"][rt.nA + hb] = 0
    sm["envg"][rt.nA + hb] = 0.0
    sm["diagV"][hb] = coeff
    sm["diagVx"][hb] = LD(coeff)
    sm["envdV"][hb] = 0.0
    return sm


def dampings(rt, sm):
    """test_gpu_free_entrywise.dampings over the free entries of cameras AND points: (mu = 1e-3 max diag over the
    free entries, mu = 1e-6 median diag N) and the diagonal of N"""
    diag = np.concatenate([sm["diagU"], sm["diagV"]])
    return {"big": 1e-3 * float(diag[rt.free_all].max()), "small": 1e-6 * float(np.median(diag))}, diag


def damp_ref(rt, sm, rule=fr.NO_RULE):
    """free_ref.damp_ref; D of a held point is clamp(coeff) exactly (no envelope)"""
    D, env = fr.damp_ref(rt, sm, rule)
    env = env.copy()
    env[rt.nA + rt.held_b] = 0.0
    return D, env


schur_blocks = fr.schur_blocks      # (it skips the route's held points)


def schur_ref(rt, sm, mu, rule=fr.NO_RULE):
    """S and e_a of the embedded system in 80-bit, rounded once to double (either rule)"""
    S, ea = schur_blocks(rt, mu, damp_ref(rt, sm, rule)[0])
    return S.astype(np.float64), ea.astype(np.float64)


def shared_schur_ref(rt, sm, mu, rule=fr.NO_RULE):
    """shared_ref.schur_ref on the held route's blocks: the point blocks damped, the fold of the undamped camera
    part (it touches intrinsic coordinates only), then mu D once on the diagonal"""
    D = sr.damp_ref(rt, sm, rule)[0]
    S, ea = sr.fold(*schur_blocks(rt, mu, D, camera=False), rt.rep, rt.free, 0.0)
    k = np.arange(rt.nA)
    S[k, k] += LD(mu) * ar.ld(D[:rt.nA])
    return S.astype(np.float64), ea.astype(np.float64)


# ---- the exact parts ---------------------------------------------------------------------------------------------------

def check_held_system(rt, S, ea, mu, rule=fr.NO_RULE, coeff=1.0):
    """free_ref.check_exact_parts (held rows clear, e_a = 0, the placeholder diagonal) and the held COLUMNS"""
    fr.check_exact_parts(rt, S, ea, mu, rule, coeff)
    col = S[:, rt.held].copy()
    col[rt.held, np.arange(rt.held.size)] = 0.0
    assert np.all(col == 0.0), "a held column is not clear"


def check_held_step(rt, g, dp, cur, new):
    """g and dp exactly 0 at every held entry; the proposal bit-identical to the current values there.  g may be None;
    cur, new: flat [nT] (cameras then points)"""
    idx = rt.held_all
    if g is not None:
        assert np.all(np.asarray(g)[idx] == 0.0), "g of a held entry is not 0"
    assert np.all(np.asarray(dp)[idx] == 0.0), "dp of a held entry is not 0"
    a, b = np.ascontiguousarray(np.asarray(cur)[idx]), np.ascontiguousarray(np.asarray(new)[idx])
    assert a.tobytes() == b.tobytes(), "the proposal moved a held entry"


def check_max_diag(rt, sm, got):
    """psba_max_diag: the maximum over the free entries (the rule of test_gpu_free_entrywise.py: 1e-11 relative)"""
    want = float(np.concatenate([sm["diagU"], sm["diagV"]])[rt.free_all].max())
    assert abs(got - want) <= 1e-11 * want, f"max diag {got!r}, over the free entries {want!r}"
    return want


def flat(cams, pts):
    return np.concatenate([np.asarray(cams, dtype=np.float64).reshape(-1), np.asarray(pts, dtype=np.float64).reshape(-1)])


# ---- reduced against embedded (dense, fp64) ------------------------------------------------------------------------------

def dense_normal(rt, blocks):
    """N = J^T J [nT, nT] and g = J^T e of blocks (e, A, B, _)"""
    e, A, B, _ = blocks
    J = np.zeros((2 * rt.nO, rt.nT))
    for a in range(rt.nO):
        J[2 * a:2 * a + 2, rt.cnp * rt.j[a]:rt.cnp * rt.j[a] + rt.cnp] = A[a]
        J[2 * a:2 * a + 2, rt.nA + 3 * rt.i[a]:rt.nA + 3 * rt.i[a] + 3] = B[a]
    return J.T @ J, J.T @ e.reshape(-1)


def reduced_solve(rt, mu, scaled=False):
    """the held columns deleted from the unheld blocks, (N_ff + mu I) x = g_f solved, scattered back with zeros.
    scaled: solved in the scaling diag(N_ff + mu I)^-1/2 (for mu = 0, where the focal-length rows would hide the rest)"""
    N, g = dense_normal(rt, rt.unheld_blocks())
    f = rt.free_all
    Nf, gf = N[np.ix_(f, f)] + mu * np.eye(int(f.sum())), g[f]
    d = 1.0 / np.sqrt(np.diag(Nf)) if scaled else np.ones(gf.size)
    dp = np.zeros(rt.nT)
    dp[f] = d * np.linalg.solve(d[:, None] * Nf * d[None, :], d * gf)
    return dp


def embedded_solve(rt, mu, coeff=1.0):
    """the zeroed blocks, the placeholder on the held diagonal, (N + mu I) dp = g solved in full size"""
    N, g = dense_normal(rt, rt.blocks())
    N[rt.held_all, rt.held_all] = coeff
    return np.linalg.solve(N + mu * np.eye(rt.nT), g), N, g


def reduced_scaled_S(rt, mu=0.0):
    """the Schur complement of the reduced system scaled by its own diagonal (the conditioning facts of the GPU tests);
    no holds: the full-size one"""
    N, g = dense_normal(rt, rt.unheld_blocks())
    fa = rt.free_all[:rt.nA]
    Naa, Nab, Nbb = N[:rt.nA, :rt.nA][np.ix_(fa, fa)], N[:rt.nA, rt.nA:][fa], N[rt.nA:, rt.nA:]
    fb = rt.free_all[rt.nA:]
    Nab, Nbb = Nab[:, fb], Nbb[np.ix_(fb, fb)] + mu * np.eye(int(fb.sum()))
    S = Naa + mu * np.eye(int(fa.sum())) - Nab @ np.linalg.solve(Nbb, Nab.T)
    d = 1.0 / np.sqrt(np.diag(S))
    return d[:, None] * S * d[None, :]


# ---- a plain fp64 evaluation with the faults the judges must reject -----------------------------------------------------

def plain_try(rt, mu, rule=fr.NO_RULE, fault=None):
    """free_ref.plain_try for the held route, from free_ref's pieces: one damping try in plain fp64 (what the kernels
    compute), with g and max_diag.  Faults: "pose-column" (a held pose column of A left non-zero), "no-placeholder"
    (the held diagonals keep their zero sums), "point-g" (g_b of a held point from its unzeroed B), "max-diag-all" (the
    maximum over every coordinate of the unheld diagonal).  A faulted try leaves the held entries of the step as
    they come out."""
    e, A, B, _ = rt.blocks(fault)
    U, ga, V, gb, W = fr.plain_sums(rt, e, A, B)
    hq = np.flatnonzero(rt.held_pts)
    V[hq] = np.eye(3)
    gb[hq] = 0.0
    if fault == "point-g":
        _, _, B0, _ = rt.unheld_blocks()
        g0 = np.zeros((rt.nP, 3))
        np.add.at(g0, rt.i, np.einsum("ari,ar->ai", B0, e))
        gb[hq] = g0[hq]
    k, k3 = np.arange(rt.cnp), np.arange(3)
    dU = U[:, k, k].reshape(-1)
    dU[rt.held_mask] = 1.0
    if fault != "no-placeholder":
        dU[rt.held] = 1.0
    diag = np.concatenate([dU, V[:, k3, k3].reshape(-1)])
    max_diag = float(diag[rt.free_all].max())
    if fault == "max-diag-all":
        _, A0, B0, _ = rt.unheld_blocks()
        d0, _ = ar._segsum((A0 * A0).sum(axis=1), rt.j, rt.nC)
        max_diag = float(max(d0.max(), diag.max()))
    D = rule.clamp(diag) if rule.marquardt else np.ones(rt.nT)
    S, ea, Vs = fr.plain_scatter(rt, U, dU, ga, V, gb, W, mu, D)
    g = np.concatenate([ga.reshape(-1), gb.reshape(-1)])
    dpa = fr.plain_solve(S, ea)
    if fault is None:
        dpa[rt.held] = 0.0
    out = fr.plain_finish(rt, S, ea, dict(Vs=Vs, W=W, g=g), dpa, mu, D, hold_b=hq if fault is None else None)
    return dict(out, g=g, cams=rt.current()[0], D=D, max_diag=max_diag)


# ---- a dense LM with the holds: TwinKD.levmar with the held columns deleted ---------------------------------------------

class HeldTwin(TwinKD):
    """TwinKD whose levmar (TwinKD's own loop and log rows) solves the reduced system, with the largest diagonal entry
    taken over the columns that are left: poses [nC], pts [nP] flags, non-zero = held"""

    def __init__(self, prob, kc=None, free=None, poses=None, pts=None):
        super().__init__(prob, kc, free)
        hp = np.zeros(self.nC, dtype=bool) if poses is None else (np.asarray(poses).reshape(self.nC) != 0)
        hq = np.zeros(self.nP, dtype=bool) if pts is None else (np.asarray(pts).reshape(self.nP) != 0)
        fa = self.free_a.reshape(self.nC, CNP).copy()
        fa[hp, 10:] = False
        self.keep = np.r_[fa.reshape(-1), np.repeat(~hq, 3)]   # the columns that are left

    def start_mu(self, tau, N):
        return tau * float(np.diag(N)[self.keep].max())

    def solve_step(self, N, g, mu, D):
        """TwinKD.solve_step on the columns `keep`: N, g and D restricted to them, the step scattered back with zeros"""
        f = self.keep
        x = cholesky_solve(N[np.ix_(f, f)] + mu * np.diag(D[f]), g[f])
        if x is None:
            return None
        dp = np.zeros(self.nT)
        dp[f] = x
        return dp


def held_ring(seed=7):
    """freekd_twin.ring_problem with the true poses of cameras 0 and 1 written into the start (its local rotations
    are zero and its translations those of _ring_cameras(6)): (start problem, start kc, held pose flags)"""
    from freekd_twin import _ring_cameras, ring_problem
    start, kc0, _, _ = ring_problem(seed)
    _, t = _ring_cameras(6)
    cams = np.array(start["cams"], dtype=np.float64)
    cams[:2, :3] = 0.0
    cams[:2, 3:] = t[:2]
    poses = np.zeros(6, dtype=np.uint8)
    poses[:2] = 1
    return dict(start, cams=cams), kc0, poses
