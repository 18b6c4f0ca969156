"""Independent (test-only) numpy twin of PSBA_CAMERA_FREE_KD: camera blocks of 16 parameters
(fu, u0, v0, ar, s | k1, k2, k3, k4, k5 | v0, v1, v2 | t0, t1, t2) with a mask over the ten intrinsics.

Built on lens_twin.Twin (projection, the six extrinsic columns and B); this file adds the ten intrinsic columns
(include/psba_hip.h): with (x, y) the normalised point, r2 = x^2 + y^2, (xd, yd) the distorted point,
    d(u, v) / d(fu, u0, v0, ar, s) = [ xd, 1, 0, 0, yd ;  ar yd, 0, 1, fu yd, 0 ]
    d xd / d(k1..k5) = (r2 x, r2^2 x, 2 x y, r2 + 2 x^2, r2^3 x)
    d yd / d(k1..k5) = (r2 y, r2^2 y, r2 + 2 y^2, 2 x y, r2^3 y)
    d u / dk = fu d xd + s d yd,   d v / dk = fu ar d yd
a dense J, N = J^T J with the placeholder 1 on the diagonal of masked coordinates, S and e_a by a dense solve of the
point block, and a dense LM that restates the damping and accept rules of psba_amd/csrc/lm_loop.cpp.  Formulated
differently from the HIP route on purpose: one dense matrix, no blocks, no Schur elimination inside the LM.

Two things live here once for every reference of the free-intrinsics routes: TwinKD.levmar, the LM loop that
damping_twin.TwinDamp, held_ref.HeldTwin (and prior_ref.PriorTwin, weight_ref.WeightTwin on it) and shared_ref.SharedTwin
specialise by overriding system, start_mu, damping_diag, solve_step, proposal and norm2; and ldl_rows, the per-point L D L^T
substitution of the 80-bit Schur restatements.
"""
import numpy as np

import lens_twin

CNP = 16
BAL = (1, 0, 0, 0, 0, 1, 1, 0, 0, 0)


class LmResult:
    pass


class TwinKD:
    """prob: Problem / dict (K, initrot, cams, pts, impts, iidx, jidx); kc [nC, 5] starting distortion or None;
    free [10] the intrinsics mask (non-zero = optimised), None = all free."""

    def __init__(self, prob, kc=None, free=None):
        self.t = lens_twin.Twin(prob, kc)
        t = self.t
        self.nC, self.nP, self.nO = t.nC, t.nP, t.nO
        self.i, self.j = t.i, t.j
        self.cams = np.hstack([t.K, t.kc, t.cams]).copy()  # [nC, 16]
        self.pts = t.pts.copy()
        self.free = np.ones(10, dtype=bool) if free is None else (np.asarray(free).reshape(10) != 0)
        self.nA, self.nB = CNP * self.nC, 3 * self.nP
        self.nT = self.nA + self.nB
        # per coordinate of the camera part: is it optimised?
        self.free_a = np.tile(np.r_[self.free, np.ones(6, dtype=bool)], self.nC)

    def _set(self, cams, pts):
        cams = self.cams if cams is None else np.asarray(cams, dtype=np.float64).reshape(self.nC, CNP)
        pts = self.pts if pts is None else np.asarray(pts, dtype=np.float64).reshape(self.nP, 3)
        self.t.K, self.t.kc = cams[:, :5], cams[:, 5:10]
        return cams, pts

    def residual(self, cams=None, pts=None):
        cams, pts = self._set(cams, pts)
        return self.t.m - self.t.project(cams[:, 10:], pts)

    def cost(self, cams=None, pts=None):
        e = self.residual(cams, pts)
        return float((e * e).sum())

    def linearize(self, cams=None, pts=None, masked=True):
        """e [nO, 2], A [nO, 2, 16] (masked columns zero), B [nO, 2, 3]: derivatives of the projection"""
        cams, pts = self._set(cams, pts)
        proj, A6, B = self.t.project(cams[:, 10:], pts, jac=True)
        e = self.t.m - proj
        c, M = cams[self.j], pts[self.i]
        s, u, _ = lens_twin._quat(self.t.q0[self.j], c[:, 10:13])
        P = np.einsum("nab,nb->na", lens_twin._rot(s, u), M) + c[:, 13:]
        x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
        xd, yd, _ = lens_twin.distort(c[:, 5:10], x, y)
        fu, ar, sk = c[:, 0], c[:, 3], c[:, 4]
        r2 = x * x + y * y
        A = np.zeros((self.nO, 2, CNP))
        A[:, 0, 0], A[:, 0, 1], A[:, 0, 4] = xd, 1.0, yd
        A[:, 1, 0], A[:, 1, 2], A[:, 1, 3] = ar * yd, 1.0, fu * yd
        dxd = np.stack([r2 * x, r2 ** 2 * x, 2 * x * y, r2 + 2 * x * x, r2 ** 3 * x], 1)
        dyd = np.stack([r2 * y, r2 ** 2 * y, r2 + 2 * y * y, 2 * x * y, r2 ** 3 * y], 1)
        A[:, 0, 5:10] = fu[:, None] * dxd + sk[:, None] * dyd
        A[:, 1, 5:10] = (fu * ar)[:, None] * dyd
        A[:, :, 10:] = A6
        if masked:
            A[:, :, :10] *= self.free[None, None, :]
        return e, A, B

    def jacobian(self, masked=True):
        """dense J [2 nO, nA + nB] of the projection (columns: cameras, then points)"""
        e, A, B = self.linearize(masked=masked)
        J = np.zeros((2 * self.nO, self.nT))
        for a in range(self.nO):
            J[2 * a:2 * a + 2, CNP * self.j[a]:CNP * self.j[a] + CNP] = A[a]
            J[2 * a:2 * a + 2, self.nA + 3 * self.i[a]:self.nA + 3 * self.i[a] + 3] = B[a]
        return e, J

    def normal(self):
        """(cost, N = J^T J with 1 on the diagonal of masked coordinates, g = J^T e)"""
        e, J = self.jacobian()
        N = J.T @ J
        held = np.flatnonzero(~self.free_a)
        N[held, held] = 1.0
        return float((e * e).sum()), N, J.T @ e.reshape(-1)

    def max_diag(self, N):
        d = np.diag(N).copy()
        d[:self.nA][~self.free_a] = 0.0
        return d.max()

    def schur(self, N, g, mu):
        """S = U* - W V*^-1 W^T, e_a = g_a - W V*^-1 g_b by a dense solve of the (damped) point block"""
        nA = self.nA
        Nbb = N[nA:, nA:] + mu * np.eye(self.nB)
        X = np.linalg.solve(Nbb, np.c_[N[:nA, nA:].T, g[nA:]])
        S = N[:nA, :nA] + mu * np.eye(nA) - N[:nA, nA:] @ X[:, :nA]
        ea = g[:nA] - N[:nA, nA:] @ X[:, nA]
        return S, ea

    def schur_blocks(self, mu, dtype=np.longdouble):
        """The same S and e_a from the fp64 Jacobian blocks with every sum in `dtype` (80-bit by default), block by
        block: what the fp64 twin's own rounding is measured against."""
        e, A, B = self.linearize()
        e, A, B = e.astype(dtype), A.astype(dtype), B.astype(dtype)
        nC, nP = self.nC, self.nP
        U = np.zeros((nC, CNP, CNP), dtype)
        ga = np.zeros((nC, CNP), dtype)
        np.add.at(U, self.j, np.einsum("nri,nrk->nik", A, A))
        np.add.at(ga, self.j, np.einsum("nri,nr->ni", A, e))
        V = np.zeros((nP, 3, 3), dtype)
        gb = np.zeros((nP, 3), dtype)
        np.add.at(V, self.i, np.einsum("nri,nrk->nik", B, B))
        np.add.at(gb, self.i, np.einsum("nri,nr->ni", B, e))
        W = np.einsum("nri,nrk->nik", A, B)
        S = np.zeros((self.nA, self.nA), dtype)
        ea = ga.reshape(-1).copy()
        for j in range(nC):
            Uj = U[j].copy()
            for k in np.flatnonzero(~self.free):
                Uj[k, k] = 1
            S[CNP * j:CNP * j + CNP, CNP * j:CNP * j + CNP] = Uj + dtype(mu) * np.eye(CNP, dtype=dtype)
        for i, obs in obs_by_point(self.i, nP):
            Wi = W[obs].reshape(-1, 3)                 # rows: (observation, parameter)
            Yi = ldl_rows(V[i] + dtype(mu) * np.eye(3, dtype=dtype), Wi)
            rows = (CNP * self.j[obs][:, None] + np.arange(CNP)[None, :]).reshape(-1)
            S[np.ix_(rows, rows)] -= Yi @ Wi.T
            ea[rows] -= Yi @ gb[i]
        return S, ea

    # ---- what levmar asks of the twin: a subclass overrides these, never the loop ----
    def system(self):
        """(cost, N, g) of the current parameters in the numbering of the loop"""
        return self.normal()

    def start_mu(self, tau, N):
        return tau * self.max_diag(N)

    def damping_diag(self, N):
        """D [n] of a linearization: the system solved is N + mu diag(D)"""
        return np.ones(N.shape[0])

    def solve_step(self, N, g, mu, D):
        """dp of (N + mu diag(D)) dp = g by a Cholesky factorization, None when it breaks down"""
        dp = cholesky_solve(N + mu * np.diag(D), g)
        if dp is not None:
            dp[:self.nA][~self.free_a] = 0.0
        return dp

    def proposal(self, dp):
        return self.cams + dp[:self.nA].reshape(self.nC, CNP), self.pts + dp[self.nA:].reshape(self.nP, 3)

    def norm2(self, cams, pts):
        """|p|^2 of the loop's p_L2"""
        return float((cams * cams).sum() + (pts * pts).sum())

    def levmar(self, max_iter=20, init_mu=0.0, stop_small=True):
        """psba_amd/csrc/lm_loop.cpp restated (tr_handoff off): Nielsen's mu / nu update, the same stop tests, one
        log row (itno, cost after the try, rho, mu, accepted) per damping try.  stop_small=False leaves out the
        loop's absolute stop (cost <= 1e-12), which ends a noise-free problem before fp64 is used up.  The only LM
        loop of the free-intrinsics twins: the system is system() (normal() here), everything else that differs between them is one of
        the methods above, and dp, g and D live in whatever numbering those methods share."""
        STOP, EPS_SQ = 1e-12, 1e-24
        tau = init_mu if init_mu != 0.0 else 1e-3
        res, log = LmResult(), []
        ex, N, g = self.system()
        res.init_err = ex
        mu, nu, p_L2, first, flag, tries = 0.0, 2, 0.0, True, 0, 0
        itno = 0
        while itno < max_iter and flag == 0:
            if not first:
                _, N, g = self.system()
            else:
                mu, p_L2, nu, first = self.start_mu(tau, N), 1e3, 2, False
                res.mu0 = mu
            D = self.damping_diag(N)
            while True:
                tries += 1
                dp = self.solve_step(N, g, mu, D)
                if dp is not None:
                    dp_L2 = float(dp @ dp)
                    if dp_L2 < p_L2 * STOP * STOP:
                        flag = 1
                        break
                    if dp_L2 >= (p_L2 + STOP) / EPS_SQ:
                        flag = 2
                        break
                    newc, newp = self.proposal(dp)
                    new_ex = self.cost(newc, newp)
                    rho = (ex - new_ex) / float(dp @ ((mu * D) * dp + g))
                    log.append([itno, new_ex, rho, mu, 1.0 if rho > 0 else 0.0])
                    if rho > 0:
                        tmp = 2 * rho - 1
                        tmp = 1.0 - tmp * tmp * tmp
                        mu *= tmp if tmp >= 1.0 / 3.0 else 1.0 / 3.0
                        nu = 2
                        self.cams, self.pts = newc, newp
                        p_L2 = self.norm2(newc, newp)
                        ex = new_ex
                        break
                else:
                    log.append([itno, np.nan, np.nan, mu, -1.0])
                mu *= nu
                if 2.0 * nu > 1e9:
                    flag = 2
                    break
                nu *= 2
            if stop_small and ex <= STOP:
                flag = 3
            itno += 1
        res.flag, res.iters, res.tries, res.final_err, res.mu_final = flag, itno, tries, ex, mu
        return res, np.asarray(log).reshape(-1, 5)


def cholesky_solve(M, g):
    """M^-1 g through M = L L^T, None when the factorization breaks down"""
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, g))


def obs_by_point(i, nP):
    """(point, indices of its observations in their given order) for every point that has any"""
    order = np.argsort(i, kind="stable")
    ptr = np.searchsorted(i[order], np.arange(nP + 1))
    for k in range(nP):
        if ptr[k + 1] > ptr[k]:
            yield k, order[ptr[k]:ptr[k + 1]]


def ldl_rows(v, Wi):
    """Y = Wi v^-1 for a symmetric v [3, 3] and rows Wi [n, 3], by L D L^T and substitution in the operands' dtype:
    backward stable per row, so a nearly singular block (a point seen once, small mu) does not amplify rounding the way
    a product with its inverse would.  The one statement of it for every 80-bit reference of the free-intrinsics
    routes (TwinKD.schur_blocks, free_ref.schur_blocks)."""
    l10, l20 = v[0, 1] / v[0, 0], v[0, 2] / v[0, 0]
    d1 = v[1, 1] - l10 * v[0, 1]
    l21 = (v[1, 2] - l20 * v[0, 1]) / d1
    d2 = v[2, 2] - l20 * v[0, 2] - l21 * l21 * d1
    z1 = Wi[:, 1] - l10 * Wi[:, 0]
    z2 = Wi[:, 2] - l20 * Wi[:, 0] - l21 * z1
    y2 = z2 / d2
    y1 = z1 / d1 - l21 * y2
    return np.stack([Wi[:, 0] / v[0, 0] - l10 * y1 - l20 * y2, y1, y2], 1)


# ---- the test problems of tests/test_freekd_*.py ----
def start_kc(nC):
    """(2e-2, -5e-3, 1e-3, -1e-3, 1e-3) (1 + 0.1 N(0, 1)) per camera, default_rng(1)"""
    rng = np.random.default_rng(1)
    return np.array([2e-2, -5e-3, 1e-3, -1e-3, 1e-3]) * (1.0 + 0.1 * rng.standard_normal((nC, 5)))


def _rot_to_quat(R):
    """unit quaternion (s, u) with R'(q) = R (R a rotation, trace > -1)"""
    s = 0.5 * np.sqrt(1.0 + np.trace(R))
    u = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4.0 * s)
    return np.r_[s, u]


def tiny_problem():
    """2 cameras, 3 points: point 0 seen by both, point 1 by camera 0 only, point 2 by camera 1 only."""
    rng = np.random.default_rng(5)
    pts = np.array([[0.1, -0.2, 0.3], [-0.4, 0.3, -0.1], [0.5, 0.2, 0.2]])
    K = np.array([[800.0, 3.0, -2.0, 1.01, 0.5], [820.0, -1.0, 4.0, 0.99, -0.3]])
    q0 = np.array([[1.0, 0, 0, 0], [np.cos(0.1), 0, np.sin(0.1), 0]])
    cams = np.array([[0.01, -0.02, 0.005, 0.1, -0.1, 5.0], [-0.01, 0.015, 0.02, -0.2, 0.1, 5.5]])
    iidx, jidx = np.array([0, 0, 1, 2], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32)
    prob = dict(K=K, initrot=q0, cams=cams, pts=pts, impts=np.zeros((4, 2)), iidx=iidx, jidx=jidx, nC=2, nP=3, nO=4)
    prob["impts"] = lens_twin.Twin(prob, start_kc(2)).project() + rng.standard_normal((4, 2))
    return prob


def ring_problem(seed=7):
    """6 cameras at radius 5 looking at the origin, 120 points uniform in [-1, 1]^3, 30 % of the observations dropped
    (not those of cameras 0 and 1); exact projections with K = (800 (1 + 0.05 N), 0, 0, 1, 0) and kc = (-0.05, 0.01,
    0, 0, 0) (1 + 0.2 N).  Returns (start problem, start kc = 0, true K [6, 5], true kc [6, 5])."""
    rng = np.random.default_rng(seed)
    nC, nP = 6, 120
    pts = rng.uniform(-1.0, 1.0, (nP, 3))
    q0, t = np.zeros((nC, 4)), np.zeros((nC, 3))
    for j in range(nC):
        th = 2.0 * np.pi * j / nC
        centre = 5.0 * np.array([np.cos(th), 0.0, np.sin(th)])
        z = -centre / np.linalg.norm(centre)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])      # rows: camera axes in world coordinates
        q0[j] = _rot_to_quat(R)
        t[j] = -R @ centre
    K = np.zeros((nC, 5))
    K[:, 0] = 800.0 * (1.0 + 0.05 * rng.standard_normal(nC))
    K[:, 3] = 1.0
    kc = np.array([-0.05, 0.01, 0.0, 0.0, 0.0]) * (1.0 + 0.2 * rng.standard_normal((nC, 5)))
    keep = rng.uniform(size=(nP, nC)) >= 0.3
    keep[:, :2] = True
    iidx, jidx = np.nonzero(keep)
    cams = np.hstack([np.zeros((nC, 3)), t])
    true = dict(K=K, initrot=q0, cams=cams, pts=pts, impts=np.zeros((iidx.size, 2)), iidx=iidx.astype(np.int32),
                jidx=jidx.astype(np.int32), nC=nC, nP=nP, nO=int(iidx.size))
    impts = lens_twin.Twin(true, kc).project()
    Ks = K.copy()
    Ks[:, 0] *= 1.03
    cs = cams.copy()
    cs[:, :3] += 0.005 * rng.standard_normal((nC, 3))
    cs[:, 3:] += 0.02 * rng.standard_normal((nC, 3))
    start = dict(true, K=Ks, cams=cs, pts=pts + 0.02 * rng.standard_normal((nP, 3)), impts=impts)
    return start, np.zeros((nC, 5)), K, kc


def _rot_to_quat_any(R):
    """_rot_to_quat for any rotation (a ring of 4 k cameras holds a half turn, trace = -1): the largest of the four
    components from the diagonal, the other three from the off-diagonal sums and differences"""
    tr = np.trace(R)
    c2 = np.r_[1.0 + tr, 1.0 + 2.0 * np.diag(R) - tr] / 4.0
    k = int(np.argmax(c2))
    if k == 0:
        return _rot_to_quat(R)
    a = k - 1
    b, c = (a + 1) % 3, (a + 2) % 3
    q = np.zeros(4)
    q[k] = np.sqrt(c2[k])
    q[0] = (R[c, b] - R[b, c]) / (4.0 * q[k])
    q[1 + b] = (R[a, b] + R[b, a]) / (4.0 * q[k])
    q[1 + c] = (R[a, c] + R[c, a]) / (4.0 * q[k])
    return q


def _ring_cameras(nC, radius=5.0):
    """initrot [nC, 4] and translations [nC, 3] of nC cameras on a ring in the x-z plane, looking at the origin"""
    q0, t = np.zeros((nC, 4)), np.zeros((nC, 3))
    for j in range(nC):
        th = 2.0 * np.pi * j / nC
        centre = radius * np.array([np.cos(th), 0.0, np.sin(th)])
        z = -centre / np.linalg.norm(centre)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        q0[j] = _rot_to_quat_any(R)
        t[j] = -R @ centre
    return q0, t


def _varied_K(rng, nC):
    """f 800 (1 +- 2 %), u0 / v0 a few pixels, ar 1 +- 1 %, skew +- 0.3: no intrinsic column is degenerate"""
    return np.stack([800.0 * (1.0 + rng.uniform(-0.02, 0.02, nC)), rng.uniform(-5.0, 5.0, nC), rng.uniform(-5.0, 5.0, nC),
                     1.0 + rng.uniform(-0.01, 0.01, nC), rng.uniform(-0.3, 0.3, nC)], 1)


def _scene(rng, nC, pts, keep):
    """The problem of a visibility table keep [nP, nC]: ring cameras, perturbed K, projections through start_kc(nC)
    with one pixel of noise; point-major observations with ascending cameras.  The start is the generating scene with
    the points moved by 0.01 N(0, 1)."""
    q0, t = _ring_cameras(nC)
    iidx, jidx = np.nonzero(keep)
    prob = dict(K=_varied_K(rng, nC), initrot=q0, cams=np.hstack([np.zeros((nC, 3)), t]), pts=pts,
                impts=np.zeros((iidx.size, 2)), iidx=iidx.astype(np.int32), jidx=jidx.astype(np.int32), nC=nC,
                nP=pts.shape[0], nO=int(iidx.size))
    prob["impts"] = lens_twin.Twin(prob, start_kc(nC)).project() + rng.standard_normal((iidx.size, 2))
    prob["pts"] = pts + 0.01 * rng.standard_normal(pts.shape)
    return prob


WIDE_COUNTS = (64, 65, 63, 1, 0)   # observations of cameras 0..4 of wide_problem: a full unit, one more, one less, one, none


def wide_problem(nC, nP=240, seed=11):
    """nC >= 16 ring cameras, nP >= 120 points in [-1, 1]^3 with few views each, so that the launch geometry changes
    with nC alone (65 cameras of 16 / 94 of 11: the first second trip of the finalize kernels' grid-stride loop) while
    the dense twin stays small.  The visibility table is drawn and then cut down to:
      * cameras 0, 1, 2, 3, 4 with exactly 64, 65, 63, 1 and 0 observations (WIDE_COUNTS),
      * the last point without any observation,
      * the first nP // 8 points (12.5 %) seen by exactly one camera, the others by at least three."""
    rng = np.random.default_rng(seed)
    assert nC >= 16 and nP >= 120
    pts = rng.uniform(-1.0, 1.0, (nP, 3))
    n1 = nP // 8
    keep = np.zeros((nP, nC), dtype=bool)
    for i in range(nP - 1):
        k = 1 if i < n1 else int(rng.integers(3, 9))
        keep[i, 5 + rng.choice(nC - 5, size=k, replace=False)] = True
    keep[:, :5] = False
    for j, n in enumerate(WIDE_COUNTS):
        keep[n1 + rng.choice(nP - 1 - n1, size=n, replace=False), j] = True
    keep[nP - 1] = False
    per_cam, per_pt = keep.sum(0), keep.sum(1)
    assert tuple(per_cam[:5]) == WIDE_COUNTS and per_pt[nP - 1] == 0
    assert (per_pt == 1).sum() >= 0.1 * nP and (per_pt == 0).sum() == 1 and np.all(per_cam[5:] > 0)
    return _scene(rng, nC, pts, keep)


def many_obs_problem(seed=13):
    """65 cameras, 6600 points with ten views each: 66 000 observations (the residual kernels' 256 x 256 threads
    first stride at 65 537), about 1000 per camera (16 units of 64) and 363 000 products on 2145 blocks (several
    default-length segments per block)."""
    rng = np.random.default_rng(seed)
    nC, nP, views = 65, 6600, 10
    pts = rng.uniform(-1.0, 1.0, (nP, 3))
    keep = np.zeros((nP, nC), dtype=bool)
    cols = np.argsort(rng.uniform(size=(nP, nC)), axis=1)[:, :views]
    keep[np.arange(nP)[:, None], cols] = True
    assert keep.sum() == nP * views > 65536
    return _scene(rng, nC, pts, keep)
