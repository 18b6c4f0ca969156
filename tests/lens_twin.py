"""Independent (test-only) numpy twin of the lens model: distortion kc = (k1..k5) and per-observation covariances.

Model (include/psba_hip.h, psba_amd/csrc/camera_model.h):
    P = R'(q) M + t, q = q_l(v) (x) q0, (x, y) = (Px, Py) / Pz, r2 = x^2 + y^2
    radial = 1 + k1 r2 + k2 r2^2 + k5 r2^3
    xd = radial x + 2 k3 x y + k4 (r2 + 2 x^2),   yd = radial y + k3 (r2 + 2 y^2) + 2 k4 x y
    u = fu xd + s yd + u0,   v = fu ar yd + v0,   e = m - (u, v)
    cost = sum e^T Sigma^-1 e;   whitened: e <- L e, A <- L A, B <- L B with L^T L = Sigma^-1, L upper triangular.

The reference has no arithmetic for either part; this twin is pinned to the CPU oracle (tests/oracle_lib.py) where
the models coincide (kc = 0, Sigma = I) and to central differences elsewhere.  A = d(u, v)/d(v0, v1, v2, t0, t1, t2)
and B = d(u, v)/dM as the oracle lays them out (2 x 6 and 2 x 3 row-major per observation); as the oracle's, they
are the derivatives of the projection (e = m - proj: the Jacobian of e is minus these).
"""
import numpy as np


def _quat(q0, v):
    """q = (sqrt(1 - |v|^2), v) (x) q0, arrays [n, 4] / [n, 3] -> s [n], u [n, 3]"""
    sl = np.sqrt(1.0 - (v * v).sum(1))
    s0, a = q0[:, 0], q0[:, 1:]
    s = sl * s0 - (a * v).sum(1)
    u = s0[:, None] * v + sl[:, None] * a + np.cross(v, a)
    return s, u, sl


def _rot(s, u):
    """R'(q) = 2 u u^T + (s^2 - |u|^2) I + 2 s [u]x, [n, 3, 3]"""
    n = s.shape[0]
    R = 2.0 * u[:, :, None] * u[:, None, :]
    R += ((s * s - (u * u).sum(1))[:, None, None]) * np.eye(3)[None]
    X = np.zeros((n, 3, 3))
    X[:, 0, 1], X[:, 0, 2], X[:, 1, 2] = -u[:, 2], u[:, 1], -u[:, 0]
    X[:, 1, 0], X[:, 2, 0], X[:, 2, 1] = u[:, 2], -u[:, 1], u[:, 0]
    return R + 2.0 * s[:, None, None] * X


def _skew(w):
    n = w.shape[0]
    X = np.zeros((n, 3, 3))
    X[:, 0, 1], X[:, 0, 2], X[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
    X[:, 1, 0], X[:, 2, 0], X[:, 2, 1] = w[:, 2], -w[:, 1], w[:, 0]
    return X


def distort(kc, x, y):
    """kc [n, 5], x, y [n] -> xd, yd, J [n, 2, 2] = d(xd, yd)/d(x, y)"""
    k1, k2, k3, k4, k5 = (kc[:, c] for c in range(5))
    r2 = x * x + y * y
    radial = 1.0 + k1 * r2 + k2 * r2 ** 2 + k5 * r2 ** 3
    xd = radial * x + 2.0 * k3 * x * y + k4 * (r2 + 2.0 * x * x)
    yd = radial * y + k3 * (r2 + 2.0 * y * y) + 2.0 * k4 * x * y
    drad = k1 + 2.0 * k2 * r2 + 3.0 * k5 * r2 ** 2  # d radial / d r2
    J = np.empty((x.shape[0], 2, 2))
    J[:, 0, 0] = radial + x * 2.0 * x * drad + 2.0 * k3 * y + k4 * 6.0 * x
    J[:, 0, 1] = x * 2.0 * y * drad + 2.0 * k3 * x + k4 * 2.0 * y
    J[:, 1, 0] = y * 2.0 * x * drad + k3 * 2.0 * x + 2.0 * k4 * y
    J[:, 1, 1] = radial + y * 2.0 * y * drad + k3 * 6.0 * y + 2.0 * k4 * x
    return xd, yd, J


def whitening(cov):
    """cov [n, 2, 2] SPD -> L [n, 2, 2] upper triangular with L^T L = cov^-1 (the library's factorisation)"""
    p, q, r = cov[:, 0, 0], 0.5 * (cov[:, 0, 1] + cov[:, 1, 0]), cov[:, 1, 1]
    det = p * r - q * q
    i00, i01, i11 = r / det, -q / det, p / det
    l00 = np.sqrt(i00)
    l01 = i01 / l00
    l11 = np.sqrt(i11 - l01 * l01)
    L = np.zeros((cov.shape[0], 2, 2))
    L[:, 0, 0], L[:, 0, 1], L[:, 1, 1] = l00, l01, l11
    return L


class Twin:
    """prob: a Problem / dict (K, initrot, cams, pts, impts, iidx, jidx); kc [nC, 5] or None; cov [nO, 2, 2] or None."""

    def __init__(self, prob, kc=None, cov=None):
        self.prob = prob
        self.nC, self.nP, self.nO = int(prob["nC"]), int(prob["nP"]), int(prob["nO"])
        self.K = np.asarray(prob["K"], dtype=np.float64).reshape(self.nC, 5)
        self.q0 = np.asarray(prob["initrot"], dtype=np.float64).reshape(self.nC, 4)
        self.m = np.asarray(prob["impts"], dtype=np.float64).reshape(self.nO, 2)
        self.i = np.asarray(prob["iidx"], dtype=np.int64)
        self.j = np.asarray(prob["jidx"], dtype=np.int64)
        self.cams = np.asarray(prob["cams"], dtype=np.float64).reshape(self.nC, 6).copy()
        self.pts = np.asarray(prob["pts"], dtype=np.float64).reshape(self.nP, 3).copy()
        self.kc = np.zeros((self.nC, 5)) if kc is None else np.asarray(kc, dtype=np.float64).reshape(self.nC, 5)
        self.L = None if cov is None else whitening(np.asarray(cov, dtype=np.float64).reshape(self.nO, 2, 2))
        self.nA, self.nB = 6 * self.nC, 3 * self.nP

    def project(self, cams=None, pts=None, jac=False):
        cams = self.cams if cams is None else np.asarray(cams).reshape(self.nC, 6)
        pts = self.pts if pts is None else np.asarray(pts).reshape(self.nP, 3)
        c, M = cams[self.j], pts[self.i]
        q0, K, kc = self.q0[self.j], self.K[self.j], self.kc[self.j]
        s, u, sl = _quat(q0, c[:, :3])
        R = _rot(s, u)
        P = np.einsum("nab,nb->na", R, M) + c[:, 3:]
        x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
        xd, yd, J = distort(kc, x, y)
        fu, u0, v0, ar, sk = (K[:, k] for k in range(5))
        proj = np.stack([fu * xd + sk * yd + u0, fu * ar * yd + v0], 1)
        if not jac:
            return proj
        Km = np.zeros((self.nO, 2, 2))
        Km[:, 0, 0], Km[:, 0, 1], Km[:, 1, 1] = fu, sk, fu * ar
        iz = 1.0 / P[:, 2]
        dxy = np.zeros((self.nO, 2, 3))
        dxy[:, 0, 0], dxy[:, 0, 2] = iz, -x * iz
        dxy[:, 1, 1], dxy[:, 1, 2] = iz, -y * iz
        D = Km @ J @ dxy                                   # d(u, v)/dP
        A = np.zeros((self.nO, 2, 6))
        A[:, :, 3:] = D
        B = D @ R
        # dq / dv_k: q_l = (sl, v), dsl/dv_k = -v_k / sl; q = q_l (x) q0 (Hamilton product, linear in q_l)
        for k in range(3):
            dql = np.zeros((self.nO, 4))
            dql[:, 0] = -c[:, k] / sl
            dql[:, 1 + k] = 1.0
            ds = dql[:, 0] * q0[:, 0] - (dql[:, 1:] * q0[:, 1:]).sum(1)
            du = q0[:, 0:1] * dql[:, 1:] + dql[:, 0:1] * q0[:, 1:] + np.cross(dql[:, 1:], q0[:, 1:])
            dR = 2.0 * (du[:, :, None] * u[:, None, :] + u[:, :, None] * du[:, None, :])
            dR += (2.0 * (s * ds - (u * du).sum(1)))[:, None, None] * np.eye(3)[None]
            dR += 2.0 * ds[:, None, None] * _skew(u) + 2.0 * s[:, None, None] * _skew(du)
            A[:, :, k] = np.einsum("nab,nb->na", D, np.einsum("nab,nb->na", dR, M))
        return proj, A, B

    def residual(self, cams=None, pts=None):
        """whitened e [nO, 2]"""
        e = self.m - self.project(cams, pts)
        return e if self.L is None else np.einsum("nab,nb->na", self.L, e)

    def cost(self, cams=None, pts=None):
        e = self.residual(cams, pts)
        return float((e * e).sum())

    def linearize(self):
        """whitened e [nO, 2], A [nO, 2, 6], B [nO, 2, 3]"""
        proj, A, B = self.project(jac=True)
        e = self.m - proj
        if self.L is not None:
            e = np.einsum("nab,nb->na", self.L, e)
            A = self.L @ A
            B = self.L @ B
        return e, A, B

    def jacobian(self):
        """dense whitened J [2 nO, nA + nB] of the projection (columns: cameras, then points)"""
        _, A, B = self.linearize()
        J = np.zeros((2 * self.nO, self.nA + self.nB))
        for a in range(self.nO):
            J[2 * a:2 * a + 2, 6 * self.j[a]:6 * self.j[a] + 6] = A[a]
            J[2 * a:2 * a + 2, self.nA + 3 * self.i[a]:self.nA + 3 * self.i[a] + 3] = B[a]
        return J

    def normal(self, mu=0.0):
        """dense weighted normal equations: N = J^T J (+ mu I), g = J^T e (the oracle's sign: the step solves N dp = g)"""
        e, _, _ = self.linearize()
        J = self.jacobian()
        N = J.T @ J + mu * np.eye(J.shape[1])
        return N, J.T @ e.reshape(-1)

    def schur(self, mu):
        """S = U* - W V*^-1 W^T and e_a = g_a - W V*^-1 g_b from the dense normal equations"""
        N, g = self.normal(mu)
        nA = self.nA
        Vinv = np.linalg.inv(N[nA:, nA:])
        W = N[:nA, nA:]
        S = N[:nA, :nA] - W @ Vinv @ W.T
        ea = g[:nA] - W @ Vinv @ g[nA:]
        return S, ea

    def step(self, mu):
        """dp of the damped system (N + mu I) dp = g"""
        N, g = self.normal(mu)
        return np.linalg.solve(N, g)


def oracle_pieces(prob, e, A, B, coeff=1.0, coeff_g=1.0, mu=None):
    """The oracle's U, V, W, g (and with mu: S, e_a, dp) from given (whitened) e, A, B: the same sums in the same
    order as the reference's kernels, with the twin's Jacobian blocks in place of the reference's."""
    import oracle_lib as ol
    o = ol.Oracle(prob)
    ex = np.ascontiguousarray(e.reshape(-1))
    JA = np.ascontiguousarray(A.reshape(-1))
    JB = np.ascontiguousarray(B.reshape(-1))
    U, V, UVdiag = np.empty(36 * o.nC), np.empty(9 * o.nP), np.empty(o.nT)
    W, g = np.empty(18 * o.nO), np.empty(o.nT)
    ol._U(o.nC, o.nO, JA, o.jidx, coeff, U, UVdiag)
    ol._V(o.nC, o.nP, o.nO, JB, o.iidx, coeff, V, UVdiag)
    ol._W(o.nO, JA, JB, coeff, W)
    ol._g(o.nC, o.nP, o.nO, coeff_g, JA, JB, o.iidx, o.jidx, ex, g)
    lin = dict(ex=ex, JA=JA, JB=JB, U=U, V=V, UVdiag=UVdiag, W=W, g=g, maxdiag=ol._maxuv(o.nT, UVdiag))
    if mu is None:
        return lin
    sch = o.schur(lin, mu)
    ret, dp, eab = o.solve(lin, sch)
    return dict(lin, S=sch["S"], ea=sch["eab"][:o.nA], dp=dp, ret=ret, Vinv=sch["Vinv"])
