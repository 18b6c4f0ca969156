"""Host reference for the per-observation camera model of psba_amd/csrc/camera_model.h, entry by entry (no GPU):
a derived bound on what one fp64 evaluation of the model's text may differ from the exact value, per output entry,
the exact values themselves from mpmath in another formulation, and the input families that stress the model.

Three number types run ONE text (linearize / residual below, operation for operation that of camera_model.h):
numpy float64 arrays (the CPU stand-in of a kernel), the error-carrying class E, and mpmath's mpf (scalars).

E holds, per observation, a value v in np.longdouble (epsilon at most 1.1e-19, as tests/dense_ref.py requires) and a
bound b with this meaning: EVERY evaluation of the same operations whose roundings are each relative and at most
u = 2^-53 + 2^-63 (as in tests/assembly_ref.py: the fp64 rounding being judged plus the extended reference's own)
lies within b of the exact value.  The fp64 kernels are such evaluations and so is v itself.  Hence, with
m(x) = |v| + 2 b >= |x^| for every such evaluation x^ (and >= |x|), the rules, one line each:
  * z = x + y:    b_z = b_x + b_y + u (|v_z| + 2 (b_x + b_y))        (propagated, plus one rounding of the computed sum)
  * z = x y:      b_z = m(x) b_y + m(y) b_x + u m(x) m(y)            (|x^ y^ - x y| <= |x^| |y^ - y| + |y| |x^ - x|)
  * z = c x, c a constant: b_z = |c| b_x (+ u |c| m(x) unless c is a power of two: scaling by 2^k is exact);
    z = x + 0.0 and z = -x are exact
  * z = x / y:    b_z = (b_x + m(x) / l(y) b_y) / l(y) + u m(x) / l(y),  l(y) = |v_y| - 2 b_y <= |y^|, |y|;
    refused (Refused is raised) where l(y) <= 0: the divisor's bound reaches its magnitude
  * z = sqrt(x):  b_z = b_x / (2 sqrt(l(x))) + u sqrt(m(x)),  l(x) = v_x - 2 b_x;  refused where l(x) <= 0
  * z = (x <= y) ? p : q:  the branch of v; where |v_x - v_y| <= 2 (b_x + b_y) an evaluation may take the other
    branch than the exact value does: b_z = 2 (b_p + b_q) + |v_p - v_q| there (the larger of the two branches plus
    their distance: Huber's weight is continuous at c^2, so this stays small)
  * fma(x, y, z) rounds once where x y + z rounds twice: contraction only removes a rounding, the bounds hold
    whichever way a compiler contracts.  (The one rounding is relative to |x^ y^ + z^|, the add's term is relative
    to |fl(x^ y^) + z^|: they differ by at most u |x^ y^|, which the product's unspent u m(x) m(y) covers.)
Second order: the rules are complete, not first-order -- every magnitude is m(.) and every divisor l(.), which
already contain the bounds -- so the factor that covers second order is 1 (SECOND_ORDER below).  The first-order
form of the issue is what remains when m(.) = l(.) = |v|.
Inputs are exact (b = 0): the doubles the kernels read.  c^2 and 1 / c^2 of the robust loss are formed on the host
in fp64 (make_robust_loss) and therefore carry their own roundings here.  The whitening factors are inputs: the
doubles tests/lens_twin.py's whitening() gives, the host's factorisation operation for operation (IEEE double
without contraction: the host code is compiled for baseline x86-64, which has no fused multiply-add).

The exact values (exact()) use mpmath at 64 digits and nothing of camera_model.h's analytic Jacobian: the rotation is
the quaternion sandwich q (0, M) q* (not the matrix), the lens model is its definition, and every derivative is
taken by forward-mode dual numbers over mpf.  The robust weight is sqrt(rho'(s)) with rho' the dual part of rho
written as the loss's definition.

W_a = c A_a^T B_a of the kernels that store it is judged against exact c A^T B with
|A|^T b_B + b_A^T |B| + gamma(3) |c| |A|^T |B| (w_bound); the gradient of a single-observation problem is
c_g J^T e with the same form (three roundings on top of the model's bounds)."""
import functools

import numpy as np

import dense_ref as dr

LD = dr.LD
LD_OK = dr.LD_OK
U = 2.0 ** -53 + 2.0 ** -63
SECOND_ORDER = 1.0
DPS = 64  # mpmath digits of the exact values
LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY, LOSS_SOFT_L1 = 0, 1, 2, 3
KD_ALL_FREE = 0x3FF
BAL_MASK = 0b0001100001  # fu, k1, k2 (capi.INTRINSICS_BAL)
NOBS = 333


def gamma(k):
    return k * U / (1.0 - k * U)


class Refused(ArithmeticError):
    """a division or square root whose operand's bound reaches its magnitude"""


def _is_pow2(c):
    m, _ = np.frexp(abs(float(c)))
    return m == 0.5


class E:
    """value and bound per observation (module docstring)"""
    __slots__ = ("v", "b")
    __array_ufunc__ = None  # ndarray op E -> E's reflected operator

    def __init__(self, v, b=None):
        self.v = np.asarray(v).astype(LD)
        self.b = np.zeros(self.v.shape, dtype=LD) if b is None else np.asarray(b).astype(LD)

    @property
    def m(self):
        return np.abs(self.v) + 2 * self.b

    @staticmethod
    def _const(o):
        return not isinstance(o, E)

    def __neg__(self):
        return E(-self.v, self.b)

    def __add__(self, o):
        if E._const(o):
            if np.ndim(o) == 0 and float(o) == 0.0:
                return self
            o = E(np.broadcast_to(np.asarray(o, dtype=np.float64), self.v.shape))
        v = self.v + o.v
        bb = self.b + o.b
        return E(v, bb + U * (np.abs(v) + 2 * bb))

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if E._const(o):
            if np.ndim(o) == 0:
                c = float(o)
                if c == 0.0:
                    return E(np.zeros(self.v.shape))
                r = 0.0 if _is_pow2(c) else U
                return E(LD(c) * self.v, abs(c) * self.b + r * abs(c) * self.m)
            o = E(np.broadcast_to(np.asarray(o, dtype=np.float64), self.v.shape))
        mx, my = self.m, o.m
        return E(self.v * o.v, mx * o.b + my * self.b + U * mx * my)

    __rmul__ = __mul__

    def __truediv__(self, o):
        if E._const(o):
            o = E(np.broadcast_to(np.asarray(o, dtype=np.float64), self.v.shape))
        low = np.abs(o.v) - 2 * o.b
        if not np.all(low > 0):
            raise Refused(f"division: the divisor's bound reaches its magnitude at {np.flatnonzero(~(low > 0))[:8]}")
        mx = self.m
        return E(self.v / o.v, (self.b + mx / low * o.b) / low + U * mx / low)

    def __rtruediv__(self, o):
        return E(np.broadcast_to(np.asarray(o, dtype=np.float64), self.v.shape)) / self

    def sqrt(self):
        low = self.v - 2 * self.b
        if not np.all(low > 0):
            raise Refused(f"sqrt: the operand's bound reaches its magnitude at {np.flatnonzero(~(low > 0))[:8]}")
        return E(np.sqrt(self.v), self.b / (2 * np.sqrt(low)) + U * np.sqrt(self.m))


def _mpf_type():
    import mpmath
    return mpmath.mpf


def sqrt(x):
    if isinstance(x, E):
        return x.sqrt()
    if isinstance(x, np.ndarray) or isinstance(x, (float, np.floating)):
        return np.sqrt(x)
    import mpmath
    return mpmath.sqrt(x)


def select_le(x, y, p, q):
    """(x <= y) ? p : q"""
    if isinstance(x, E):
        def lift(o):
            return o if isinstance(o, E) else E(np.broadcast_to(np.asarray(o, dtype=np.float64), x.v.shape))
        y, p, q = lift(y), lift(p), lift(q)
        c = x.v <= y.v
        amb = np.abs(x.v - y.v) <= 2 * (x.b + y.b)
        b = np.where(c, p.b, q.b)
        b = np.where(amb, 2 * (p.b + q.b) + np.abs(p.v - q.v), b)
        return E(np.where(c, p.v, q.v), b)
    if isinstance(x, np.ndarray):
        return np.where(x <= y, p, q)
    return p if x <= y else q


def zero_where(mask, x):
    """mask ? 0.0 : x (mask: a boolean per observation, or a Python bool)"""
    if isinstance(x, E):
        return E(np.where(mask, LD(0), x.v), np.where(mask, LD(0), x.b))
    if isinstance(x, np.ndarray):
        return np.where(mask, 0.0, x)
    return type(x)(0) if mask else x


def const_like(x, c):
    if isinstance(x, E):
        return E(np.full(x.v.shape, c, dtype=np.float64))
    if isinstance(x, np.ndarray):
        return np.full(x.shape, c, dtype=np.float64)
    return type(x)(c)


# ---- the model's text (camera_model.h, operation for operation) ------------------------------------------------------

def _pose(q0, cam, M, mutate=None):
    """compose_quat, quat_matrix, P = R M + t and the reciprocal"""
    v0, v1, v2 = cam[0], cam[1], cam[2]
    sl = sqrt(1.0 - v0 * v0 - v1 * v1 - v2 * v2)
    s0, a0, a1, a2 = q0
    qs = sl * s0 - (a0 * v0 + a1 * v1 + a2 * v2)
    u0 = s0 * v0 + sl * a0 + a2 * v1 - a1 * v2
    u1 = s0 * v1 + sl * a1 + a0 * v2 - a2 * v0
    u2 = s0 * v2 + sl * a2 + a1 * v0 - a0 * v1
    ss, x, y, z = qs * qs, u0, u1, u2
    xx, yy, zz = x * x, y * y, z * z
    R = [None] * 9
    R[0] = ss + xx - yy - zz
    R[4] = ss - xx + yy - zz
    R[8] = ss - xx - yy + zz
    xy, xz, yz, sx, sy, sz = x * y, x * z, y * z, qs * x, qs * y, qs * z
    R[1] = 2.0 * (xy - sz)
    R[2] = 2.0 * (xz + sy)
    R[3] = 2.0 * (xy + sz)
    R[5] = 2.0 * (yz - sx)
    R[6] = 2.0 * (xz - sy)
    R[7] = 2.0 * (yz + sx)
    Px = R[0] * M[0] + R[1] * M[1] + R[2] * M[2] + cam[3]
    Py = R[3] * M[0] + R[4] * M[1] + R[5] * M[2] + cam[4]
    Pz = R[6] * M[0] + R[7] * M[1] + R[8] * M[2] + cam[5]
    inv = 1.0 / Pz
    if mutate == "recip":  # the mutation check of tests/test_camera_ref.py: a reciprocal 2^-48 off
        inv = inv * (1.0 + 2.0 ** -48)
    return sl, (qs, u0, u1, u2), R, (Px, Py, Pz), inv


def _rot_columns(q0, cam, M, sl, q, D):
    """the rotation columns of A: dP / dv_k, then D dP (D row-major 2 x 3)"""
    qs, u0, u1, u2 = q
    s0, a0, a1, a2 = q0
    isl = 1.0 / sl
    udM = u0 * M[0] + u1 * M[1] + u2 * M[2]
    c0 = u1 * M[2] - u2 * M[1]
    c1 = u2 * M[0] - u0 * M[2]
    c2 = u0 * M[1] - u1 * M[0]
    top, bot = [], []
    for k in range(3):
        dsl = -cam[k] * isl
        ak = (a0, a1, a2)[k]
        ds = dsl * s0 - ak
        x0 = (0.0, a2, -a1)[k]
        x1 = (-a2, 0.0, a0)[k]
        x2 = (a1, -a0, 0.0)[k]
        du0 = (s0 if k == 0 else 0.0) + dsl * a0 + x0
        du1 = (s0 if k == 1 else 0.0) + dsl * a1 + x1
        du2 = (s0 if k == 2 else 0.0) + dsl * a2 + x2
        dudM = du0 * M[0] + du1 * M[1] + du2 * M[2]
        udu = u0 * du0 + u1 * du1 + u2 * du2
        g = qs * ds - udu
        m0 = du1 * M[2] - du2 * M[1]
        m1 = du2 * M[0] - du0 * M[2]
        m2 = du0 * M[1] - du1 * M[0]
        dP0 = 2.0 * (du0 * udM + u0 * dudM + g * M[0] + ds * c0 + qs * m0)
        dP1 = 2.0 * (du1 * udM + u1 * dudM + g * M[1] + ds * c1 + qs * m1)
        dP2 = 2.0 * (du2 * udM + u2 * dudM + g * M[2] + ds * c2 + qs * m2)
        if D[3] is None:  # linearize_obs: d10 is a structural zero
            top.append(D[0] * dP0 + D[1] * dP1 + D[2] * dP2)
            bot.append(D[4] * dP1 + D[5] * dP2)
        else:
            top.append(D[0] * dP0 + D[1] * dP1 + D[2] * dP2)
            bot.append(D[3] * dP0 + D[4] * dP1 + D[5] * dP2)
    return top, bot


def residual_obs(K, q0, cam, M, m, mutate=None):
    _, _, _, (Px, Py, Pz), inv = _pose(q0, cam, M, mutate)
    e0 = m[0] - (K[0] * Px + K[4] * Py + K[1] * Pz) * inv
    e1 = m[1] - (K[0] * K[3] * Py + K[2] * Pz) * inv
    return [e0, e1]


def linearize_obs(K, q0, cam, M, m, mutate=None):
    """-> e [2], A [12], B [6], xn [2]"""
    sl, q, R, (Px, Py, Pz), inv = _pose(q0, cam, M, mutate)
    x = (K[0] * Px + K[4] * Py + K[1] * Pz) * inv
    y = (K[0] * K[3] * Py + K[2] * Pz) * inv
    e = [m[0] - x, m[1] - y]
    xn = [Px * inv, Py * inv]
    d00, d01, d02 = K[0] * inv, K[4] * inv, (K[1] - x) * inv
    d11, d12 = K[0] * K[3] * inv, (K[2] - y) * inv
    A = [None] * 12
    A[3], A[4], A[5] = d00, d01, d02
    A[9] = const_like(inv, 0.0)
    A[10], A[11] = d11, d12
    B = [d00 * R[0] + d01 * R[3] + d02 * R[6],
         d00 * R[1] + d01 * R[4] + d02 * R[7],
         d00 * R[2] + d01 * R[5] + d02 * R[8],
         d11 * R[3] + d12 * R[6],
         d11 * R[4] + d12 * R[7],
         d11 * R[5] + d12 * R[8]]
    top, bot = _rot_columns(q0, cam, M, sl, q, [d00, d01, d02, None, d11, d12])
    A[0:3] = top
    A[6:9] = bot
    return e, A, B, xn


def distort(kc, x, y, jac=False, mutate=None):
    r2 = x * x + y * y
    radial = 1.0 + r2 * (kc[0] + r2 * (kc[1] + r2 * kc[4]))
    xy = x * y
    xd = radial * x + 2.0 * kc[2] * xy + kc[3] * (r2 + 2.0 * x * x)
    yd = radial * y + kc[2] * (r2 + 2.0 * y * y) + 2.0 * kc[3] * xy
    if not jac:
        return xd, yd, None
    dr = kc[0] + r2 * (2.0 * kc[1] + 3.0 * kc[4] * r2)
    six = 2.0 if mutate == "k4" else 6.0  # the mutation check: 6 k4 x written as 2 k4 x
    J = [radial + 2.0 * x * x * dr + 2.0 * kc[2] * y + six * kc[3] * x,
         2.0 * xy * dr + 2.0 * kc[2] * x + 2.0 * kc[3] * y,
         2.0 * xy * dr + 2.0 * kc[2] * x + 2.0 * kc[3] * y,
         radial + 2.0 * y * y * dr + 6.0 * kc[2] * y + 2.0 * kc[3] * x]
    return xd, yd, J


def residual_obs_dist(K, q0, cam, M, kc, m, mutate=None):
    _, _, _, (Px, Py, Pz), inv = _pose(q0, cam, M, mutate)
    xd, yd, _ = distort(kc, Px * inv, Py * inv)
    e0 = m[0] - (K[0] * xd + K[4] * yd + K[1])
    e1 = m[1] - (K[0] * K[3] * yd + K[2])
    return [e0, e1]


def linearize_obs_dist(K, q0, cam, M, kc, m, mutate=None):
    """-> e [2], A [12], B [6], (x, y, xd, yd)"""
    sl, q, R, (Px, Py, Pz), inv = _pose(q0, cam, M, mutate)
    x, y = Px * inv, Py * inv
    xd, yd, J = distort(kc, x, y, True, mutate)
    e = [m[0] - (K[0] * xd + K[4] * yd + K[1]), m[1] - (K[0] * K[3] * yd + K[2])]
    fa = K[0] * K[3]
    g00, g01 = K[0] * J[0] + K[4] * J[2], K[0] * J[1] + K[4] * J[3]
    g10, g11 = fa * J[2], fa * J[3]
    D = [g00 * inv, g01 * inv, -(g00 * x + g01 * y) * inv, g10 * inv, g11 * inv, -(g10 * x + g11 * y) * inv]
    A = [None] * 12
    B = [None] * 6
    for r in range(2):
        A[6 * r + 3], A[6 * r + 4], A[6 * r + 5] = D[3 * r], D[3 * r + 1], D[3 * r + 2]
        for c in range(3):
            B[3 * r + c] = D[3 * r] * R[c] + D[3 * r + 1] * R[3 + c] + D[3 * r + 2] * R[6 + c]
    top, bot = _rot_columns(q0, cam, M, sl, q, D)
    A[0:3] = top
    A[6:9] = bot
    return e, A, B, (x, y, xd, yd)


def linearize_obs_freek(p, q0, M, m, mutate=None):
    """p = (fu, u0, v0, ar, s | v | t) -> e [2], A [22], B [6]"""
    e, A6, B, xn = linearize_obs(p[:5], q0, p[5:], M, m, mutate)
    one, zero = const_like(xn[0], 1.0), const_like(xn[0], 0.0)
    A = [xn[0], one, zero, zero, xn[1]] + A6[0:6] + [p[3] * xn[1], zero, one, p[0] * xn[1], zero] + A6[6:12]
    return e, A, B


def linearize_obs_freekd(p, q0, M, m, free_mask=KD_ALL_FREE, mutate=None):
    """p = (fu, u0, v0, ar, s | k1..k5 | v | t) -> e [2], A [32], B [6]"""
    e, A6, B, (x, y, xd, yd) = linearize_obs_dist(p[:5], q0, p[10:], M, p[5:10], m, mutate)
    # (the kernel forms x, y, xd, yd once more from the same operations: the same values, the same bounds)
    r2, xy2 = x * x + y * y, 2.0 * x * y
    dxd = [r2 * x, r2 * r2 * x, xy2, r2 + 2.0 * x * x, r2 * r2 * r2 * x]
    dyd = [r2 * y, r2 * r2 * y, r2 + 2.0 * y * y, xy2, r2 * r2 * r2 * y]
    fa = p[0] * p[3]
    one, zero = const_like(x, 1.0), const_like(x, 0.0)
    top = [xd, one, zero, zero, yd] + [p[0] * dxd[k] + p[4] * dyd[k] for k in range(5)]
    bot = [p[3] * yd, zero, one, p[0] * yd, zero] + [fa * dyd[k] for k in range(5)]
    for k in range(10):
        if not (free_mask >> k) & 1:
            top[k], bot[k] = zero, zero
    return e, top + A6[0:6] + bot + A6[6:12], B


def whiten2(w, e0, e1):
    return w[0] * e0 + w[1] * e1, w[2] * e1


def robust_weight(loss, s):
    """w of robust_eval; loss = (kind, c) with c a number of s's type"""
    kind, c = loss
    c2 = c * c
    ic2 = 1.0 / c2
    if kind == LOSS_HUBER:
        r = sqrt(s)
        return select_le(s, c2, 1.0, sqrt(c / r))
    if kind == LOSS_CAUCHY:
        return 1.0 / sqrt(1.0 + s * ic2)
    if kind == LOSS_SOFT_L1:
        return 1.0 / sqrt(sqrt(1.0 + s * ic2))
    return const_like(s, 1.0)


def linearize(x, mutate=None):
    """lens_linearize + fix_mask (blocks of 6) or linearize_obs_freek / _freekd (blocks of 11 / 16) on the inputs x
    (gather() below): -> e [2], A [2 cnp], B [6]."""
    cnp = x["cnp"]
    if cnp == 11:
        return linearize_obs_freek(x["K"] + x["cam"], x["q0"], x["M"], x["m"], mutate)
    if cnp == 16:
        return linearize_obs_freekd(x["K"] + x["kc"] + x["cam"], x["q0"], x["M"], x["m"], x["free_mask"], mutate)
    if x["kc"] is not None:
        e, A, B, _ = linearize_obs_dist(x["K"], x["q0"], x["cam"], x["M"], x["kc"], x["m"], mutate)
    else:
        e, A, B, _ = linearize_obs(x["K"], x["q0"], x["cam"], x["M"], x["m"], mutate)
    if x["L"] is not None:  # whiten_obs
        w = x["L"]
        e = list(whiten2(w, e[0], e[1]))
        for k in range(6):
            A[k], A[6 + k] = whiten2(w, A[k], A[6 + k])
        for k in range(3):
            B[k], B[3 + k] = whiten2(w, B[k], B[3 + k])
    if x["loss"] is not None:  # robust_scale
        w = robust_weight(x["loss"], e[0] * e[0] + e[1] * e[1])
        e = [e[0] * w, e[1] * w]
        A = [a * w for a in A]
        B = [b * w for b in B]
    if x["fix"] is not None:  # fix_mask
        fc, fp = x["fix"]
        A = [zero_where(fc, a) for a in A]
        B = [zero_where(fp, b) for b in B]
    return e, A, B


def residual(x, mutate=None):
    """lens_residual + lens_cost (k_residual): -> e [2] (whitened, weighted), s = |L e|^2"""
    if x["kc"] is not None:
        e = residual_obs_dist(x["K"], x["q0"], x["cam"], x["M"], x["kc"], x["m"], mutate)
    else:
        e = residual_obs(x["K"], x["q0"], x["cam"], x["M"], x["m"], mutate)
    if x["L"] is not None:
        e = list(whiten2(x["L"], e[0], e[1]))
    s = e[0] * e[0] + e[1] * e[1]
    if x["loss"] is not None:
        w = robust_weight(x["loss"], s)
        e = [e[0] * w, e[1] * w]
    return e, s


# ---- inputs ---------------------------------------------------------------------------------------------------------

def gather(case, kind="f64", cnp=6, free_mask=KD_ALL_FREE, cams=None, pts=None, sel=None):
    """The per-observation inputs of a case (families() below) as lists of numbers of one type: kind "f64" (numpy
    arrays), "E" (error-carrying) or "raw" (float64 arrays for exact()).  cams [nC, 6], pts [nP, 3]: other parameters
    than the problem's own; sel: a subset of the observations."""
    prob = case["prob"]
    i = np.asarray(prob["iidx"], dtype=np.int64)
    j = np.asarray(prob["jidx"], dtype=np.int64)
    if sel is not None:
        i, j = i[sel], j[sel]
    lift = (lambda a: E(a)) if kind == "E" else (lambda a: np.ascontiguousarray(a, dtype=np.float64))

    def cols(a, idx):
        a = np.asarray(a, dtype=np.float64)
        return [lift(a[idx, k]) for k in range(a.shape[1])]
    m = np.asarray(prob["impts"], dtype=np.float64).reshape(-1, 2)
    x = dict(cnp=cnp, free_mask=free_mask, kc=None, L=None, loss=None, fix=None)
    x["K"] = cols(prob["K"], j)
    x["q0"] = cols(prob["initrot"], j)
    x["cam"] = cols(np.asarray(prob["cams"] if cams is None else cams).reshape(-1, 6), j)
    x["M"] = cols(np.asarray(prob["pts"] if pts is None else pts).reshape(-1, 3), i)
    x["m"] = cols(m if sel is None else m[sel], slice(None))
    kc = case.get("kc")
    if cnp == 16:
        kc = np.zeros((int(prob["nC"]), 5)) if kc is None else kc
    if kc is not None and cnp != 11:
        x["kc"] = cols(kc, j)
    if cnp != 6:
        return x
    if case.get("cov") is not None:
        from lens_twin import whitening
        Lm = whitening(np.asarray(case["cov"], dtype=np.float64).reshape(-1, 2, 2))
        Lm = Lm if sel is None else Lm[sel]
        x["L"] = [lift(Lm[:, 0, 0]), lift(Lm[:, 0, 1]), lift(Lm[:, 1, 1])]
    if case.get("loss") is not None:
        lk, c = case["loss"]
        x["loss"] = (lk, lift(np.full(i.shape, float(c))) if kind != "raw" else float(c))
    if case.get("fixed_cams") is not None or case.get("fixed_pts") is not None:
        fc = np.zeros(int(prob["nC"]), bool) if case.get("fixed_cams") is None else np.asarray(case["fixed_cams"]) != 0
        fp = np.zeros(int(prob["nP"]), bool) if case.get("fixed_pts") is None else np.asarray(case["fixed_pts"]) != 0
        x["fix"] = (fc[j], fp[i])
    return x


def stack(vals):
    """list of per-observation numbers -> (value [n, k] in extended precision, bound [n, k] or None)"""
    if isinstance(vals[0], E):
        return np.stack([t.v for t in vals], 1), SECOND_ORDER * np.stack([t.b for t in vals], 1).astype(np.float64)
    return np.stack([np.asarray(t, dtype=np.float64) for t in vals], 1), None


def atb_bound(A, bA, B, bB, c):
    """exact c A^T B [n, p, q] from exact A [n, 2, p], B [n, 2, q] (extended precision) and the bound for a kernel that
    forms it from its own A^ and B^ with two products, one add and the scaling (three roundings on a term's path):
    |c| (|A^|^T b_B + b_A^T |B|) + gamma(3) |c| |A^|^T |B^|, with |A^| <= |A| + b_A and |B^| <= |B| + b_B"""
    aA, aB = np.abs(A.astype(np.float64)), np.abs(B.astype(np.float64))
    X = LD(c) * np.einsum("aki,akj->aij", A, B)
    bound = abs(c) * (np.einsum("aki,akj->aij", aA + bA, bB) + np.einsum("aki,akj->aij", bA, aB)
                      + gamma(3) * np.einsum("aki,akj->aij", aA + bA, aB + bB))
    return X, bound


def w_bound(A, bA, B, bB, coeff, cnp):
    """W_a = c A_a^T B_a [n, cnp, 3] and its bound from the flat blocks A [n, 2 cnp], B [n, 6]"""
    return atb_bound(A.reshape(-1, 2, cnp), bA.reshape(-1, 2, cnp), B.reshape(-1, 2, 3), bB.reshape(-1, 2, 3), coeff)


def gradient_bound(J, bJ, e, be, c_g, p):
    """c_g J_a^T e_a [n, p] of a single observation and its bound (J flat [n, 2 p], e [n, 2])"""
    g, b = atb_bound(J.reshape(-1, 2, p), bJ.reshape(-1, 2, p), e.reshape(-1, 2, 1), be.reshape(-1, 2, 1), c_g)
    return g[:, :, 0], b[:, :, 0]


# ---- the exact values -------------------------------------------------------------------------------------------------

class _Dual:
    """forward-mode dual number over mpf with a sparse derivative {direction: mpf}"""
    __slots__ = ("v", "d")

    def __init__(self, v, d=None):
        self.v = v
        self.d = {} if d is None else d

    @staticmethod
    def lift(o):
        return o if isinstance(o, _Dual) else _Dual(_mpf_type()(o))

    def __neg__(self):
        return _Dual(-self.v, {k: -g for k, g in self.d.items()})

    def __add__(self, o):
        o = _Dual.lift(o)
        d = dict(self.d)
        for k, g in o.d.items():
            d[k] = d[k] + g if k in d else g
        return _Dual(self.v + o.v, d)

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-_Dual.lift(o))

    def __rsub__(self, o):
        return _Dual.lift(o) + (-self)

    def __mul__(self, o):
        o = _Dual.lift(o)
        d = {k: g * o.v for k, g in self.d.items()}
        for k, g in o.d.items():
            d[k] = d[k] + self.v * g if k in d else self.v * g
        return _Dual(self.v * o.v, d)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _Dual.lift(o)
        z = self.v / o.v
        d = {k: g / o.v for k, g in self.d.items()}
        for k, g in o.d.items():
            t = -z * g / o.v
            d[k] = d[k] + t if k in d else t
        return _Dual(z, d)

    def __rtruediv__(self, o):
        return _Dual.lift(o) / self


def _dsqrt(x):
    import mpmath
    r = mpmath.sqrt(x.v)
    return _Dual(r, {k: g / (2 * r) for k, g in x.d.items()})


def _dlog(x):
    import mpmath
    return _Dual(mpmath.log(x.v), {k: g / x.v for k, g in x.d.items()})


def _hamilton(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0])


def _rho_prime(kind, c, s):
    """rho'(s) of the loss's definition (camera_model.h's table), by a dual number in s"""
    import mpmath
    one = mpmath.mpf(1)
    sd = _Dual(s, {0: one})
    c2 = c * c
    if kind == LOSS_HUBER:
        rho = sd if s <= c2 else 2 * c * _dsqrt(sd) - c2
    elif kind == LOSS_CAUCHY:
        rho = c2 * _dlog(1 + sd / c2)
    elif kind == LOSS_SOFT_L1:
        rho = 2 * c2 * (_dsqrt(1 + sd / c2) - 1)
    else:
        rho = sd
    return rho.d[0]


def _to_ld(x):
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


_EXT = ["r0", "r1", "r2", "t0", "t1", "t2"]  # the local rotation v (named r here: v0 is the principal point) and t
ORDER = {6: _EXT, 11: ["fu", "u0", "v0", "ar", "sk"] + _EXT,
         16: ["fu", "u0", "v0", "ar", "sk", "k1", "k2", "k3", "k4", "k5"] + _EXT}


def _exact_one(K, q0, cam, M, m, kc, L, loss, order):
    """one observation: the projection as a dual number in the directions `order` names;
    -> e [2], J [2][len(order)] (whitened, weighted), s (whitened, unweighted)"""
    import mpmath
    mpf = mpmath.mpf
    vals = dict(fu=K[0], u0=K[1], v0=K[2], ar=K[3], sk=K[4])
    for t in range(5):
        vals[f"k{t + 1}"] = kc[t] if kc is not None else 0.0
    for t in range(3):
        vals[f"r{t}"], vals[f"t{t}"], vals[f"M{t}"] = cam[t], cam[3 + t], M[t]
    P = {k: _Dual(mpf(float(v)), {order.index(k): mpf(1)} if k in order else None) for k, v in vals.items()}
    v = [P["r0"], P["r1"], P["r2"]]
    ql = (_dsqrt(1 - v[0] * v[0] - v[1] * v[1] - v[2] * v[2]), v[0], v[1], v[2])
    q = _hamilton(ql, tuple(_Dual(mpf(float(t))) for t in q0))
    conj = (q[0], -q[1], -q[2], -q[3])
    rot = _hamilton(_hamilton(q, (_Dual(mpf(0)), P["M0"], P["M1"], P["M2"])), conj)  # q (0, M) q*
    Pc = [rot[1 + t] + P[f"t{t}"] for t in range(3)]
    x, y = Pc[0] / Pc[2], Pc[1] / Pc[2]
    if kc is not None:
        r2 = x * x + y * y
        radial = 1 + P["k1"] * r2 + P["k2"] * r2 * r2 + P["k5"] * r2 * r2 * r2
        xd = x * radial + 2 * P["k3"] * x * y + P["k4"] * (r2 + 2 * x * x)
        yd = y * radial + P["k3"] * (r2 + 2 * y * y) + 2 * P["k4"] * x * y
    else:
        xd, yd = x, y
    pu = P["fu"] * xd + P["sk"] * yd + P["u0"]
    pv = P["fu"] * P["ar"] * yd + P["v0"]
    nd = len(order)
    e = [mpf(float(m[0])) - pu.v, mpf(float(m[1])) - pv.v]
    J = [[pu.d.get(t, mpf(0)) for t in range(nd)], [pv.d.get(t, mpf(0)) for t in range(nd)]]
    if L is not None:
        l00, l01, l11 = (mpf(float(t)) for t in L)
        e = [l00 * e[0] + l01 * e[1], l11 * e[1]]
        J = [[l00 * a + l01 * b for a, b in zip(J[0], J[1])], [l11 * b for b in J[1]]]
    s = e[0] * e[0] + e[1] * e[1]
    if loss is not None:
        w = mpmath.sqrt(_rho_prime(loss[0], mpf(float(loss[1])), s))
        e = [w * e[0], w * e[1]]
        J = [[w * a for a in row] for row in J]
    return e, J, s


def exact(x):
    """The exact e [n, 2], A [n, 2 cnp], B [n, 6], s [n] (the whitened squared residual, unweighted) of the inputs
    x = gather(case, "raw", ...), in extended precision (each the nearest long double of the 64-digit value).
    The fixed mask and the intrinsics mask zero their entries afterwards, as the model defines them."""
    import mpmath
    cnp = x["cnp"]
    n = x["m"][0].shape[0]
    order = ORDER[cnp] + ["M0", "M1", "M2"]
    e = np.zeros((n, 2), dtype=LD)
    A = np.zeros((n, 2, cnp), dtype=LD)
    B = np.zeros((n, 2, 3), dtype=LD)
    s = np.zeros(n, dtype=LD)
    with mpmath.workdps(DPS):
        for a in range(n):
            at = lambda lst: None if lst is None else [t[a] for t in lst]
            ea, Ja, sa = _exact_one(at(x["K"]), at(x["q0"]), at(x["cam"]), at(x["M"]), at(x["m"]), at(x["kc"]),
                                    at(x["L"]), x["loss"], order)
            e[a] = [_to_ld(t) for t in ea]
            for r in range(2):
                A[a, r] = [_to_ld(t) for t in Ja[r][:cnp]]
                B[a, r] = [_to_ld(t) for t in Ja[r][cnp:]]
            s[a] = _to_ld(sa)
    if cnp == 16:
        for k in range(10):
            if not (x["free_mask"] >> k) & 1:
                A[:, :, k] = 0
    if x["fix"] is not None:
        fc, fp = x["fix"]
        A[fc] = 0
        B[fp] = 0
    return e, A.reshape(n, 2 * cnp), B.reshape(n, 6), s


def at_mpf(x, a):
    """observation a of x = gather(case, "raw", ...) as mpf scalars: the text over mpmath"""
    import mpmath
    one = lambda lst: None if lst is None else [mpmath.mpf(float(t[a])) for t in lst]
    y = dict(x)
    for k in ("K", "q0", "cam", "M", "m", "kc", "L"):
        y[k] = one(x[k])
    if x["loss"] is not None:
        y["loss"] = (x["loss"][0], mpmath.mpf(float(x["loss"][1])))
    if x["fix"] is not None:
        y["fix"] = (bool(x["fix"][0][a]), bool(x["fix"][1][a]))
    return y


# ---- input families ---------------------------------------------------------------------------------------------------
# Every family is one problem of nC = 9 cameras, nP = 111 points and nO = 333 observations (not a multiple of 64):
# camera 0 sees the points 0 .. 64 (65 observations: more than a wave), every point is seen by three cameras.

FAMILIES = ("benign", "far", "near", "rot", "dist", "cov", "robust-huber", "robust-cauchy", "robust-softl1", "fixed")
N_CAMS, N_PTS = 9, 111
ROBUST_C = 1.7  # c^2 and 1 / c^2 are not representable: the host's roundings of them count


def _qmul(a, b):
    return np.array(_hamilton(a, b))


def _qrot(q):
    s, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                     [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                     [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]])


def _pattern(rng):
    iidx = np.repeat(np.arange(N_PTS, dtype=np.int32), 3)
    jidx = np.empty(3 * N_PTS, dtype=np.int32)
    for i in range(N_PTS):
        if i < 65:
            jidx[3 * i:3 * i + 3] = np.r_[0, np.sort(rng.choice(np.arange(1, N_CAMS), 2, replace=False))]
        else:
            jidx[3 * i:3 * i + 3] = np.sort(rng.choice(np.arange(1, N_CAMS), 3, replace=False))
    return iidx, jidx


def _unit(rng, n=3):
    v = rng.normal(size=n)
    return v / np.linalg.norm(v)


def _geometry(rng, vs, depth, centre, lateral, thick, tilt):
    """Cameras whose composed rotation q_l(v_j) (x) q0_j is a rotation by at most `tilt` away from one random rotation,
    points M = centre + (lateral, lateral, thick) in that rotation's frame, t_j such that P = R_j (M - centre) +
    (0, 0, depth_j).  vs [nC, 3]: the local rotations (q0 is chosen to match)."""
    base = _unit(rng, 4)
    Rb = _qrot(base)
    q0 = np.empty((N_CAMS, 4))
    cams = np.empty((N_CAMS, 6))
    for j in range(N_CAMS):
        ang = tilt * rng.random()
        dq = np.r_[np.cos(ang / 2), np.sin(ang / 2) * _unit(rng)]
        qt = _qmul(dq, base)
        v = vs[j]
        ql = np.r_[np.sqrt(1.0 - v @ v), v]
        q0[j] = _qmul(np.r_[ql[0], -ql[1:]] / (ql @ ql), qt)  # q_l^-1 (x) q_t
        cams[j, :3] = v
        cams[j, 3:] = -_qrot(qt) @ centre + np.r_[0.0, 0.0, depth[j]]
    loc = np.stack([lateral * rng.uniform(-1, 1, N_PTS), lateral * rng.uniform(-1, 1, N_PTS),
                    thick * rng.random(N_PTS)], 1)
    pts = centre[None, :] + loc @ Rb
    return q0, cams, pts


def _small_v(rng):
    return 1e-3 * rng.normal(size=(N_CAMS, 3))


@functools.lru_cache(maxsize=None)
def family(name):
    """-> dict(prob=Problem-like dict, kc [nC, 5] | None, cov [nO, 2, 2] | None, loss (kind, c) | None,
    fixed_cams [nC] | None, fixed_pts [nP] | None)"""
    rng = np.random.default_rng([20260, FAMILIES.index(name)])
    iidx, jidx = _pattern(rng)
    nO = iidx.size
    assert nO == NOBS and np.bincount(jidx)[0] == 65
    K = np.stack([1000.0 * (1 + 0.1 * rng.uniform(-1, 1, N_CAMS)), 500 + 50 * rng.normal(size=N_CAMS),
                  400 + 50 * rng.normal(size=N_CAMS), 1 + 0.05 * rng.uniform(-1, 1, N_CAMS),
                  2.0 * rng.uniform(-1, 1, N_CAMS)], 1)
    case = dict(kc=None, cov=None, loss=None, fixed_cams=None, fixed_pts=None)
    ten = np.full(N_CAMS, 10.0) + rng.uniform(-1, 1, N_CAMS)
    zero = np.zeros(3)
    if name == "far":  # |M|, |t| of 1e2 to 1e4 depths
        depth = np.geomspace(2.0, 200.0, N_CAMS)
        q0, cams, pts = _geometry(rng, _small_v(rng), depth, 2e4 * _unit(rng), 1.0, 1.0, 0.05)
    elif name == "near":  # depth 1e-2 of the scene scale, projections up to ~1e5 px off centre
        depth = 0.01 * (1 + 0.2 * rng.random(N_CAMS))
        q0, cams, pts = _geometry(rng, _small_v(rng), depth, 1.0 * _unit(rng), 1.0, 0.005, 1e-3)
    elif name == "rot":  # |v| in {0, one component 0, 0.9, 0.999, 1 - 1e-6}
        mags = [0.0, 0.36, 0.9, 0.999, 1 - 1e-6, 0.9, 0.999, 1 - 1e-6, 0.5]
        vs = np.stack([mg * _unit(rng) for mg in mags])
        vs[1, 1] = 0.0
        vs[8, 0] = 0.0
        q0, cams, pts = _geometry(rng, vs, ten, zero, 1.0, 1.0, np.pi)
    elif name == "dist":  # r2 up to 2; radial and the 2 x 2 J come near zero; camera 8 has kc = 0 exactly
        q0, cams, pts = _geometry(rng, _small_v(rng), ten, zero, 10.5, 1.0, 0.02)
        kc = np.stack([rng.uniform(-0.52, -0.46, N_CAMS), 0.03 * rng.uniform(-1, 1, N_CAMS),
                       0.01 * rng.uniform(-1, 1, N_CAMS), 0.01 * rng.uniform(-1, 1, N_CAMS),
                       0.005 * rng.uniform(-1, 1, N_CAMS)], 1)
        kc[8] = 0.0
        case["kc"] = kc
    else:  # the geometry of the bundled sets: cameras ten units from a unit ball of points, any orientation
        q0, cams, pts = _geometry(rng, _small_v(rng), ten, zero, 1.0, 1.0, np.pi)
    prob = dict(K=K, initrot=q0, cams=cams, pts=pts, iidx=iidx, jidx=jidx, nC=N_CAMS, nP=N_PTS, nO=nO,
                impts=np.zeros((nO, 2)))
    case["prob"] = prob
    if name == "fixed":  # every model bit at once: mild distortion and covariances, Huber, a third of each kind fixed
        case["kc"] = np.stack([0.05 * rng.uniform(-1, 1, N_CAMS), 0.01 * rng.uniform(-1, 1, N_CAMS),
                               1e-3 * rng.uniform(-1, 1, N_CAMS), 1e-3 * rng.uniform(-1, 1, N_CAMS),
                               1e-3 * rng.uniform(-1, 1, N_CAMS)], 1)
        case["fixed_cams"] = (np.arange(N_CAMS) % 3 == 0).astype(np.uint8)
        case["fixed_pts"] = (np.arange(N_PTS) % 3 == 1).astype(np.uint8)
        case["loss"] = (LOSS_HUBER, ROBUST_C)
    # measurements: the fp64 projection plus noise
    x = gather(dict(prob=prob, kc=case["kc"]), "f64")
    e, _ = residual(x)
    proj = -np.stack(e, 1)
    noise = rng.normal(size=(nO, 2))
    if name.startswith("robust"):  # s / c^2 from 1e-12 to 1e12; a tenth within 1e-9 relative of Huber's boundary
        kind = {"robust-huber": LOSS_HUBER, "robust-cauchy": LOSS_CAUCHY, "robust-softl1": LOSS_SOFT_L1}[name]
        case["loss"] = (kind, ROBUST_C)
        r = ROBUST_C * 10.0 ** rng.uniform(-6, 6, nO)
        edge = np.arange(nO) % 10 == 0
        r[edge] = ROBUST_C * (1 + rng.choice([-1e-9, -1e-12, 0.0, 1e-12, 1e-9], int(edge.sum())))
        noise = r[:, None] * np.stack([_unit(rng, 2) for _ in range(nO)])
    prob["impts"] = proj + noise
    if name in ("cov", "fixed"):  # cov: condition 1e8 and l01 != 0
        s1, s2 = (100.0, 0.01) if name == "cov" else (2.0, 0.7)
        th = rng.uniform(0.2, 1.3, nO)
        Q = np.stack([np.stack([np.cos(th), -np.sin(th)], 1), np.stack([np.sin(th), np.cos(th)], 1)], 1)
        cov = Q @ np.diag([s1 * s1, s2 * s2])[None] @ Q.transpose(0, 2, 1)
        case["cov"] = 0.5 * (cov + cov.transpose(0, 2, 1))
    return case


def single_observation(case, n):
    """The problem nC = nP = nO = n whose observation a joins camera a to point a: the first n observations of a
    family, each with a copy of its camera and of its point (every K1 sum has one term)."""
    prob = case["prob"]
    i, j = np.asarray(prob["iidx"])[:n], np.asarray(prob["jidx"])[:n]
    ar = np.arange(n, dtype=np.int32)
    out = dict(case)
    out["prob"] = dict(K=np.asarray(prob["K"])[j], initrot=np.asarray(prob["initrot"])[j], cams=np.asarray(prob["cams"])[j],
                       pts=np.asarray(prob["pts"])[i], impts=np.asarray(prob["impts"])[:n], iidx=ar, jidx=ar.copy(),
                       nC=n, nP=n, nO=n)
    if case.get("kc") is not None:
        out["kc"] = np.asarray(case["kc"])[j]
    if case.get("cov") is not None:
        out["cov"] = np.asarray(case["cov"])[:n]
    return out
