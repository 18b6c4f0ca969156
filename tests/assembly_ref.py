"""Host reference for the normal-equation kernels K1 (U, V, W, g), K2 (V*^-1, Y, S, e_a) and K3 (e_b, dp_b and the try
scalars), entry by entry (no GPU).

Every function takes fp64 inputs and returns, per quantity, the exact result of the same operation (kept in extended
precision) and an envelope of the same shape: the check is |got - exact| <= bound for EVERY entry, the bound built from
that entry's own envelope -- never from the maximum of an array.  Extended precision is np.longdouble (its epsilon
must be at most 1.1e-19, as tests/dense_ref.py requires); the reference is then itself rounded, with unit roundoff
2^-64 per operation and the same operation counts as the fp64 kernels, so every gamma below uses
u = 2^-53 + 2^-63, which covers both the fp64 rounding being judged and the reference's own.

Notation: gamma(k) = k u / (1 - k u) bounds the relative error of k roundings (Higham, Lemma 3.1).  A sum of n terms
taken in ANY order -- a tree over slabs, partial sums per workgroup, atomics, a merge of rank buffers -- has at most
n - 1 roundings on each term's path, so the envelopes do not depend on the kernel's summation order.  |X| is the
entrywise absolute value, products of |.| are matrix products of absolute values.

Constants (one line each):
  * K1 sums U_j = c sum A^T A, V_i = c sum B^T B, g = c_g sum J^T e over n observations: each observation's term is
    two products and one add (gamma(2)), the n terms summed (gamma(n - 1)), then scaled by c (one rounding):
    gamma(n + 2) * (the same sum over absolute values).
  * W_a = c A_a^T B_a: two products, one add, one scaling: gamma(3) |c| |A_a|^T |B_a|.
  * V* = V + mu I as the kernels form it: one rounding of each diagonal entry: u |V*_rr| (the same for U*).
  * V*^-1 by sym3_inverse (camera_model.h: adjugate over T = -det, iT = -1 / T, entry = cofactor * iT): T is five
    triple products and four adds (at most six roundings on a path: gamma(6) T_abs), a cofactor is two products and
    one add (gamma(2) C_abs), then the reciprocal and the product (two roundings): to first order the error is
    (gamma(2) C_abs + 2u |C| + |C| gamma(6) T_abs / |T|) / |T| <= gamma(8) (C_abs + |V*^-1| T_abs) / |T|, divided by
    1 - gamma(8) T_abs / |T| for the perturbed divisor.
  * An envelope dV of the input V* propagates as |V*^-1| dV |V*^-1| / (1 - eta), eta the largest row sum of
    |V*^-1| dV (Neumann series of (V* + D)^-1).
  * Y_a = W_a V*^-1: three products and two adds per entry: gamma(3) |W_a| |V*^-1| plus |W_a| env(V*^-1).
  * S_jk = delta_jk U*_j - sum_(a,b) Y_a W_b^T over the p_jk observation pairs (a of camera j, b of camera k, one
    point): 3 p_jk products summed (gamma(3 p_jk)), the subtraction from U* (1), U*'s own diagonal rounding (1) and
    Y's formation (counted in F below through gamma(3) |V*^-1|), r partial sums merged (r): the bound is
    gamma(3 p_jk + 4 + r) E + F, E = delta_jk |U*_j| + sum |Y_a| |W_b|^T,
    F = sum (|W_a| (env(V*^-1) + gamma(3) |V*^-1|)) |W_b|^T plus the propagated envelopes of U*, W when given.
  * e_a,j = g_a,j - sum_a Y_a g_b,i(a) over the n_j observations of camera j: gamma(3 n_j + 4 + r) (|g_a| +
    sum |Y_a| |g_b|) + sum |W_a| (env(V*^-1) + gamma(3) |V*^-1|) |g_b| plus the propagated envelopes of g, W.
  * e_b,i = g_b,i - sum_a W_a^T dpa_j(a): 6 products per observation, n_i observations, the subtraction:
    gamma(6 n_i + 2) (|g_b| + sum |W_a|^T |dpa|) when K3 reads W.  The default K3 recomputes A, B and forms
    c B^T (A dpa) (kernels_backsub.hip): gamma(6 n_i + 4) (|g_b| + |c| sum |B_a|^T |A_a| |dpa|).
  * dp_b,i = V*_i^-1 e_b,i with K3's own sym3_inverse: three products, two adds: (gamma(3) |V*^-1| + env(V*^-1))
    |e_b| plus |V*^-1| env(e_b).
  * the try scalars are sums over all terms of the step, r the partial sums merged (ranks): dp_l2 = sum dp^2:
    gamma(nT + 1 + r) sum dp^2; gain_den: k_backsub adds mu d d and d g_a as two terms per camera entry and
    d (mu d + g_b) as one per point entry, 2 nA + nB terms with at most three roundings before the sum:
    gamma(2 nA + nB + 3 + r) sum |dp| (|mu dp| + |g|) + sum |dp| env(g); newp_l2: gamma(nT + 1 + r) sum newp^2;
    new_cost = sum rho(s), s = |e|^2 (two products, one add), rho = s, or the robust loss of camera_model.h
    (robust_eval: at most six roundings, sqrt correctly rounded and log1p within two ulps, each relative to the
    terms of rho: 2 c sqrt(s) + c^2 for Huber's outer branch, rho itself for the others): per observation
    gamma(2) s + gamma(8) rho_abs, the sum gamma(nO + 1 + r) sum rho, and the residual slack below through
    |rho'(s)| <= 1: 2 |e| slack + slack^2.
Slacks where a kernel recomputes instead of reading (stated assumptions; the constants are not fitted to results):
  * RESIDUAL_SLACK: K1 sums the residual of linearize_obs (kernels_linearize.hip), the readable one is that of
    residual_obs (k_residual, psba_compute_exQT).  Their projection text is the same, but each kernel is compiled
    on its own, so every a b + c of the shared text may or may not become an FMA, and linearize_obs rounds x before
    m - x where residual_obs may fuse it.  So the two differ by up to twice the forward error of one fp64 evaluation
    of the projection: at most 64 roundings on a path (composition, rotation matrix, P = R M + t, the divide, the
    intrinsics, distortion up to r^6), each relative to a magnitude at most 4 (|m| + |proj|), hence
    2 * 64 * 4 u (|m| + |proj|) = 2^-44 (|m| + |proj|) per unwhitened component.  Whitening maps it through |L|,
    and the robust scaling w e has a derivative at most 1 in e, so the whitened, weighted slack is the 2-norm of
    |L| (slack_0, slack_1).  It enters g (|c_g| sum |J|^T slack) and new_cost.  Under a robust loss the weight of
    recomputed blocks moves with the recomputed residual: |dw| / w <= |dr| / c (robust_jac_slack), added to the
    relative JACOBIAN_SLACK of A and B.
  * JACOBIAN_SLACK: A and B are recomputed by other kernels than the dumping one: the default K3, the camera-major
    K1 pass (k_cam_sums: from 228 cameras on, or PSBA_LIN_GLOBAL_ACC), and the fused K1 itself (the non-dump
    instantiation).  With the same argument (the Jacobian's forward error, twice), we allow 2^-40 |A|, 2^-40 |B|
    per entry.  It enters e_b as |c| (s_B^T |A| + |B|^T s_A) |dpa|, U and V as (2 s + s^2) |c| sum |A|^T |A|
    (|B|^T |B|), W as (2 s + s^2) |c| |A|^T |B|, and g as s |c_g| sum |J|^T (|e| + e slack).
"""
import numpy as np

import dense_ref as dr

LD = dr.LD
LD_OK = dr.LD_OK
U = 2.0 ** -53 + 2.0 ** -63
RESIDUAL_SLACK = 2.0 ** -44
JACOBIAN_SLACK = 2.0 ** -40
PAIR_CHUNK = 1 << 16  # observation pairs per chunk of the S products


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def ld(x):
    return np.asarray(x).astype(LD)


def _segsum(x, key, n):
    """sum of the rows of x per key in [0, n) (any dtype); returns (sums, counts)."""
    key = np.asarray(key, dtype=np.int64)
    cnt = np.bincount(key, minlength=n)
    out = np.zeros((n,) + x.shape[1:], dtype=x.dtype)
    if key.size:
        order = np.argsort(key, kind="stable")
        starts = np.searchsorted(key[order], np.arange(n))
        nz = cnt > 0
        out[nz] = np.add.reduceat(x[order], starts[nz], axis=0)
    return out, cnt


def excess(got, exact, bound):
    """Largest |got - exact| / bound over all entries (inf where the bound is 0 and got differs), and the flat index."""
    err = np.abs(np.asarray(got).astype(LD) - exact).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    if ratio.size == 0:
        return 0.0, -1
    k = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[k]), k


# ---- K1 ---------------------------------------------------------------------------------------------------------

def residual_slack(impts, proj, L=None):
    """RESIDUAL_SLACK per observation [nO, 2]: 2^-44 (|m| + |proj|) per component, through |L| (whitening, L [nO,2,2])
    and, when L is given, as the 2-norm of the whitened pair in both components (the robust scaling)."""
    m = np.abs(np.asarray(impts, dtype=np.float64).reshape(-1, 2))
    s = RESIDUAL_SLACK * (m + np.abs(np.asarray(proj, dtype=np.float64).reshape(-1, 2)))
    if L is None:
        return s
    sw = np.einsum("nab,nb->na", np.abs(np.asarray(L, dtype=np.float64)), s)
    return np.repeat(np.sqrt((sw * sw).sum(axis=1))[:, None], 2, axis=1)


def robust_jac_slack(e_slack, c):
    """JACOBIAN_SLACK per observation under a robust loss: the recomputed blocks carry the weight w = sqrt(rho'(s)) of
    the recomputed residual, and |dw / w| <= |d r| / c for Huber, Cauchy and soft-L1 (r = |e|, c the scale), so a
    residual that differs by e_slack (its 2-norm) moves A, B by e_slack / c relative on top of JACOBIAN_SLACK."""
    es = np.asarray(e_slack, dtype=np.float64).reshape(-1, 2)
    return JACOBIAN_SLACK + np.sqrt((es * es).sum(axis=1)) / c


def k1_sums(JA, JB, ex, iidx, jidx, nC, nP, coeff=1.0, coeff_g=1.0, e_slack=None, recomputed=(), jac_slack=None):
    """U [nC,6,6], V [nP,3,3], W [nO,6,3], g [nT] (g_a then g_b) from the per-observation blocks A [2x6], B [2x3], e [2].
    e_slack [nO, 2]: e is not the residual the kernel summed (residual_slack).  recomputed: the names among "U",
    "ga", "V", "W", "gb" the kernel formed from blocks it recomputed (jac_slack per observation, default
    JACOBIAN_SLACK; see robust_jac_slack).  Returns {name: (exact, env)}."""
    A = np.asarray(JA, dtype=np.float64).reshape(-1, 2, 6)
    B = np.asarray(JB, dtype=np.float64).reshape(-1, 2, 3)
    e = np.asarray(ex, dtype=np.float64).reshape(-1, 2)
    iidx, jidx = np.asarray(iidx), np.asarray(jidx)
    AL, BL, eL = ld(A), ld(B), ld(e)
    aA, aB, ae = np.abs(A), np.abs(B), np.abs(e)
    c, cg = LD(coeff), LD(coeff_g)
    out = {}
    Ux, nU = _segsum(np.einsum("aki,akj->aij", AL, AL), jidx, nC)
    Ua, _ = _segsum(np.einsum("aki,akj->aij", aA, aA), jidx, nC)
    out["U"] = (c * Ux, gamma(nU + 2)[:, None, None] * abs(coeff) * Ua)
    Vx, nV = _segsum(np.einsum("aki,akj->aij", BL, BL), iidx, nP)
    Va, _ = _segsum(np.einsum("aki,akj->aij", aB, aB), iidx, nP)
    out["V"] = (c * Vx, gamma(nV + 2)[:, None, None] * abs(coeff) * Va)
    out["W"] = (c * np.einsum("aki,akj->aij", AL, BL), gamma(3) * abs(coeff) * np.einsum("aki,akj->aij", aA, aB))
    gax, _ = _segsum(np.einsum("aki,ak->ai", AL, eL), jidx, nC)
    gaa, _ = _segsum(np.einsum("aki,ak->ai", aA, ae), jidx, nC)
    gbx, _ = _segsum(np.einsum("aki,ak->ai", BL, eL), iidx, nP)
    gba, _ = _segsum(np.einsum("aki,ak->ai", aB, ae), iidx, nP)
    genv_a = gamma(nU + 2)[:, None] * abs(coeff_g) * gaa
    genv_b = gamma(nV + 2)[:, None] * abs(coeff_g) * gba
    es = np.zeros(ae.shape)
    if e_slack is not None:
        es = np.asarray(e_slack, dtype=np.float64).reshape(-1, 2)
        genv_a = genv_a + abs(coeff_g) * _segsum(np.einsum("aki,ak->ai", aA, es), jidx, nC)[0]
        genv_b = genv_b + abs(coeff_g) * _segsum(np.einsum("aki,ak->ai", aB, es), iidx, nP)[0]
    s = np.broadcast_to(JACOBIAN_SLACK if jac_slack is None else np.asarray(jac_slack, dtype=np.float64), (A.shape[0],))
    s2 = (2 * s + s * s)[:, None, None]
    if "U" in recomputed:
        out["U"] = (out["U"][0], out["U"][1] + abs(coeff) * _segsum(s2 * np.einsum("aki,akj->aij", aA, aA), jidx, nC)[0])
    if "V" in recomputed:
        out["V"] = (out["V"][0], out["V"][1] + abs(coeff) * _segsum(s2 * np.einsum("aki,akj->aij", aB, aB), iidx, nP)[0])
    if "W" in recomputed:
        out["W"] = (out["W"][0], out["W"][1] + abs(coeff) * s2 * np.einsum("aki,akj->aij", aA, aB))
    if "ga" in recomputed:
        genv_a = genv_a + abs(coeff_g) * _segsum(s[:, None] * np.einsum("aki,ak->ai", aA, ae + es), jidx, nC)[0]
    if "gb" in recomputed:
        genv_b = genv_b + abs(coeff_g) * _segsum(s[:, None] * np.einsum("aki,ak->ai", aB, ae + es), iidx, nP)[0]
    out["g"] = (cg * np.concatenate([gax.reshape(-1), gbx.reshape(-1)]),
                np.concatenate([genv_a.reshape(-1), genv_b.reshape(-1)]))
    return out


def damped(M, env, mu):
    """M + mu I per block (exact) and the envelope with the kernels' rounding of the diagonal."""
    M = ld(M).copy()
    env = np.array(env, dtype=np.float64)
    n = M.shape[-1]
    d = np.arange(n)
    M[:, d, d] += LD(mu)
    env[:, d, d] += U * np.abs(M[:, d, d].astype(np.float64))
    return M, env


# ---- K2 ---------------------------------------------------------------------------------------------------------

def vinv(Vs, env=None):
    """V*^-1 per point [nP,3,3] (exact, env).  Vs may be double (the GPU's V*) or extended (an exact V*)."""
    V = ld(Vs).reshape(-1, 3, 3)
    a11, a12, a13 = V[:, 0, 0], V[:, 0, 1], V[:, 0, 2]
    a22, a23, a33 = V[:, 1, 1], V[:, 1, 2], V[:, 2, 2]
    T = a33 * a12 * a12 - 2 * a12 * a13 * a23 + a22 * a13 * a13 + a11 * a23 * a23 - a11 * a22 * a33
    C = np.empty_like(V)
    C[:, 0, 0] = a22 * a33 - a23 * a23
    C[:, 0, 1] = a13 * a23 - a12 * a33
    C[:, 0, 2] = a12 * a23 - a13 * a22
    C[:, 1, 1] = a11 * a33 - a13 * a13
    C[:, 1, 2] = a12 * a13 - a11 * a23
    C[:, 2, 2] = a11 * a22 - a12 * a12
    C[:, 1, 0], C[:, 2, 0], C[:, 2, 1] = C[:, 0, 1], C[:, 0, 2], C[:, 1, 2]
    X = -C / T[:, None, None]
    b = np.abs(V.astype(np.float64))
    b11, b12, b13, b22, b23, b33 = b[:, 0, 0], b[:, 0, 1], b[:, 0, 2], b[:, 1, 1], b[:, 1, 2], b[:, 2, 2]
    Tabs = b33 * b12 * b12 + 2 * b12 * b13 * b23 + b22 * b13 * b13 + b11 * b23 * b23 + b11 * b22 * b33
    Cabs = np.empty(b.shape)
    Cabs[:, 0, 0] = b22 * b33 + b23 * b23
    Cabs[:, 0, 1] = b13 * b23 + b12 * b33
    Cabs[:, 0, 2] = b12 * b23 + b13 * b22
    Cabs[:, 1, 1] = b11 * b33 + b13 * b13
    Cabs[:, 1, 2] = b12 * b13 + b11 * b23
    Cabs[:, 2, 2] = b11 * b22 + b12 * b12
    Cabs[:, 1, 0], Cabs[:, 2, 0], Cabs[:, 2, 1] = Cabs[:, 0, 1], Cabs[:, 0, 2], Cabs[:, 1, 2]
    aT = np.abs(T.astype(np.float64))
    aX = np.abs(X.astype(np.float64))
    rel = gamma(8) * Tabs / aT
    envX = gamma(8) * (Cabs + aX * Tabs[:, None, None]) / aT[:, None, None] / (1.0 - rel)[:, None, None]
    if env is not None:
        M = aX @ np.asarray(env, dtype=np.float64).reshape(-1, 3, 3)
        eta = M.sum(axis=2).max(axis=1)
        envX = envX + (M @ aX) / (1.0 - eta)[:, None, None]
    return X, envX


def yblks(W, X, envX, iidx):
    """Y_a = W_a V*^-1 (exact with the exact V*^-1 X) and env from the GPU's formation and env(V*^-1)."""
    iidx = np.asarray(iidx)
    Wd = np.asarray(W, dtype=np.float64).reshape(-1, 6, 3)
    aW = np.abs(Wd)
    aX = np.abs(X.astype(np.float64))
    Yx = ld(Wd) @ X[iidx]
    env = aW @ (gamma(3) * aX + envX)[iidx]
    return Yx, env


def _pairs(iidx, nP):
    """All observation pairs (a, b) of one point, a-major: index arrays of length sum n_i^2."""
    iidx = np.asarray(iidx, dtype=np.int64)
    cnt = np.bincount(iidx, minlength=nP)
    ptr = np.concatenate([[0], np.cumsum(cnt)])
    n_of = cnt[iidx]
    a = np.repeat(np.arange(iidx.size), n_of)
    start = np.repeat(np.cumsum(n_of) - n_of, n_of)
    b = ptr[iidx[a]] + (np.arange(a.size) - start)
    return a, b


def schur(Us, W, Vs, g, iidx, jidx, nC, nP, r=1, envU=None, envW=None, envV=None, envg=None):
    """S (as blocks), e_a and V*^-1 from U* [nC,6,6], W [nO,6,3], V* [nP,3,3], g [nT] (doubles or exact values) with
    optional input envelopes.  Returns dict: jk [nb,2] (the blocks S has: the diagonal and every camera pair that shares
    a point), S [nb,6,6] exact, S_env, ea [6 nC] exact, ea_env, Vinv, Vinv_env, Y, Y_env."""
    iidx, jidx = np.asarray(iidx, dtype=np.int64), np.asarray(jidx, dtype=np.int64)
    nA = 6 * nC
    Wx = ld(W).reshape(-1, 6, 3)
    aW = np.abs(Wx.astype(np.float64))
    eW = None if envW is None else np.asarray(envW, dtype=np.float64).reshape(-1, 6, 3)
    X, envX = vinv(Vs, envV)
    aX = np.abs(X.astype(np.float64))
    M = gamma(3) * aX + envX
    Yx = Wx @ X[iidx]
    aY = np.abs(Yx.astype(np.float64))
    # |W_a| M_i (+ env(W_a) |V*^-1|): the F operand of every product; |W_a| |V*^-1| multiplies env(W_b)
    WM = aW @ M[iidx]
    if eW is not None:
        WM = WM + eW @ aX[iidx]
        WX = aW @ aX[iidx]
    a, b = _pairs(iidx, nP)
    key = jidx[a] * nC + jidx[b]
    keys = np.unique(np.concatenate([key, np.arange(nC) * (nC + 1)]))
    nb = keys.size
    Sx = np.zeros((nb, 6, 6), dtype=LD)
    E = np.zeros((nb, 6, 6))
    F = np.zeros((nb, 6, 6))
    p = np.zeros(nb)
    for c0 in range(0, a.size, PAIR_CHUNK):
        aa, bb = a[c0:c0 + PAIR_CHUNK], b[c0:c0 + PAIR_CHUNK]
        slot = np.searchsorted(keys, key[c0:c0 + PAIR_CHUNK])
        Wb_t = Wx[bb].transpose(0, 2, 1)
        aWb_t = aW[bb].transpose(0, 2, 1)
        np.add.at(p, slot, 1.0)
        s, _ = _segsum(Yx[aa] @ Wb_t, slot, nb)
        Sx += s
        s, _ = _segsum(aY[aa] @ aWb_t, slot, nb)
        E += s
        f = WM[aa] @ aWb_t
        if eW is not None:
            f = f + WX[aa] @ eW[bb].transpose(0, 2, 1)
        s, _ = _segsum(f, slot, nb)
        F += s
    dslot = np.searchsorted(keys, np.arange(nC) * (nC + 1))
    Sx = -Sx
    Usx = ld(Us).reshape(-1, 6, 6)
    Sx[dslot] += Usx
    E[dslot] += np.abs(Usx.astype(np.float64))
    if envU is not None:
        F[dslot] += np.asarray(envU, dtype=np.float64).reshape(-1, 6, 6)
    S_env = gamma(3 * p + 4 + r)[:, None, None] * E + F
    # e_a = g_a - sum Y_a g_b over each camera's observations
    gx = ld(g)
    gb = gx[nA:].reshape(-1, 3)
    agb = np.abs(gb.astype(np.float64))
    t, n_j = _segsum(np.einsum("art,at->ar", Yx, gb[iidx]), jidx, nC)
    ea = gx[:nA] - t.reshape(-1)
    Ee, _ = _segsum(np.einsum("art,at->ar", aY, agb[iidx]), jidx, nC)
    Fe, _ = _segsum(np.einsum("art,at->ar", WM, agb[iidx]), jidx, nC)
    if envg is not None:
        eg = np.asarray(envg, dtype=np.float64)
        Fe = Fe + _segsum(np.einsum("art,at->ar", WX if eW is not None else aW @ aX[iidx],
                                    eg[nA:].reshape(-1, 3)[iidx]), jidx, nC)[0]
        Fe = Fe + eg[:nA].reshape(-1, 6)
    ea_env = (gamma(3 * n_j + 4 + r)[:, None] * (np.abs(gx[:nA].astype(np.float64)).reshape(-1, 6) + Ee) + Fe)
    return dict(jk=np.stack([keys // nC, keys % nC], axis=1), S=Sx, S_env=S_env, ea=ea, ea_env=ea_env.reshape(-1),
                Vinv=X, Vinv_env=envX, Y=Yx, Y_env=aW @ M[iidx] if eW is None else WM, npairs=p)


def dense_to_blocks(S, jk, lower=False):
    """The blocks jk [nb,2] of a dense nA x nA S; lower: only the blocks on or below the diagonal (j >= k) and the lower
    triangle of the diagonal blocks are returned meaningful -- returns (blocks, mask of the judged entries)."""
    S = np.asarray(S)
    j, k = jk[:, 0], jk[:, 1]
    r = 6 * j[:, None] + np.arange(6)[None, :]
    c = 6 * k[:, None] + np.arange(6)[None, :]
    blk = S[r[:, :, None], c[:, None, :]]
    mask = np.ones(blk.shape, dtype=bool)
    if lower:
        mask &= (j >= k)[:, None, None]
        mask[j == k] &= np.tril(np.ones((6, 6), dtype=bool))
    return blk, mask


def outside_blocks(S, jk, nC, lower=False):
    """Entries of a dense S outside the blocks jk (on the judged triangle): they must be exact zeros."""
    present = np.zeros((nC, nC), dtype=bool)
    present[jk[:, 0], jk[:, 1]] = True
    if lower:
        present |= np.triu(np.ones((nC, nC), dtype=bool), 1)
    m = np.kron(~present, np.ones((6, 6), dtype=bool))
    return np.asarray(S)[m]


# ---- K3 ---------------------------------------------------------------------------------------------------------

def eb_ref(g, dpa, iidx, jidx, nC, nP, W=None, JA=None, JB=None, coeff=1.0, envW=None, envg=None, jac_slack=None):
    """e_b,i = g_b,i - sum_a W_a^T dpa_j(a).  W given: K3 reads W (and W may be exact with an envelope);
    otherwise K3 recomputes c B^T (A dpa) from the Jacobian blocks JA, JB (JACOBIAN_SLACK included)."""
    iidx, jidx = np.asarray(iidx, dtype=np.int64), np.asarray(jidx, dtype=np.int64)
    nA = 6 * nC
    gx = ld(g)
    d = np.asarray(dpa, dtype=np.float64).reshape(-1, 6)
    dL, ad = ld(d)[jidx], np.abs(d)[jidx]
    if W is not None:
        Wx = ld(W).reshape(-1, 6, 3)
        t, n_i = _segsum(np.einsum("akc,ak->ac", Wx, dL), iidx, nP)
        ab, _ = _segsum(np.einsum("akc,ak->ac", np.abs(Wx.astype(np.float64)), ad), iidx, nP)
        k = 6 * n_i + 2
        extra = 0.0
    else:
        A = np.asarray(JA, dtype=np.float64).reshape(-1, 2, 6)
        B = np.asarray(JB, dtype=np.float64).reshape(-1, 2, 3)
        Wx = LD(coeff) * np.einsum("aki,akj->aij", ld(A), ld(B))
        t, n_i = _segsum(np.einsum("akc,ak->ac", Wx, dL), iidx, nP)
        sA = np.einsum("aki,ai->ak", np.abs(A), ad)  # |A| |dpa|
        ab, _ = _segsum(abs(coeff) * np.einsum("akc,ak->ac", np.abs(B), sA), iidx, nP)
        k = 6 * n_i + 4
        js = np.broadcast_to(JACOBIAN_SLACK if jac_slack is None else np.asarray(jac_slack, dtype=np.float64),
                             (A.shape[0],))
        extra, _ = _segsum(abs(coeff) * (2 * js + js * js)[:, None] * np.einsum("akc,ak->ac", np.abs(B), sA), iidx, nP)
    eb = gx[nA:].reshape(-1, 3) - t
    env = gamma(k)[:, None] * (np.abs(gx[nA:].astype(np.float64)).reshape(-1, 3) + ab) + extra
    if envW is not None:
        env = env + _segsum(np.einsum("akc,ak->ac", np.asarray(envW, dtype=np.float64).reshape(-1, 6, 3), ad),
                            iidx, nP)[0]
    if envg is not None:
        env = env + np.asarray(envg, dtype=np.float64)[nA:].reshape(-1, 3)
    return eb.reshape(-1), env.reshape(-1)


def dpb_ref(X, envX, eb, env_eb=None):
    """dp_b,i = V*_i^-1 e_b,i from the exact V*^-1 (X, envX) and e_b (double or exact) with an optional envelope."""
    e = ld(eb).reshape(-1, 3)
    ae = np.abs(e.astype(np.float64))
    aX = np.abs(X.astype(np.float64))
    dp = np.einsum("irc,ic->ir", X, e)
    env = np.einsum("irc,ic->ir", gamma(3) * aX + envX, ae)
    if env_eb is not None:
        env = env + np.einsum("irc,ic->ir", aX, np.asarray(env_eb, dtype=np.float64).reshape(-1, 3))
    return dp.reshape(-1), env.reshape(-1)


def rho_ext(s, kind=0, c=1.0):
    """rho(s) of camera_model.h's robust_eval in extended precision, and the magnitude its rounding is relative to."""
    sL = ld(s)
    sd = np.asarray(s, dtype=np.float64)
    cL, c2 = LD(c), LD(c) * LD(c)
    if kind == 1:  # Huber
        inside = sL <= c2
        r = np.where(inside, sL, 2 * cL * np.sqrt(sL) - c2)
        mag = np.where(inside, sd, 2 * c * np.sqrt(sd) + c * c)
    elif kind == 2:  # Cauchy
        r = c2 * np.log1p(sL / c2)
        mag = np.abs(r.astype(np.float64))
    elif kind == 3:  # soft-L1
        r = 2 * sL / (np.sqrt(1 + sL / c2) + 1)
        mag = np.abs(r.astype(np.float64))
    else:
        r, mag = sL, sd
    return r, mag


def try_scalars(dp, newp, mu, g, nA, s_new, e_slack=None, envg=None, loss=(0, 1.0), r=1, extra=0):
    """The four sums of one damping try: {name: (exact, bound)}.  dp, newp: the GPU's step and proposal; g (double or
    exact) with its envelope; s_new [nO] the squared whitened residuals at the proposal as k_residual forms them
    (e_slack [nO, 2]: K3 recomputes them); loss (kind, c); r the partial sets merged on the host.  mu: a scalar, or
    the weights mu D [nT] of a diagonal damping in extended precision (free_ref), formed by the kernel with `extra`
    roundings more per term of gain_den."""
    dpL = ld(dp)
    ad = np.abs(np.asarray(dp, dtype=np.float64))
    gx = ld(g)
    nT = ad.size
    out = {"dp_l2": (np.sum(dpL * dpL), float(gamma(nT + 1 + r) * np.sum(ad * ad)))}
    if np.ndim(mu) == 0:   # (the scalar rule: the expressions are what they always were)
        den_env = float(gamma(2 * nA + (nT - nA) + 3 + r) * np.sum(ad * (abs(mu) * ad + np.abs(gx.astype(np.float64)))))
        mu = LD(mu)
    else:
        mu = ld(mu)
        den_env = float(gamma(2 * nA + (nT - nA) + 3 + extra + r)
                        * np.sum(ad * (np.abs(mu.astype(np.float64)) * ad + np.abs(gx.astype(np.float64)))))
    if envg is not None:
        den_env += float(np.sum(ad * np.asarray(envg, dtype=np.float64)))
    out["gain_den"] = (np.sum(dpL * (mu * dpL + gx)), den_env)
    npL = ld(newp)
    out["newp_l2"] = (np.sum(npL * npL), float(gamma(nT + 1 + r) * np.sum(np.abs(np.asarray(newp, dtype=np.float64)) ** 2)))
    sd = np.asarray(s_new, dtype=np.float64).reshape(-1)
    rx, mag = rho_ext(sd, *loss)
    per = gamma(2) * sd + gamma(8) * mag
    if e_slack is not None:
        es = np.asarray(e_slack, dtype=np.float64).reshape(-1, 2).max(axis=1)
        ae = np.sqrt(sd)
        per = per + 2 * np.sqrt(2) * ae * es + 2 * es * es
    cost_env = float(gamma(sd.size + 1 + r) * np.sum(np.abs(rx.astype(np.float64))) + np.sum(per))
    out["new_cost"] = (np.sum(rx), cost_env)
    return out
