"""Fixed parameter blocks (psba_set_fixed) on top of tests/assembly_ref.py (host only, not a test file).

The mirror verbs dump the masked blocks (A = 0 for a fixed camera, B = 0 for a fixed point), so assembly_ref's
k1_sums, schur, eb_ref, dpb_ref and try_scalars apply to them unchanged: every sum over a fixed block is an exact zero
with a zero envelope.  What the sums do not know is the placeholder the library stores in the diagonal block of a fixed
camera or point.  `install` and `damped` state that rule once, as exact values with a zero envelope:
  * U_j = place I for a fixed camera on the rank that owns the camera terms, 0 on the others (k_fixed_diag's cam_diag);
  * V_i = place I for a fixed point;
  * g = 0 on fixed blocks;
  * U* and V* on those blocks are the once-rounded fp64 sum place + mu.
`place` is the coefficient of psba_linearize on the GPU (1, or 2 under the trust-region coefficients) and 0 for the
oracle's sums, which have no placeholder.  `free_max` is the maximum over the diagonals of free blocks only.
No constant is added here: every bound is one of assembly_ref's envelopes or exactly zero.

The masks of the tests (mixed, island, long) are computed here from the problem, with the upload's greedy tiling
restated (psba_api.cpp cut_tiles; TILE_OBS, TILE_PTS from psba_internal.h)."""
import numpy as np

import assembly_ref as ar

TILE_OBS = 256  # observations per point-aligned tile (psba_internal.h)
TILE_PTS = 128  # points per tile
WAVE = 64


def flags(fc, fp):
    return np.asarray(fc) != 0, np.asarray(fp) != 0


def fixed_entries(fc, fp):
    """boolean [6 nC + 3 nP]: the entries of the parameter vector that belong to fixed blocks"""
    fc, fp = flags(fc, fp)
    return np.r_[np.repeat(fc, 6), np.repeat(fp, 3)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same_bits(got, want):
    """equal as bit patterns: -0.0 is not +0.0 (np.array_equal says it is)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def plus_zero(x):
    """every entry is +0.0"""
    return not np.any(bits(x))


def install(k1, fc, fp, place, owner=True):
    """The placeholder rule on the output of ar.k1_sums: {name: (exact, env)} with U_j = place I (0 where this rank
    does not own the camera terms), V_i = place I and g = 0 on fixed blocks, all with a zero envelope."""
    fc, fp = flags(fc, fp)
    out = dict(k1)
    Ux, Ue = k1["U"][0].copy(), np.array(k1["U"][1], dtype=np.float64)
    Vx, Ve = k1["V"][0].copy(), np.array(k1["V"][1], dtype=np.float64)
    gx, ge = k1["g"][0].copy(), np.array(k1["g"][1], dtype=np.float64)
    Ux[fc] = ar.LD(place if owner else 0.0) * np.eye(6, dtype=ar.LD)
    Ue[fc] = 0.0
    Vx[fp] = ar.LD(place) * np.eye(3, dtype=ar.LD)
    Ve[fp] = 0.0
    fx = fixed_entries(fc, fp)
    gx[fx] = 0.0
    ge[fx] = 0.0
    out["U"], out["V"], out["g"] = (Ux, Ue), (Vx, Ve), (gx, ge)
    return out


def damped(M, env, mu, fixed, place):
    """ar.damped with the fixed blocks (place + mu) I exactly: the once-rounded fp64 sum, zero envelope."""
    fixed = np.asarray(fixed) != 0
    X, e = ar.damped(M, env, mu)
    n = X.shape[-1]
    X[fixed] = ar.LD(np.float64(place) + np.float64(mu)) * np.eye(n, dtype=ar.LD)
    e[fixed] = 0.0
    return X, e


def free_max(U, V, fc, fp):
    """The largest diagonal entry of U [nC,6,6] and V [nP,3,3] over the free blocks."""
    fc, fp = flags(fc, fp)
    U = np.asarray(U, dtype=np.float64).reshape(-1, 6, 6)
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3, 3)
    return max(float(np.diagonal(U[~fc], axis1=1, axis2=2).max(initial=0.0)),
               float(np.diagonal(V[~fp], axis1=1, axis2=2).max(initial=0.0)))


def all_max(U, V):
    """The maximum a kernel that forgot the mask returns: placeholders included."""
    return free_max(U, V, np.zeros(np.asarray(U).size // 36, dtype=bool), np.zeros(np.asarray(V).size // 9, dtype=bool))


# ---- the masks ----------------------------------------------------------------------------------------------------

def point_ptr(iidx, nP):
    iidx = np.asarray(iidx, dtype=np.int64)
    assert np.all(np.diff(iidx) >= 0), "observations are sorted by point"
    return np.concatenate([[0], np.cumsum(np.bincount(iidx, minlength=nP))])


def tiles(iidx, nP):
    """[(p0, p1)]: whole points, at most TILE_OBS observations and TILE_PTS points per tile; a point with more than
    TILE_OBS observations is a tile of its own (cut_tiles in psba_api.cpp)."""
    ptr = point_ptr(iidx, nP)
    out, p0 = [], 0
    while p0 < nP:
        p1 = p0
        if ptr[p0 + 1] - ptr[p0] > TILE_OBS:
            p1 = p0 + 1
        else:
            while p1 < nP and ptr[p1 + 1] - ptr[p0] <= TILE_OBS and p1 - p0 < TILE_PTS:
                p1 += 1
        out.append((p0, p1))
        p0 = p1
    return out


def crosses_wave(ptr, p0, p):
    """point p of the tile that starts at point p0 has observations on both sides of a multiple of 64 in the tile"""
    first, last = ptr[p] - ptr[p0], ptr[p + 1] - 1 - ptr[p0]
    return first // WAVE != last // WAVE


def mixed_mask(prob, cam_of_max, frac=0.1, seed=17):
    """Cameras 0, 1, nC - 1 and the one with the largest diagonal entry of U; points: the seeded 10 % of
    tests/test_gpu_fixed.py, point 0 and nP - 1, the first and the last point of every fourth tile, and one point whose
    observations cross a multiple of 64 inside its tile.  Returns (fc, fp, info)."""
    nC, nP = int(prob["nC"]), int(prob["nP"])
    fc = np.zeros(nC, dtype=np.uint8)
    fc[[0, 1, nC - 1, int(cam_of_max)]] = 1
    fp = np.zeros(nP, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    fp[rng.choice(nP, max(1, round(frac * nP)), replace=False)] = 1
    fp[[0, nP - 1]] = 1
    tl = tiles(prob["iidx"], nP)
    edge = sorted({p for p0, p1 in tl[::4] for p in (p0, p1 - 1)})
    fp[edge] = 1
    ptr = point_ptr(prob["iidx"], nP)
    cross = next(p for p0, p1 in tl if ptr[p1] - ptr[p0] <= TILE_OBS for p in range(p0, p1) if crosses_wave(ptr, p0, p))
    fp[cross] = 1
    t0 = next(p0 for p0, p1 in tl if p0 <= cross < p1)
    assert crosses_wave(ptr, t0, cross)
    assert not fc.all() and not fp.all()
    info = dict(cams=np.flatnonzero(fc).tolist(), n_pts=int(fp.sum()), tiles=len(tl), tile_edges=len(edge),
                wave_point=int(cross), wave_obs=(int(ptr[cross] - ptr[t0]), int(ptr[cross + 1] - 1 - ptr[t0])))
    return fc, fp, info


def island_mask(prob):
    """Cameras 0 and 1; every camera of the point with the fewest views (that point stays free and sees only fixed
    cameras: its W are zero, dp_b = V*^-1 g_b); every point of the camera with the fewest observations among those
    still free (that camera stays free and sees only fixed points: S_jj = U*_j, the rest of its row exactly zero)."""
    nC, nP = int(prob["nC"]), int(prob["nP"])
    iidx, jidx = np.asarray(prob["iidx"], dtype=np.int64), np.asarray(prob["jidx"], dtype=np.int64)
    fc = np.zeros(nC, dtype=np.uint8)
    fc[[0, 1]] = 1
    views = np.bincount(iidx, minlength=nP)
    pt = int(np.argmin(np.where(views > 0, views, views.max() + 1)))
    fc[jidx[iidx == pt]] = 1
    nobs = np.bincount(jidx, minlength=nC)
    cam = int(np.argmin(np.where((fc == 0) & (nobs > 0), nobs, nobs.max() + 1)))
    fp = np.zeros(nP, dtype=np.uint8)
    fp[iidx[jidx == cam]] = 1
    assert fc[cam] == 0 and fp[pt] == 0
    assert np.all(fc[jidx[iidx == pt]] == 1) and np.all(fp[iidx[jidx == cam]] == 1)
    assert not fc.all() and not fp.all()
    info = dict(cams=np.flatnonzero(fc).tolist(), n_pts=int(fp.sum()), island_point=pt, island_cam=cam)
    return fc, fp, info


def long_mask(prob):
    """Cameras 0 and 1; the first point with more than TILE_OBS views fixed; twenty cameras of the second such point."""
    nC, nP = int(prob["nC"]), int(prob["nP"])
    iidx, jidx = np.asarray(prob["iidx"], dtype=np.int64), np.asarray(prob["jidx"], dtype=np.int64)
    lng = np.flatnonzero(np.bincount(iidx, minlength=nP) > TILE_OBS)
    assert lng.size >= 2, "two long points"
    fc = np.zeros(nC, dtype=np.uint8)
    fc[[0, 1]] = 1
    cams = jidx[iidx == lng[1]]
    fc[cams[~np.isin(cams, [0, 1])][:20]] = 1
    fp = np.zeros(nP, dtype=np.uint8)
    fp[lng[0]] = 1
    assert int(fc[cams].sum()) >= 20 and not fc[cams].all()
    assert not fc.all() and not fp.all()
    info = dict(cams=np.flatnonzero(fc).tolist(), n_pts=1, fixed_long_point=int(lng[0]), other_long_point=int(lng[1]))
    return fc, fp, info


def scaled_problem(prob, k=-22):
    """The problem with K's fu, u0, v0 and every image point multiplied by 2^k: an exact scaling of A, B and e, which
    brings the largest free diagonal entry of U and V below the placeholder."""
    s = np.ldexp(1.0, k)
    K = np.array(prob["K"], dtype=np.float64).reshape(int(prob["nC"]), 5).copy()
    K[:, :3] *= s
    out = type(prob)(prob)
    out["K"] = K.reshape(np.asarray(prob["K"]).shape)
    out["impts"] = np.asarray(prob["impts"], dtype=np.float64) * s
    return out
