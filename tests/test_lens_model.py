"""Lens distortion and per-observation covariances on the host (no GPU): the numpy twin (tests/lens_twin.py) against
central differences and the oracle, psba_read_problem_ex and psba_convert_bal_kd."""
import os

import numpy as np
import pytest

import psba_amd
from lens_twin import Twin
from oracle_lib import Oracle
from sba_text import KK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")


def _prob7():
    return psba_amd.read_problem(os.path.join(DATA, "7cams.txt"), os.path.join(DATA, "7pts.txt"), KK)


def _random_spd(rng, n):
    G = rng.normal(size=(n, 2, 2))
    return G @ np.transpose(G, (0, 2, 1)) + 0.5 * np.eye(2)[None]


def _perturbed(prob, rng):
    """the 7-camera problem at a nearby point with nonzero local rotations (the rotation columns then matter)"""
    cams = np.array(prob["cams"], dtype=np.float64)
    cams[:, :3] += 0.01 * rng.normal(size=(prob["nC"], 3))
    return cams


def test_twin_jacobian_central_differences():
    rng = np.random.default_rng(1)
    prob = _prob7()
    kc = np.tile([0.3, -0.2, 0.004, -0.003, 0.05], (prob["nC"], 1)) * (1.0 + 0.1 * rng.normal(size=(prob["nC"], 5)))
    cov = _random_spd(rng, prob["nO"])
    t = Twin(prob, kc, cov)
    t.cams = _perturbed(prob, rng)
    e, A, B = t.linearize()
    # every sixth observation: the central differences of the whitened projection -L proj (e = L (m - proj))
    sel = np.arange(0, prob["nO"], 6)
    h = 1e-6
    for k in range(6):
        cp, cm = t.cams.copy(), t.cams.copy()
        cp[:, k] += h
        cm[:, k] -= h
        d = -(t.residual(cams=cp) - t.residual(cams=cm)) / (2 * h)
        ref = A[:, :, k]
        err = np.abs(d[sel] - ref[sel]).max() / np.abs(ref[sel]).max()
        assert err < 1e-6, f"camera column {k}: {err:.2e}"
    for k in range(3):
        pp, pm = t.pts.copy(), t.pts.copy()
        pp[:, k] += h
        pm[:, k] -= h
        d = -(t.residual(pts=pp) - t.residual(pts=pm)) / (2 * h)
        ref = B[:, :, k]
        err = np.abs(d[sel] - ref[sel]).max() / np.abs(ref[sel]).max()
        assert err < 1e-6, f"point column {k}: {err:.2e}"
    # and the distortion is not negligible here: the same geometry without it projects elsewhere
    assert np.abs(Twin(prob).project(cams=t.cams) - t.project()).max() > 1.0


def test_twin_pinned_to_oracle():
    prob = _prob7()
    rng = np.random.default_rng(2)
    cams = _perturbed(prob, rng)
    prob = psba_amd.Problem(prob, cams=cams)
    o = Oracle(prob)
    t = Twin(prob, np.zeros((prob["nC"], 5)), np.tile(np.eye(2), (prob["nO"], 1, 1)))
    e, A, B = t.linearize()
    ex = o.exQT()
    JA, JB = o.jacobiQT()
    assert np.abs(e.reshape(-1) - ex).max() <= 1e-12 * max(1.0, np.abs(ex).max())
    assert np.abs(A.reshape(-1) - JA).max() <= 1e-12 * np.abs(JA).max()
    assert np.abs(B.reshape(-1) - JB).max() <= 1e-12 * np.abs(JB).max()


def test_whitening_exact_for_scaled_identity():
    from lens_twin import whitening
    L = whitening(np.tile(4.0 * np.eye(2), (3, 1, 1)))
    assert (L == np.tile(0.5 * np.eye(2), (3, 1, 1))).all()


def test_read_problem_ex_54camsvarKD():
    cams, pts = os.path.join(DATA, "54camsvarKD.txt"), os.path.join(DATA, "54pts.txt")
    p = psba_amd.read_problem_ex(cams, pts)
    assert p["kc"] is not None and p["kc"].shape == (54, 5)
    assert (p["kc"] == 0.0).all()  # the reference's file carries zero distortion
    assert p["cov"] is None
    base = psba_amd.read_problem(cams, pts)
    for k in ("K", "initrot", "cams", "pts", "impts", "iidx", "jidx"):
        assert np.array_equal(p[k], base[k]), k
    # the 12-column file of the same cameras: the same base arrays, no kc
    q = psba_amd.read_problem_ex(os.path.join(DATA, "54camsvarK.txt"), pts)
    assert q["kc"] is None and q["cov"] is None
    for k in ("K", "initrot", "cams", "pts", "impts", "iidx", "jidx"):
        assert np.allclose(q[k], base[k], rtol=0, atol=1e-15), k


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)


@pytest.mark.parametrize("ncov", [0, 3, 4])
def test_read_problem_ex_written_files(tmp_path, ncov):
    rng = np.random.default_rng(3 + ncov)
    nC, nP = 4, 6
    K = np.array([800.0, 320.0, 240.0, 1.0, 0.0])
    kc = rng.normal(scale=0.05, size=(nC, 5))
    lines = ["# fu u0 v0 ar s kc(1:5) q t"]
    for j in range(nC):
        q = np.array([1.0, 0.01 * j, -0.02 * j, 0.005])
        q /= np.linalg.norm(q)
        lines.append(" ".join(f"{v:.17g}" for v in np.concatenate([K, kc[j], q, [0.1 * j, -0.2, 0.3]])))
    _write(tmp_path / "c.txt", "\n".join(lines) + "\n")
    # frames out of camera order; every frame's covariance tagged by (point, camera) so that the reorder shows
    expect = {}
    plines = []
    for i in range(nP):
        frames = rng.permutation(nC)[: 2 + i % 3]
        toks = [f"{rng.normal():.6f}", f"{rng.normal():.6f}", f"{5 + rng.normal():.6f}", str(len(frames))]
        for cam in frames:
            x, y = rng.normal(scale=100, size=2)
            a, b, c = 1.0 + i + 0.1 * cam, 0.01 * (i + 1) * (cam + 1), 2.0 + 0.5 * cam
            toks += [str(cam), f"{x:.6f}", f"{y:.6f}"]
            if ncov == 4:
                toks += [f"{a:.17g}", f"{b:.17g}", f"{b:.17g}", f"{c:.17g}"]
            elif ncov == 3:
                toks += [f"{a:.17g}", f"{b:.17g}", f"{c:.17g}"]
            expect[(i, int(cam))] = (x, y, np.array([[a, b], [b, c]]))
        plines.append(" ".join(toks))
    _write(tmp_path / "p.txt", "\n".join(plines) + "\n")
    p = psba_amd.read_problem_ex(str(tmp_path / "c.txt"), str(tmp_path / "p.txt"))
    base = psba_amd.read_problem(str(tmp_path / "c.txt"), str(tmp_path / "p.txt"))
    for k in ("K", "initrot", "cams", "pts", "impts", "iidx", "jidx"):
        assert np.array_equal(p[k], base[k]), k
    assert np.array_equal(p["kc"], np.array([[float(f"{v:.17g}") for v in row] for row in kc]))
    assert (np.diff(p["jidx"])[np.diff(p["iidx"]) == 0] > 0).all()  # cameras ascending inside a point
    if ncov == 0:
        assert p["cov"] is None
        return
    assert p["cov"].shape == (p["nO"], 2, 2)
    for a in range(p["nO"]):
        x, y, S = expect[(int(p["iidx"][a]), int(p["jidx"][a]))]
        assert np.allclose(p["impts"][a], [x, y], atol=1e-6)
        assert np.array_equal(p["cov"][a], S), a


def _bal_text(rng, nC=3, nP=12, k1=-0.3, k2=0.1):
    """A small BAL problem: cameras looking down -z at points in front, with radial distortion."""
    cams = []
    for j in range(nC):
        r = rng.normal(scale=0.05, size=3)
        t = np.array([0.2 * j, -0.1, -8.0])
        cams.append(np.concatenate([r, t, [600.0 + 10 * j, k1 * (1 + 0.1 * j), k2]]))
    pts = rng.uniform(-2.0, 2.0, size=(nP, 3))
    obs = []

    def rodrigues(r):
        th = np.linalg.norm(r)
        k = r / th
        X = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(th) * X + (1 - np.cos(th)) * X @ X

    for i in range(nP):
        for j in range(nC):
            c = cams[j]
            P = rodrigues(c[:3]) @ pts[i] + c[3:6]
            p = -P[:2] / P[2]
            n2 = p @ p
            x, y = c[6] * (1 + c[7] * n2 + c[8] * n2 * n2) * p
            obs.append((j, i, x, y))
    rng.shuffle(obs)
    out = [f"{nC} {nP} {len(obs)}"]
    out += [f"{j} {i} {x:.17g} {y:.17g}" for j, i, x, y in obs]
    out += [f"{v:.17g}" for c in cams for v in c]
    out += [f"{v:.17g}" for p in pts for v in p]
    return "\n".join(out) + "\n"


def test_convert_bal_kd(tmp_path):
    rng = np.random.default_rng(5)
    _write(tmp_path / "bal.txt", _bal_text(rng))
    c, p = str(tmp_path / "c.txt"), str(tmp_path / "p.txt")
    psba_amd.convert_bal_kd(str(tmp_path / "bal.txt"), c, p)
    prob = psba_amd.read_problem_ex(c, p)
    assert prob["kc"] is not None and prob["cov"] is None
    assert (prob["kc"][:, 2:] == 0.0).all()
    r = Twin(prob, prob["kc"]).residual()
    assert np.abs(r).max() < 1e-9, np.abs(r).max()
    # without the radial terms the same cameras miss by pixels
    assert np.abs(Twin(prob).residual()).max() > 1.0
    # the plain converter: the same base problem
    c2, p2 = str(tmp_path / "c2.txt"), str(tmp_path / "p2.txt")
    kmax = psba_amd.convert_bal(str(tmp_path / "bal.txt"), c2, p2)
    assert kmax > 0.2
    plain = psba_amd.read_problem(c2, p2)
    for k in ("K", "initrot", "cams", "pts", "impts", "iidx", "jidx"):
        assert np.array_equal(plain[k], prob[k]), k


def test_shard_problem_carries_cov():
    from psba_amd.capi import shard_problem
    rng = np.random.default_rng(6)
    prob = _prob7()
    prob["kc"] = rng.normal(size=(prob["nC"], 5))
    prob["cov"] = _random_spd(rng, prob["nO"])
    total = 0
    for r in range(3):
        s = shard_problem(prob, 3, r)
        assert s["kc"] is prob["kc"]
        assert s["cov"].shape == (s["nO"], 2, 2)
        assert np.array_equal(s["cov"], prob["cov"][total:total + s["nO"]])
        total += s["nO"]
    assert total == prob["nO"]
