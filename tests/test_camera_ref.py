"""The derived per-entry bound of tests/camera_ref.py against the exact values, without a GPU: the fp64 numpy evaluation
of the model's text stands in for a kernel.

  * bound validity: on every input family |fp64 - exact| <= bound for EVERY entry of e, A, B (lens_linearize and the
    blocks of 11 and 16) and of k_residual's e and s; no entry is left out and no divisor is refused (a refusal raises);
  * the families have the properties they are named for;
  * the text over mpmath agrees with the exact values, which come from another formulation (quaternion sandwich, dual
    numbers): a mistake in either shows here;
  * mutations of the text that a kernel could carry are flagged: a reciprocal 2^-48 off, 6 k4 x written as 2 k4 x;
  * a report (asserted nowhere) of how twice the derived bound compares per entry with RESIDUAL_SLACK and
    JACOBIAN_SLACK of tests/assembly_ref.py on the problems the entrywise suites use.
The module prints the worst error-to-bound ratio per family and quantity."""
import numpy as np
import pytest

import assembly_ref as ar
import camera_ref as cr

pytestmark = pytest.mark.skipif(not cr.LD_OK, reason="needs an 80-bit long double")

# (family, camera block, intrinsics mask): the fixed-intrinsics model on every family, the free blocks where the GPU
# module judges them
CASES = [(f, 6, cr.KD_ALL_FREE) for f in cr.FAMILIES] + [
    ("far", 11, cr.KD_ALL_FREE), ("rot", 11, cr.KD_ALL_FREE), ("dist", 16, cr.KD_ALL_FREE), ("dist", 16, cr.BAL_MASK),
    ("rot", 16, cr.KD_ALL_FREE)]
WORST = {}


def _id(c):
    return c[0] if c[1] == 6 else f"{c[0]}-{c[1]}" + ("" if c[2] == cr.KD_ALL_FREE else "-bal")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nworst |fp64 - exact| / bound per family and quantity (numpy stand-in):")
        for fam in dict.fromkeys(f for f, _ in WORST):
            print(f"  {fam}: " + ", ".join(f"{q} {v:.3f}" for (ff, q), v in WORST.items() if ff == fam))


def judge(fam, what, got, exact, bound, record=True):
    r, k = ar.excess(got, exact, bound)
    if record:
        WORST[(fam, what)] = max(WORST.get((fam, what), 0.0), r)
    assert r <= 1.0, (f"{fam} {what}: entry {k} = {np.asarray(got).reshape(-1)[k]!r}, exact "
                      f"{float(np.asarray(exact).reshape(-1)[k])!r}, bound {float(np.asarray(bound).reshape(-1)[k]):.3e} "
                      f"(ratio {r:.3e})")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bound_validity(case):
    fam, cnp, mask = case
    c = cr.family(fam)
    eE, AE, BE = cr.linearize(cr.gather(c, "E", cnp, mask))  # (a refused divisor raises here)
    ef, Af, Bf = cr.linearize(cr.gather(c, "f64", cnp, mask))
    ex, Ax, Bx, sx = cr.exact(cr.gather(c, "raw", cnp, mask))
    name = _id(case)
    for what, vE, vf, x in (("e", eE, ef, ex), ("A", AE, Af, Ax), ("B", BE, Bf, Bx)):
        v, b = cr.stack(vE)
        f, _ = cr.stack(vf)
        assert f.shape == x.shape == b.shape and np.all(np.isfinite(b))
        judge(name, what, f, x, b)
        judge(name, what + " (extended)", v, x, b, record=False)  # the bound covers the extended evaluation too
    if cnp == 6:
        (eE, sE), (ef, sf) = cr.residual(cr.gather(c, "E")), cr.residual(cr.gather(c, "f64"))
        judge(name, "e (k_residual)", cr.stack(ef)[0], ex, cr.stack(eE)[1])
        judge(name, "s", cr.stack([sf])[0], sx[:, None], cr.stack([sE])[1])
        if c["kc"] is None:  # A[9] is a structural zero: value 0, bound 0
            v, b = cr.stack(AE)
            assert not np.any(v[:, 9]) and not np.any(b[:, 9]) and not np.any(cr.stack(Af)[0][:, 9])


def test_family_properties():
    for fam in cr.FAMILIES:
        p = cr.family(fam)["prob"]
        assert p["nO"] == cr.NOBS == 333 and p["nO"] % 64 != 0 and np.bincount(p["jidx"])[0] == 65
        assert np.all(np.diff(p["iidx"]) >= 0)
    pose = {}
    for fam in ("benign", "far", "near", "rot", "dist"):
        x = cr.gather(cr.family(fam), "f64")
        pose[fam] = (x,) + cr._pose(x["q0"], x["cam"], x["M"])
    x, _, _, _, P, _ = pose["far"]
    M, t = np.stack(x["M"], 1), np.stack(x["cam"][3:], 1)
    ratio = np.linalg.norm(M, axis=1) / P[2]
    assert ratio.min() < 2e2 and ratio.max() > 5e3 and (np.linalg.norm(t, axis=1) / P[2]).max() > 5e3
    x, _, _, _, P, inv = pose["near"]
    assert 0.005 < P[2].min() and P[2].max() < 0.02 and 3e4 < (1000 * np.abs(P[0] * inv)).max() < 3e5
    v = cr.family("rot")["prob"]["cams"][:, :3]
    n = np.linalg.norm(v, axis=1)
    assert not np.any(v[0]) and v[1, 1] == 0.0 and v[1, 0] != 0.0
    for mag in (0.9, 0.999, 1 - 1e-6):
        assert np.any(np.abs(n - mag) < 1e-12)
    x, _, _, _, P, inv = pose["dist"]
    xn, yn = P[0] * inv, P[1] * inv
    r2 = xn * xn + yn * yn
    kc = x["kc"]
    radial = 1.0 + r2 * (kc[0] + r2 * (kc[1] + r2 * kc[4]))
    J = cr.distort(kc, xn, yn, True)[2]
    assert 1.6 < r2.max() < 2.6 and np.abs(radial).min() < 0.1 and np.abs(J[0]).min() < 0.05 and np.abs(J[3]).min() < 0.05
    assert not np.any(cr.family("dist")["kc"][8]) and np.all(np.any(cr.family("dist")["kc"][:8] != 0, axis=1))
    from lens_twin import whitening
    cov = cr.family("cov")["cov"]
    ev = np.linalg.eigvalsh(cov)
    assert np.all(ev[:, 1] / ev[:, 0] > 0.9e8) and np.all(np.abs(whitening(cov)[:, 0, 1]) > 1e-3)
    for fam in ("robust-huber", "robust-cauchy", "robust-softl1"):
        c = cr.family(fam)
        _, s = cr.residual(cr.gather(c, "E"))
        q = (s.v / cr.LD(cr.ROBUST_C) ** 2).astype(np.float64)
        assert q.min() < 1e-11 and q.max() > 1e11 and np.sum(np.abs(q - 1) < 3e-9) >= 30
        if fam == "robust-huber":  # both branches, and some observations inside their own bound of the boundary
            amb = np.abs(s.v - cr.LD(cr.ROBUST_C) ** 2) <= 2 * s.b
            assert amb.sum() >= 3 and np.sum(q < 1) > 50 and np.sum(q > 1) > 50
    c = cr.family("fixed")
    assert c["fixed_cams"].sum() == 3 and c["fixed_pts"].sum() == 37 and c["kc"] is not None and c["cov"] is not None


@pytest.mark.parametrize("case", [("fixed", 6), ("robust-cauchy", 6), ("robust-softl1", 6), ("rot", 11), ("dist", 16)],
                         ids=lambda c: f"{c[0]}-{c[1]}")
def test_text_over_mpmath_agrees_with_the_exact_values(case):
    import mpmath
    fam, cnp = case
    c = cr.family(fam)
    sel = np.arange(0, cr.NOBS, 37)
    xr = cr.gather(c, "raw", cnp, sel=sel)
    ex, Ax, Bx, sx = cr.exact(xr)
    tol = 2.0 ** -62  # both sides are exact to 60 digits: what is left is the rounding to the long double
    with mpmath.workdps(cr.DPS):
        for a in range(sel.size):
            e, A, B = cr.linearize(cr.at_mpf(xr, a))
            for got, want in ((e, ex[a]), (A, Ax[a]), (B, Bx[a])):
                for g, w in zip(got, want):
                    assert abs(cr._to_ld(mpmath.mpf(g)) - w) <= tol * abs(w), (fam, cnp, a, g, w)
            if cnp == 6:
                e, s = cr.residual(cr.at_mpf(xr, a))
                assert abs(cr._to_ld(s) - sx[a]) <= tol * abs(sx[a])
                assert all(abs(cr._to_ld(g) - w) <= tol * abs(w) for g, w in zip(e, ex[a]))


def _flagged(c, mutate, cnp=6):
    """does the mutated fp64 text leave the bound anywhere?  -> worst ratio per quantity"""
    eE, AE, BE = cr.linearize(cr.gather(c, "E", cnp))
    ef, Af, Bf = cr.linearize(cr.gather(c, "f64", cnp), mutate)
    ex, Ax, Bx, _ = cr.exact(cr.gather(c, "raw", cnp))
    return {q: ar.excess(cr.stack(f)[0], x, cr.stack(E)[1])[0] for q, E, f, x in
            (("e", eE, ef, ex), ("A", AE, Af, Ax), ("B", BE, Bf, Bx))}


def test_mutations_are_flagged():
    c = cr.family("benign")
    assert max(_flagged(c, None).values()) <= 1.0
    r = _flagged(c, "recip")  # a reciprocal with a relative error of 2^-48: 32 ulps
    print(f"\nreciprocal 2^-48 off: worst ratio e {r['e']:.1f}, A {r['A']:.1f}, B {r['B']:.1f}")
    assert r["A"] > 1.0 and r["B"] > 1.0 and r["e"] > 1.0
    # the distortion Jacobian with 6 k4 x written as 2 k4 x, on the benign geometry with a mild lens
    lens = dict(c, kc=cr.family("fixed")["kc"])
    assert max(_flagged(lens, None).values()) <= 1.0
    r = _flagged(lens, "k4")
    print(f"6 k4 x as 2 k4 x: worst ratio e {r['e']:.3f}, A {r['A']:.3g}, B {r['B']:.3g}")
    assert r["A"] > 1.0 and r["B"] > 1.0 and r["e"] <= 1.0  # (the residual does not see the Jacobian)


def test_zero_distortion_is_the_plain_model():
    """camera 8 of `dist` has kc = 0 exactly: the distortion text must agree with the plain model within the bound"""
    c = cr.family("dist")
    sel = np.flatnonzero(np.asarray(c["prob"]["jidx"]) == 8)
    assert sel.size > 20
    plain = dict(c, kc=None)
    xd, xp = cr.exact(cr.gather(c, "raw", sel=sel)), cr.exact(cr.gather(plain, "raw", sel=sel))
    for d, p in zip(xd, xp):
        assert np.all(np.abs(d - p) <= 2.0 ** -62 * np.abs(p))  # the exact values coincide
    Ed, Ep = cr.linearize(cr.gather(c, "E", sel=sel)), cr.linearize(cr.gather(plain, "E", sel=sel))
    fd, fp = cr.linearize(cr.gather(c, "f64", sel=sel)), cr.linearize(cr.gather(plain, "f64", sel=sel))
    for q, k in (("e", 0), ("A", 1), ("B", 2)):
        bd, bp = cr.stack(Ed[k])[1], cr.stack(Ep[k])[1]
        judge("dist, kc = 0", q + " against exact plain", cr.stack(fd[k])[0], xp[k], bd)
        judge("dist, kc = 0", q + " against fp64 plain", cr.stack(fd[k])[0], cr.stack(fp[k])[0].astype(cr.LD), bd + bp)


def test_refusals_and_exact_operations():
    x = cr.E(np.array([1.0, 2.0]), np.array([0.0, 0.0]))
    tiny = cr.E(np.array([1e-20, 1.0]), np.array([1e-20, 0.0]))  # the first entry's bound reaches its magnitude
    with pytest.raises(cr.Refused):
        x / tiny
    with pytest.raises(cr.Refused):
        cr.sqrt(tiny)
    assert not np.any((2.0 * x).b) and not np.any((-x).b) and not np.any((x + 0.0).b) and not np.any((0.0 + x).b)
    assert np.all((3.0 * x).b == cr.U * 3.0 * x.m) and np.all((x * x).b == cr.U * x.m * x.m)
    assert np.all((x + x).b == cr.U * np.abs(2 * x.v)) and np.all((1.0 / x).b == cr.U / np.abs(x.v))
    amb = cr.select_le(cr.E([4.0, 1.0], [1e-3, 0.0]), 4.0, 1.0, cr.E([1.5, 7.0], [0.25, 0.5]))
    assert np.all(amb.v == [1.0, 1.0]) and np.all(amb.b == [2 * 0.25 + 0.5, 0.0])


def _slack_rows(name, case, proj_m):
    """twice the derived bound over the slack tests/assembly_ref.py allows, per entry"""
    eE, AE, BE = cr.linearize(cr.gather(case, "E"))
    (rE, _) = cr.residual(cr.gather(case, "E"))
    be = np.maximum(cr.stack(eE)[1], cr.stack(rE)[1])
    m, proj, L = proj_m
    es = ar.residual_slack(m, proj, L)
    js = ar.JACOBIAN_SLACK if case.get("loss") is None else ar.robust_jac_slack(es, case["loss"][1])[:, None]
    rows = []
    for what, twice, allowed in (("e", 2 * be, es), ("A", 2 * cr.stack(AE)[1], js * np.abs(cr.stack(AE)[0].astype(np.float64))),
                                 ("B", 2 * cr.stack(BE)[1], js * np.abs(cr.stack(BE)[0].astype(np.float64)))):
        ok = allowed > 0
        r = twice[ok] / allowed[ok]
        rows.append(f"  {name} {what}: 2 bound / slack median {np.median(r):.2e}, largest {r.max():.2e}, "
                    f"{int(np.sum(r > 1))} of {r.size} entries above 1")
    return rows


def test_slack_report(problems):
    """A report, asserted nowhere: RESIDUAL_SLACK and JACOBIAN_SLACK against twice the derived bound (two kernels that
    each stay within the bound differ by at most twice it) on the problems of the entrywise suites."""
    from lens_twin import Twin, whitening
    from test_gpu_robust import _one_try_case
    rows = []
    for name in ("54cams", "trafalgar21"):
        prob = problems[name]
        case = dict(prob=prob, kc=None, cov=None, loss=None)
        m = np.asarray(prob["impts"], dtype=np.float64).reshape(-1, 2)
        rows += _slack_rows(name, case, (m, Twin(prob).project(), None))
    prob, kc, cov = _one_try_case("default")
    case = dict(prob=prob, kc=kc, cov=cov, loss=(cr.LOSS_HUBER, 2.0))
    m = np.asarray(prob["impts"], dtype=np.float64).reshape(-1, 2)
    rows += _slack_rows("lens54", case, (m, Twin(prob, kc).project(), whitening(np.asarray(cov).reshape(-1, 2, 2))))
    print("\ntwice the derived bound against the slacks of assembly_ref.py:\n" + "\n".join(rows))
