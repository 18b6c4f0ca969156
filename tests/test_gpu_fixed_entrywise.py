"""Fixed parameter blocks (psba_set_fixed) beyond the masked cases of tests/test_gpu_assembly_entrywise.py, with its
judges and the reference of tests/fixed_ref.py.  Needs an MI355X.
  * the maximum over the free blocks only, on 54cams scaled by 2^-22: there the largest free diagonal entry lies below
    the placeholder, so a k_max_diag_fixed that forgot the mask returns another number (on the unscaled problems the
    free entries are 1e7 .. 1e13 and it would not);
  * k_newp_fixed (psba_set_step): the proposal's fixed blocks carry the current bits, a -0.0 included;
  * structure-only (every camera fixed): the shortcut and PSBA_FIXED_NO_SHORTCUT=1 entry by entry and against each
    other bit for bit (the mu = 0 run with a one-view point is not here: see DESIGN 7c);
  * look-ahead: the try after psba_linearize_ahead / psba_accept, the only place where k_fixed_diag writes the
    alternate set of outputs."""
import os

import numpy as np
import pytest

import assembly_ref as ar
import fixed_ref as fr
import test_gpu_assembly_entrywise as ae
from sba_text import read_problem

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    mine = {k: v for k, v in ae.WORST.items() if k[0].startswith(("structure-only", "look-ahead"))}
    if mine:
        routes = sorted({r for r, _ in mine})
        lines = [f"  {r}: " + ", ".join(f"{q} {v:.2e}" for (rr, q), v in mine.items() if rr == r) for r in routes]
        print("\nworst bound ratio per route and quantity:\n" + "\n".join(lines))


def _params(h, which=0):
    cams, pts = h.get_params(which)
    return np.r_[cams.reshape(-1), pts.reshape(-1)]


# ---- the maximum over free blocks only ---------------------------------------------------------------------------

def test_maximum_excludes_the_placeholder(problems):
    from fixed_twin import fixed_pieces
    base = problems["54cams"]
    prob = fr.scaled_problem(base)
    fc, fp, info = ae.mask_of("54cams-scaled", "mixed", prob)
    # from the twin, before the GPU: the largest free diagonal entry lies below the placeholder, and no V + mu I comes
    # near sym3_inverse's absolute 1e-16 singular flag
    _, _, lin = fixed_pieces(prob, fc, fp)
    U, V = lin["U"].reshape(-1, 6, 6), lin["V"].reshape(-1, 3, 3)
    m = fr.free_max(U, V, fc, fp)
    det = np.linalg.det(V[fp == 0] + 1e-3 * m * np.eye(3))
    print(f"\nscaled 54cams, {info}: twin's largest free diagonal entry {m:.4f}, smallest det(V + mu I) {det.min():.2e}")
    assert 0.5 < m < 0.75 and det.min() > 1e-10
    h = ae._handle(prob, None, fixed=(fc, fp))
    try:
        JA, JB = h.compute_jacobiQT()
        ex = h.compute_exQT()
        for coeff, coeff_g in ((1.0, 1.0), (2.0, -2.0)):  # the placeholder is 1, then 2
            k1 = fr.install(ar.k1_sums(JA, JB, ex, prob["iidx"], prob["jidx"], prob["nC"], prob["nP"], coeff, coeff_g),
                            fc, fp, coeff)
            Ux, Vx = k1["U"][0].astype(np.float64), k1["V"][0].astype(np.float64)
            want, leaked = fr.free_max(Ux, Vx, fc, fp), fr.all_max(Ux, Vx)
            assert leaked == coeff and want < 0.75 * coeff and abs(want - coeff * m) <= 1e-9 * want
            h.linearize(coeff, coeff_g)
            got = {"psba_max_diag": h.max_diag(), "psba_maxElmOfUV": h.maxElmOfUV(),
                   "psba_begin": h.begin(coeff, coeff_g)[1]}
            for what, v in got.items():
                print(f"coefficients ({coeff}, {coeff_g}): {what} {v!r}, over the free blocks {want!r}, "
                      f"rel {abs(v - want) / want:.2e}")
                assert abs(v - want) <= 1e-12 * want, f"{what} {v!r}: the maximum over the free blocks is {want!r}"
        k1 = ar.k1_sums(JA, JB, ex, prob["iidx"], prob["jidx"], prob["nC"], prob["nP"])
        want = 1e-3 * fr.free_max(k1["U"][0].astype(np.float64), k1["V"][0].astype(np.float64), fc, fp)
        res, _ = h.levmar(max_iter=1)
        print(f"psba_levmar: mu0 {res.mu0!r}, 1e-3 times the maximum over the free blocks {want!r}")
        assert abs(res.mu0 - want) <= 1e-12 * want
    finally:
        h.close()


# ---- k_newp_fixed --------------------------------------------------------------------------------------------------

def test_set_step_keeps_the_bits_of_fixed_blocks(problems):
    prob = problems["54cams"]
    fc, fp, _ = ae.mask_of("54cams", "mixed", prob)
    fx = fr.fixed_entries(fc, fp)
    h = ae._handle(prob, None, fixed=(fc, fp))
    try:
        assert ae.minus_zero_rotation(h) == 3, "camera 0's local rotation starts at 0"
        cur = _params(h)
        assert np.all(np.signbit(cur[:3]))
        rng = np.random.default_rng(12)
        step = 1e-3 * rng.normal(size=cur.size)
        # the contract under test (include/psba_hip.h): psba_set_step ignores the fixed entries of dp
        # whatever they hold and zeroes them -- k_newp_fixed selects before it adds, so a NaN there reaches nothing
        step[np.flatnonzero(fx)[::2]] = np.nan
        step[0] = 0.0  # -0.0 + 0.0 = +0.0: a sum in place of the select shows here
        h.set_step(step)
        new = _params(h, 1)
        assert fr.same_bits(new[fx], cur[fx]), "psba_set_step: the proposal's fixed blocks are not the current bits"
        assert fr.same_bits(new[~fx], (cur + step)[~fx])
        assert fr.plus_zero(h.get_dp()[fx]), "psba_set_step: dp of a fixed block is not +0.0"
        assert fr.same_bits(h.get_dp()[~fx], step[~fx])
    finally:
        h.close()


# ---- structure-only ------------------------------------------------------------------------------------------------

def _nine():
    return read_problem(os.path.join(DATA, "9cams.txt"), os.path.join(DATA, "9pts.txt"))


def _structure_only_try(route, prob, mu, judge):
    """one try with every camera fixed; mu None: 1e-3 max diag.  Returns (status, dp, mu)."""
    from psba_amd import capi
    nC, nP = int(prob["nC"]), int(prob["nP"])
    nA = 6 * nC
    fixed = (np.ones(nC, dtype=np.uint8), np.zeros(nP, dtype=np.uint8))
    h = ae._handle(prob, None, fixed=fixed)
    try:
        JA, JB = h.compute_jacobiQT()
        ex = h.compute_exQT()
        assert fr.plus_zero(JA) and np.all(np.any(JB.reshape(-1, 6) != 0, axis=1))
        h.linearize(1.0, 1.0)
        if mu is None:
            mu = 1e-3 * h.max_diag()
        h.schur_assemble(mu)
        h.schur_reduce()
        assert h.schur_solve() == capi.PSBA_OK
        sc = h.backsub(mu)
        dp = h.get_dp()
        assert fr.plus_zero(dp[:nA]), f"{route}: dp_a is not +0.0"
        newp = _params(h, capi.PARAMS_NEW)
        assert fr.same_bits(newp[:nA], _params(h)[:nA])
        if judge:
            assert sc.status == 0
            e_new = h.compute_exQT(capi.PARAMS_NEW)
            s_new = (ar.ld(e_new).reshape(-1, 2) ** 2).sum(axis=1)
            ref, Wx, eW, gx, eg = ae._fused_reference(JA, JB, ex, prob, 1.0, 1.0, None, mu, fixed=fixed)
            assert not np.any(Wx) and not np.any(eW)  # dp_b = (V + mu I)^-1 g_b
            sums = {k: getattr(sc, k) for k in ("dp_l2", "gain_den", "new_cost", "newp_l2")}
            ae._judge_k3(route, prob, ref, dp, JA, JB, ex, Wx, eW, gx, eg, 1.0, False, sums, newp, s_new, e_new, mu, None)
        return sc.status, dp, mu
    finally:
        h.close()


def _both_routes(label, prob, mu, judge, monkeypatch):
    monkeypatch.delenv("PSBA_FIXED_NO_SHORTCUT", raising=False)
    st0, dp0, mu = _structure_only_try(f"structure-only{label} (shortcut)", prob, mu, judge)
    monkeypatch.setenv("PSBA_FIXED_NO_SHORTCUT", "1")
    st1, dp1, _ = _structure_only_try(f"structure-only{label} (general route)", prob, mu, judge)
    assert st0 == st1, f"status {st0} with the shortcut, {st1} on the general route"
    assert fr.same_bits(dp0, dp1), "dp differs between the shortcut and the general route"
    return st0


def test_structure_only_entrywise_and_bit_for_bit(monkeypatch):
    assert _both_routes("", _nine(), None, True, monkeypatch) == 0


# ---- look-ahead ----------------------------------------------------------------------------------------------------

def test_lookahead_linearization_under_the_mask(problems):
    """backsub_async, linearize_ahead, backsub_wait, accept on rows-54cams under the mixed mask, then the next try
    through the fused judge at the accepted parameters, the blocks from a fresh dump on a second handle."""
    from psba_amd import capi
    prob = problems["54cams"]
    fc, fp, _ = ae.mask_of("54cams", "mixed", prob)
    fixed = (fc, fp)
    fx = fr.fixed_entries(fc, fp)
    h = ae._handle(prob, None, fixed=fixed)
    h2 = ae._handle(prob, None, fixed=fixed)
    try:
        assert h.schur_path() == 0
        ae.minus_zero_rotation(h)
        cur = _params(h)
        cost = h.begin(1.0, 1.0)[0]
        mu = 1e-3 * h.max_diag()
        h.schur_assemble(mu)
        h.schur_reduce()
        assert h.schur_solve() == capi.PSBA_OK
        h.backsub_async(mu)
        h.linearize_ahead()
        sc = h.backsub_wait()
        assert sc.status == 0 and sc.new_cost < cost
        h.accept()
        acc = _params(h)
        assert fr.same_bits(acc[fx], cur[fx]) and not np.array_equal(acc[~fx], cur[~fx])
        # the blocks at the accepted parameters, from a fresh dump
        h2.set_params(acc[:6 * prob["nC"]], acc[6 * prob["nC"]:])
        assert fr.same_bits(_params(h2), acc)
        JA, JB = h2.compute_jacobiQT()
        ex = h2.compute_exQT()
        # psba_linearize adopts the linearization queued ahead: it launches nothing
        h.profile_enable(True)
        h.profile_reset()
        h.linearize(1.0, 1.0)
        assert h.profile_get(capi.K_LINEARIZE)[1] == 0, "psba_linearize ran K1 again after psba_accept"
        md = h.max_diag()
        k1 = ar.k1_sums(JA, JB, ex, prob["iidx"], prob["jidx"], prob["nC"], prob["nP"])
        want = fr.free_max(k1["U"][0].astype(np.float64), k1["V"][0].astype(np.float64), fc, fp)
        assert abs(md - want) <= 1e-12 * want, (md, want)
        with ae.exact_parts():
            ae.fused_layer("look-ahead", h, prob, JA, JB, ex, 1e-3 * md, 1.0, 1.0, None, False, False, fixed,
                           linearize=False)
    finally:
        h.close()
        h2.close()
