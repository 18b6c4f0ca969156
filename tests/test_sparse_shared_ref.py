"""The host reference of shared intrinsics under the block-sparse solver (tests/sparse_shared_ref.py) judged
on the host alone: the float64 transcription of the fold product and of the folded diagonal blocks against the
long-double ones under the derived bounds (the ratios are printed), three injected faults that the judges must refuse,
and the iteration counts of the grouped conjugate gradients on the inputs of the GPU tests, which keep every one of them
inside the default cap of 500 by the reference alone."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import freepcg_ref as fp
import shared_ref as sr
import sparse_shared_ref as ss
from freekd_twin import BAL, tiny_problem, wide_problem
from test_freekd_twin import P7

pytestmark = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")

MASKS = {"all": fr.ALL, "bal": BAL}
INPUTS = {
    "tiny": lambda: (tiny_problem(), np.zeros(2, dtype=np.int32)),
    "P7-one": lambda: (P7(), np.zeros(7, dtype=np.int32)),
    "P7-two": lambda: (P7(), np.array([0, 1, 0, 1, 0, 1, 0], dtype=np.int32)),
    "wide": lambda: (wide_problem(65), sr.wide_labels(65).astype(np.int32)),
    "one-group": lambda: (wide_problem(65), np.zeros(65, dtype=np.int32)),
}
# iterations of the grouped twin at tol 1e-10: (at mu = 1e-3 max diag, at the small damping of shared_ref.dampings), as
# the float64 conjugate gradients on the 80-bit folded S gave them when the inputs were chosen.  At the big mu the
# long-double twin gives these very counts.  At the small mu the systems are ill-conditioned and the count depends on
# the rounding of the recurrences: the long-double twin needs 7 to 20 % fewer iterations, the float64 twin is held to
# the figure within max(2, 10 %) -- the band says that the inputs stay inside the default cap of 500 with the
# exception the GPU tests make (wide, all ten free, small mu: max_iter = 2000), not which rounding is right
COUNTS = {("tiny", "all"): ((7, 9), (11, 13)), ("tiny", "bal"): ((7, 9), (11, 13)),
          ("P7-one", "bal"): ((17, 17), (83, 83)), ("P7-two", "bal"): ((17, 17), (90, 90)),
          ("wide", "bal"): ((40, 40), (166, 166)), ("one-group", "bal"): ((34, 34), (89, 89)),
          ("wide", "all"): ((62, 62), (470, 470))}


@functools.lru_cache(maxsize=None)
def case(name, mask):
    p, lab = INPUTS[name]()
    rt = sr.SharedRoute(p, lab, MASKS[mask])
    sm = fr.sums(rt)
    mus, _ = sr.dampings(rt, sm)
    return rt, mus


@functools.lru_cache(maxsize=None)
def blocks(name, mask, which_mu):
    rt, mus = case(name, mask)
    return ss.dense_blocks(rt, mus[which_mu])


def folded(name, mask, which_mu, dtype):
    rt, mus = case(name, mask)
    jk, val, ea = blocks(name, mask, which_mu)
    fo = ss.FoldedOp(rt.nC, jk, val.astype(dtype), rt.rep, rt.free, mus[which_mu], dtype=dtype)
    return rt, fo, ss.fold_ea(ea.astype(dtype), fo.phi, fo.away)


@pytest.mark.parametrize("name,mask", [("tiny", "all"), ("P7-two", "bal"), ("wide", "all"), ("wide", "bal"), ("one-group", "bal")])
def test_float64_fold_product_within_the_bound_and_the_faults_outside(name, mask):
    rt, fx, _ = folded(name, mask, "small", ss.LD)
    _, f64, _ = folded(name, mask, "small", np.float64)
    # the folded operator is the fold of shared_ref on a dense matrix
    S = fp.dense_of(rt.nC, *blocks(name, mask, "small")[:2], 16)
    k = np.arange(rt.nA)
    S[k, k] += ss.LD(fx.mu)
    want, _ = sr.fold(S, np.zeros(rt.nA, dtype=ss.LD), rt.rep, rt.free, fx.mu)
    worst = 0.0
    member = int(np.flatnonzero(fx.away)[0]) // 16
    for what, x in fp.product_vectors(rt.nC, 16):
        exact = fx.times(x)
        assert float(np.abs(exact - want @ x.astype(ss.LD)).max()) <= 1e-17 * float(np.abs(want).max() * np.abs(x).max() * rt.nA)
        bound = f64.product_bound(x)
        ratio, at = ar.excess(f64.times(x), exact, bound)
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{name} {mask}, x = {what}: entry {at} is {ratio:.3e} of the bound"
        assert np.array_equal(f64.times(x)[fx.away], f64.placeholder_product(x))
        if what == "ones":
            for fault in (dict(mu_per_member=True), dict(skip_member=member)):
                bad, _ = ar.excess(f64.times(x, **fault), exact, bound)
                assert bad > 1.0, f"{name} {mask}: the fault {fault} passes the product's judge ({bad:.3e})"
    print(f"{name} {mask}: float64 fold product / bound {worst:.3e}")


@pytest.mark.parametrize("name,mask", [("tiny", "all"), ("P7-one", "bal"), ("wide", "all"), ("wide", "bal")])
@pytest.mark.parametrize("which_mu", ["big", "small"])
def test_float64_folded_blocks_and_their_inverses(name, mask, which_mu):
    rt, fx, _ = folded(name, mask, which_mu, ss.LD)
    _, f64, _ = folded(name, mask, which_mu, np.float64)
    B, E = ss.folded_blocks(fx)
    B64, _ = ss.folded_blocks(f64)
    ratio, at = ar.excess(B64, B, E)
    assert ratio <= 1.0, f"{name} {mask} {which_mu}: folded block entry {at} is {ratio:.3e} of its bound"
    M, bad = fp.block_inverse(B64)
    Mx, _ = fp.block_inverse(ss.folded_blocks(f64, drop_cross=True)[0])
    assert not bad.any()
    worst, fault_seen = 0.0, False
    for j in range(rt.nC):
        kappa, allowed = ss.precond_bound(B[j], E[j])
        found = ss.precond_residual(M[j], B[j])
        worst = max(worst, found / allowed)
        assert found <= allowed, f"{name} {mask} {which_mu}: camera {j}: {found:.3e} > {allowed:.3e} (kappa {kappa:.2e})"
        fault_seen |= ss.precond_residual(Mx[j], B[j]) > allowed
        aw = np.flatnonzero(fx.away[16 * j:16 * j + 16])
        off = M[j].copy()
        off[aw, aw] = 0.0
        assert np.all(off[aw, :] == 0.0) and np.all(off[:, aw] == 0.0)
    assert fault_seen, "a preconditioner block without the cross-member blocks passes the judge"
    print(f"{name} {mask} {which_mu}: blocks {ratio:.3e}, || M B - I || / allowed {worst:.3e}")


@pytest.mark.parametrize("name,mask", list(COUNTS))
def test_iteration_counts_stay_inside_the_cap(name, mask):
    for which_mu, dtype, (lo, hi) in zip(("big", "small"), (ss.LD, np.float64), COUNTS[(name, mask)]):
        rt, fo, b = folded(name, mask, which_mu, dtype)
        t = ss.twin_pcg(fo, b, 1e-10, 500)
        print(f"{name} {mask} {which_mu}: {t['iters']} iterations, relres {t['relres']:.3e}")
        slack = 0 if which_mu == "big" else max(2, (hi + 9) // 10)
        assert t["converged"] and lo - slack <= t["iters"] <= hi + slack, f"{name} {mask} {which_mu}: {t['iters']} iterations"
        assert t["iters"] < 500
        _, fx, bx = folded(name, mask, which_mu, ss.LD)
        tr, unit = ss.relres_and_gap(fx, t["x"], bx, t["iters"])
        assert tr <= 1e-10 + fp.C_GAP * unit
        x = t["x"].reshape(-1, 16)
        assert np.array_equal(x[:, :10], x[rt.rep][:, :10])


def test_the_twin_needs_the_members():
    """a member left out of the fold, or mu counted once per member, changes the solution beyond the judge of the solve"""
    rt, fx, b = folded("P7-two", "bal", "big", ss.LD)
    member = int(np.flatnonzero(fx.away)[0]) // 16
    for fault in (dict(mu_per_member=True), dict(skip_member=member)):
        t = ss.twin_pcg(fx, b, 1e-10, 500, **fault)
        tr, unit = ss.relres_and_gap(fx, t["x"], b, max(t["iters"], 1))
        assert not tr <= 1e-10 + fp.C_GAP * unit, f"{fault}: true residual {tr:.3e} passes"
