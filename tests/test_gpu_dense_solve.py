"""Every route of the dense solve S dpa = e_a against the extended-precision host reference (tests/dense_ref.py).

The chain (kernels_chol_graph.hip) picks its route by n32 = 6 nC rounded up to 32; psba_set_reduce_buffer puts a
chosen matrix into it and psba_chol_shape says which route ran.  Each case: a handle on a tiny synthetic problem with
the camera count of the route, psba_linearize once, then per matrix psba_schur_assemble (any mu: it makes the buffer
current and stamps the try), psba_set_reduce_buffer, psba_SPDinv_matVec.  Judged by the normwise backward error eta
(fixed bound 1e-14), the forward error against the refined reference where n <= 4416 (2 kappa 1e-14), exact zeros
for b = 0, PSBA_NOT_SPD for a first bad pivot at chosen places, bit-identical repeats, and the switches of the chain
against its default route."""

import numpy as np
import pytest

import dense_ref as dr

pytestmark = pytest.mark.gpu

ETA_MAX = 1e-14
KAPPA = 1e3  # the sweep's low-rank matrix
REFINE_MAX_N = 4416  # O(n^3) host work only up to here
PSBA_OK, PSBA_NOT_SPD = 0, 1

# the route by camera count (6 nC padded to n32): (fused, solve width, fused2, blocked, NB, diagonal-only steps)
ROUTES = [
    (1, 106, "fused<10>", dict(fused=True, fused2=False, blocked=False)),
    (107, 170, "fused<16>", dict(fused=True, fused2=False, blocked=False)),
    (171, 229, "fused2", dict(fused=False, fused2=True, blocked=False)),
    (230, 293, "flat", dict(fused=False, fused2=False, blocked=False)),
    (294, 730, "two-level all-rows", dict(fused=False, fused2=False, blocked=True, NB=256, diag_only=False,
                                          lookahead=True)),
    (731, 1360, "two-level diagonal-only", dict(fused=False, fused2=False, blocked=True, NB=256, diag_only=True,
                                                lookahead=True)),
    (1361, 10**9, "two-level NB=384", dict(fused=False, fused2=False, blocked=True, NB=384, diag_only=True,
                                           lookahead=True)),
]
SWEEP = [2, 5, 6, 106, 107, 170, 171, 229, 230, 293, 294, 300, 730, 731, 760, 1000, 1360, 1361, 2000]
SPECTRUM_AT = [6, 106, 170, 229, 293, 300]  # one size per route where n <= 2048 (O(n^3) host work)
GRADED_AT = [6, 170, 229, 293, 300, 1000]


def route_of(cams):
    for lo, hi, name, want in ROUTES:
        if lo <= cams <= hi:
            return name, want
    raise AssertionError(cams)


def check_route(h, cams, **extra):
    name, want = route_of(cams)
    want = dict(want, single=False, **extra)
    got = h.chol_shape()
    assert got["n32"] == dr.n32_of(6 * cams)
    bad = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not bad, f"{cams} cameras: route {name} expected, psba_chol_shape says {got} (differs in {bad})"
    return name


class Case:
    """A handle on a synthetic problem with `cams` cameras, and the sweep's matrix for its size."""

    def __init__(self, cams):
        import psba_amd
        import psba_amd.synth as synth
        self.cams, self.n = cams, 6 * cams
        self.n32 = dr.n32_of(self.n)
        self.prob = synth.make_problem(n_cams=cams, n_pts=max(8, 2 * cams), mean_track=5.0, seed=cams)
        self.h = self.handle()
        self.buf = dr.lowrank_shift(self.n, KAPPA, cams)
        self.A = dr.matrix(self.buf, self.n)
        self.Anorm = dr.norm_inf_mat(self.A)
        self.b, _ = dr.rhs_for(self.A, cams)
        dr.set_rhs(self.buf, self.n, self.b)
        self.ref = dr.refined_solution(self.A, self.b) if self.n <= REFINE_MAX_N else None
        self.dpa = None  # the default route's solution of the sweep's matrix, once it has passed the checks

    def handle(self):
        import psba_amd
        h = psba_amd.Psba(0)
        h.upload_problem(self.prob)
        h.linearize(1.0, 1.0)
        return h

    def solve(self, buf=None, h=None):
        h = self.h if h is None else h
        h.schur_assemble(1.0)
        h.set_reduce_buffer(self.buf if buf is None else buf)
        rc, dpa = h.SPDinv_matVec()
        return rc, dpa

    def check(self, rc, dpa, A=None, b=None, ref=None, kappa=KAPPA, Anorm=None, what="", label=None):
        """rc == PSBA_OK, eta <= 1e-14 and (with a reference) the forward error within 2 kappa 1e-14; returns eta.
        The sweep's own matrix and right-hand side when A is None."""
        if A is None:
            A, b, ref, Anorm = self.A, self.b, self.ref, self.Anorm
        assert rc == PSBA_OK, f"{self.cams} cameras {what}: rc {rc}"
        assert np.all(np.isfinite(dpa)), f"{self.cams} cameras {what}: non-finite dpa with PSBA_OK"
        eta = dr.backward_error(A, dpa, b, Anorm)
        ETAS.setdefault(label or route_of(self.cams)[0], []).append(eta)
        assert eta <= ETA_MAX, f"{self.cams} cameras {what}: eta {eta:.3e}"
        if ref is not None:
            fe = dr.forward_error(dpa, ref)
            assert fe <= 2 * kappa * 1e-14, f"{self.cams} cameras {what}: forward error {fe:.3e} (kappa {kappa:.0e})"
        return eta

    def check_good(self, what):
        """The sweep's matrix on this handle once more (after a failure, a switch, ...): identical to the solution that
        passed the checks before, or passing them itself."""
        rc, dpa = self.solve()
        if self.dpa is not None and rc == PSBA_OK and np.array_equal(dpa, self.dpa):
            return
        self.check(rc, dpa, what=what)

    def close(self):
        self.h.close()


ETAS = {}  # largest eta per route, printed at the end of the module
_CASES = {}


def case(cams):
    if cams not in _CASES:
        _CASES[cams] = Case(cams)
    return _CASES[cams]


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for c in _CASES.values():
        c.close()
    _CASES.clear()
    if ETAS:
        print("\nlargest eta per route: " + ", ".join(f"{k} {max(v):.2e} ({len(v)})" for k, v in ETAS.items()))


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def mismatch_report(route, a, b):
    d = np.flatnonzero(a.view(np.int64) != b.view(np.int64))
    rows = ", ".join(f"[{i}] {a[i]:.17e} vs {b[i]:.17e} (diff {a[i] - b[i]:.2e})" for i in d[:12])
    return f"route {route}: {d.size} of {a.size} elements differ: {rows}"


# ---- the sweep ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cams", SWEEP)
def test_route_sweep(cams):
    """Both sides of every size limit of the chain: the route, eta, the forward error, b = 0 and b = e_last."""
    c = case(cams)
    check_route(c.h, cams)
    rc, dpa = c.solve()
    c.check(rc, dpa, what="b = A x*")
    c.dpa = dpa
    # b = 0: exactly zero
    zero = c.buf[-1].copy()
    try:
        c.buf[-1] = 0.0
        rc, dz = c.solve()
        assert rc == PSBA_OK and not np.any(dz), f"b = 0 gives |dpa| up to {np.abs(dz).max():.2e}"
        # one non-zero entry, in the last real column
        bl = dr.rhs_last(c.n, 1.0 / c.A[-1, -1])
        dr.set_rhs(c.buf, c.n, bl)
        rc, dl = c.solve()
        ref = dr.refined_solution(c.A, bl) if c.n <= REFINE_MAX_N else None
        c.check(rc, dl, c.A, bl, ref, KAPPA, c.Anorm, what="b = e_last")
    finally:
        c.buf[-1] = zero


@pytest.mark.parametrize("cams", SPECTRUM_AT)
@pytest.mark.parametrize("kappa", [1e2, 1e6, 1e10])
def test_spectrum_family(cams, kappa):
    c = case(cams)
    check_route(c.h, cams)
    buf = dr.spectrum(c.n, kappa, cams)
    A = dr.matrix(buf, c.n)
    b, _ = dr.rhs_for(A, cams + 1)
    dr.set_rhs(buf, c.n, b)
    rc, dpa = c.solve(buf)
    c.check(rc, dpa, A, b, dr.refined_solution(A, b), kappa, what=f"spectrum kappa {kappa:.0e}")
    c.check_good("after the spectrum matrix")


@pytest.mark.parametrize("cams", GRADED_AT)
def test_graded_family(cams):
    """D C D with D = 2^e, e in [-20, 20]: dpa = D^-1 y with y the GPU's solution of C y = D^-1 b, within a tolerance
    set by kappa(C) = 100 -- kappa(A) is beyond 1e20 and says nothing."""
    c = case(cams)
    buf, cbuf, d = dr.graded(c.n, cams)
    A, C = dr.matrix(buf, c.n), dr.matrix(cbuf, c.n)
    b, _ = dr.rhs_for(A, cams + 2)
    dr.set_rhs(buf, c.n, b)
    rc, x = c.solve(buf)
    c.check(rc, x, A, b, what="graded A")
    dr.set_rhs(cbuf, c.n, b / d)
    rc, y = c.solve(cbuf)
    c.check(rc, y, C, b / d, dr.refined_solution(C, b / d) if c.n <= REFINE_MAX_N else None, 100.0, what="graded C")
    err = np.abs(d * x - y).max() / np.abs(y).max()
    assert err <= 2 * 100.0 * 1e-14, f"{cams} cameras: D x against y {err:.3e}"


@pytest.mark.parametrize("cams", [5, 80])
def test_single_workgroup_route(cams, monkeypatch):
    monkeypatch.setenv("PSBA_CHOL_SINGLE", "1")
    c = case(cams)
    assert c.h.chol_shape()["single"]
    rc, dpa = c.solve()
    c.check(rc, dpa, what="PSBA_CHOL_SINGLE")
    dz = c.buf[-1].copy()
    try:
        c.buf[-1] = 0.0
        rc, z = c.solve()
        assert rc == PSBA_OK and not np.any(z)
    finally:
        c.buf[-1] = dz


# ---- failures --------------------------------------------------------------------------------------------------

def _pivots(cams):
    n = 6 * cams
    NB = 384 if cams >= 1361 else 256
    ks = {0, 31, 32, n - 1}
    if cams >= 294:
        ks |= {NB - 1, NB}
    if 731 <= cams:  # a middle super-panel on the diagonal-only route, inside its block solve's rows
        ks.add((n // NB // 2) * NB + NB // 2 + 5)
    return sorted(k for k in ks if k < n)


FAIL_AT = [5, 106, 170, 229, 293, 300, 1000, 1361]


@pytest.mark.parametrize("cams,k,pivot", [(cams, k, p) for cams in FAIL_AT for i, k in enumerate(_pivots(cams))
                                          for p in ([-1.0] if i % 2 else [0.0])])
def test_first_bad_pivot_is_reported(cams, k, pivot):
    """An SPD matrix with row and column k zeroed and pivot k set to 0 or -1: PSBA_NOT_SPD, and the next good matrix
    on the same handle PSBA_OK and accurate (no stale status)."""
    c = case(cams)
    A = c.A
    row, dkk = A[k, :].copy(), A[k, k]
    try:
        A[k, :] = 0.0
        A[:, k] = 0.0
        A[k, k] = pivot
        rc, _ = c.solve()
    finally:
        A[k, :] = row
        A[:, k] = row
        A[k, k] = dkk
    assert rc == PSBA_NOT_SPD, f"{cams} cameras ({route_of(cams)[0]}): pivot {k} = {pivot} not flagged"
    c.check_good(f"after the failure at pivot {k}")


@pytest.mark.parametrize("cams", [5, 170, 229, 293, 300, 1000])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_entry_is_reported(cams, bad):
    c = case(cams)
    i, j = c.n - 1, c.n - 7
    keep = c.A[i, j]
    try:
        c.A[i, j] = bad  # one late entry of the lower triangle
        rc, _ = c.solve()
    finally:
        c.A[i, j] = keep
    assert rc == PSBA_NOT_SPD, f"{cams} cameras: {bad} at ({i}, {j}) not flagged"
    c.check_good(f"after {bad}")


# ---- determinism ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cams,reps", [(7, 16), (54, 16), (170, 16), (300, 16), (1000, 3), (2000, 3)])
def test_same_buffer_gives_identical_dpa(cams, reps):
    """The chain has no atomics on its data (the only one is the LDS flag poll of chol_factor32.h): the same buffer
    must give the same bits, on the same handle and on a fresh one.  A fixed number of repeats, no retry."""
    c = case(cams)
    name = route_of(cams)[0]
    rc, first = c.solve()
    assert rc == PSBA_OK
    for r in range(1, reps):
        rc, dpa = c.solve()
        assert rc == PSBA_OK
        assert bits_equal(dpa, first), f"repeat {r}: " + mismatch_report(name, dpa, first)
    if reps <= 3:
        h = c.handle()
        try:
            rc, dpa = c.solve(h=h)
        finally:
            h.close()
        assert rc == PSBA_OK
        assert bits_equal(dpa, first), "fresh handle: " + mismatch_report(name, dpa, first)
    c.check(PSBA_OK, first, what="determinism")


# ---- the first diagonal block as the LM loop has it ----------------------------------------------------------------

def _lm_path_solves(h, nA, reps, label):
    import psba_amd  # noqa: F401
    mu = 1e-3 * h.max_diag()
    for r in range(reps):
        h.schur_assemble(mu)
        S = h.get_reduce_buffer().reshape(-1, dr.n32_of(nA))
        A = np.tril(S[:nA, :nA])
        A = A + np.tril(A, -1).T
        b = S[-1, :nA].copy()
        h.schur_solve()
        dpa = h.get_dp()[:nA]
        eta = dr.backward_error(A, dpa, b)
        ETAS.setdefault("LM path (first block in k_schur_reduce)", []).append(eta)
        assert eta <= ETA_MAX, f"{label}, solve {r}: eta {eta:.3e} against the captured S"


@pytest.mark.parametrize("name", ["7cams", "54cams"])
def test_first_block_from_the_schur_reduce(name, problems):
    """On the LM path the first 32 x 32 block is factored inside k_schur_reduce, not by k_cholg_diag: 32 fresh
    assemblies of the real problem, each solve judged against the S it was given (psba_get_reduce_buffer)."""
    import psba_amd
    h = psba_amd.Psba(0)
    try:
        h.upload_problem(problems[name])
        h.linearize(1.0, 1.0)
        _lm_path_solves(h, h.nA, 32, name)
    finally:
        h.close()


def test_first_block_from_the_schur_reduce_at_300_cameras():
    c = case(300)
    h = c.handle()
    try:
        _lm_path_solves(h, c.n, 4, "300 cameras")
    finally:
        h.close()


# ---- switches of the chain -----------------------------------------------------------------------------------------

KNOBS = [
    ("PSBA_CHOL_LOOKAHEAD", "0", dict(lookahead=False)),
    ("PSBA_CHOL_LOOKAHEAD", "1", dict(lookahead=True)),
    ("PSBA_CHOL_TRSM_WAVE", "1", {}),
    ("PSBA_CHOL_STEPS_ALL_ROWS", "1", dict(diag_only=False)),
    ("PSBA_CHOL_STEPS_DIAG_ONLY", "1", dict(diag_only=True)),
    ("PSBA_CHOL_NEAR_FINE_MAX", "0", {}),
    ("PSBA_CHOL_NEAR_FINE_MAX", "100000", {}),
    ("PSBA_CHOL_COLS_FUSED_MAX", "0", {}),
    ("PSBA_CHOL_FAR_PAUSE", "0", {}),
    ("PSBA_CHOL_EVENT_SYSFENCE", "1", {}),
    ("PSBA_CHOL_SIDE_PRIO_DEFAULT", "1", {}),
    ("PSBA_CHOL_WIDE2", "1", dict(lookahead=False)),
    ("PSBA_CHOL_NB", "128", dict(NB=128)),
    ("PSBA_CHOL_NB", "512", dict(NB=512)),
    ("PSBA_CHOL_BACK_ONE_WG", "1", {}),
    ("PSBA_CHOL_BACK_SINGLE", "1", {}),
    ("PSBA_CHOL_FLAT", "1", dict(blocked=False)),
]
FRESH = {"PSBA_CHOL_EVENT_SYSFENCE", "PSBA_CHOL_SIDE_PRIO_DEFAULT"}  # read when the side stream / events are made


def _against_default(c, env, monkeypatch, expect=None, fresh=False):
    if c.dpa is None:
        rc, c.dpa = c.solve()
        c.check(rc, c.dpa, what="default route")
    for k, v in env:
        monkeypatch.setenv(k, v)
    h = c.handle() if fresh else c.h
    try:
        shape = h.chol_shape()
        for k, v in (expect or {}).items():
            assert shape[k] == v, f"{env}: psba_chol_shape {shape}"
        rc, dpa = c.solve(h=h)
    finally:
        if fresh:
            h.close()
        for k, _ in env:
            monkeypatch.delenv(k)
    what = " ".join(f"{k}={v}" for k, v in env)
    c.check(rc, dpa, what=what, label=f"switches at {c.cams} cameras")
    rel = np.abs(dpa - c.dpa).max() / np.abs(c.dpa).max()
    assert rel <= 1e-13, f"{c.cams} cameras {what}: {rel:.3e} from the default route"


@pytest.mark.parametrize("cams", [300, 1000])
@pytest.mark.parametrize("knob,value,expect", KNOBS, ids=[f"{k[10:]}={v}" for k, v, _ in KNOBS])
def test_switch_against_the_default_route(cams, knob, value, expect, monkeypatch):
    _against_default(case(cams), [(knob, value)], monkeypatch, expect, fresh=knob in FRESH)


def test_lookahead_off_at_12000_columns(monkeypatch):
    """one matrix of >= 6000 columns factored with and without the look-ahead's two streams."""
    c = case(2000)
    _against_default(c, [("PSBA_CHOL_LOOKAHEAD", "0")], monkeypatch, dict(lookahead=False))


FUSED_KNOBS = [
    ([("PSBA_CHOL_UNFUSED", "1")], dict(fused=False, fused2=True)),
    ([("PSBA_CHOL_FUSED_MAX", "0")], dict(fused=False, fused2=True)),
    ([("PSBA_CHOL_UNFUSED", "1"), ("PSBA_CHOL_FUSED2_MAX", "0")], dict(fused=False, fused2=False, blocked=False)),
    ([("PSBA_CHOL_GRAPH", "1")], dict(fused=True)),  # one stream at n32 <= 1024: nothing parallel is captured
]


@pytest.mark.parametrize("cams", [106, 170])
@pytest.mark.parametrize("env,expect", FUSED_KNOBS, ids=["unfused", "fused_max0", "flat", "graph"])
def test_fused_size_switches(cams, env, expect, monkeypatch):
    _against_default(case(cams), env, monkeypatch, expect)


# ---- the upper triangle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cams,env", [(5, None), (80, "PSBA_CHOL_SINGLE"), (106, None), (170, None), (229, None),
                                      (293, None), (300, None), (1000, None), (1361, None)])
def test_upper_triangle_is_not_read(cams, env, monkeypatch):
    """Every route reads the lower triangle of the buffer only (include/psba_hip.h, psba_set_reduce_buffer): unrelated
    values of the same scale above the diagonal leave dpa bit-identical."""
    if env:
        monkeypatch.setenv(env, "1")
    c = case(cams)
    rc, want = c.solve()
    assert rc == PSBA_OK
    rng = np.random.default_rng(cams)
    scale = np.abs(c.A).max()
    buf = c.buf.copy()
    n32 = c.n32
    for r0, r1 in dr._chunks(n32, n32):
        blk = buf[r0:r1, :n32]
        cols = np.arange(n32)[None, :]
        rows = np.arange(r0, r1)[:, None]
        noise = scale * rng.uniform(-1.0, 1.0, size=blk.shape)
        blk[:] = np.where(cols > rows, noise, blk)
    rc, got = c.solve(buf)
    del buf
    assert rc == PSBA_OK
    assert bits_equal(got, want), "upper triangle read: " + mismatch_report(route_of(cams)[0], got, want)


# ---- the sharded chain ---------------------------------------------------------------------------------------------

def _sharded(c, nranks, buf):
    """The two-level chain sharded over `nranks` handles on one GPU, the column exchange done by hand (as
    test_gpu_configs.py::test_sharded_dense_factorization_emulated_with_three_handles).  Returns [(status, dpa)]."""
    import psba_amd
    hs = []
    try:
        for r in range(nranks):
            h = psba_amd.Psba(0)
            h.set_rank_layout(nranks, r)
            h.upload_problem(c.prob)
            h.linearize(1.0, 1.0)
            h.schur_assemble(1.0)
            h.set_reduce_buffer(buf)
            hs.append(h)
        n32, NB, sharded = hs[0].chol_dist_shape()
        assert sharded and n32 == c.n32
        for h in hs:
            h.chol_dist_begin()
        for J in range(0, n32, NB):
            for h in hs:
                h.chol_dist_superpanel(J)
            JE = J + NB
            if JE >= n32:
                break
            for B in range(JE // 64, (min(JE + NB, n32) + 63) // 64):
                blk = hs[B % nranks].chol_dist_get_block(B)
                for r, h in enumerate(hs):
                    if r != B % nranks:
                        h.chol_dist_set_block(B, blk)
        out = []
        for h in hs:
            h.chol_dist_finish()
            dpa = h.get_dp()[:c.n].copy()
            out.append((h.backsub(1.0).status, dpa))
        return out
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("nranks", [2, 4])
def test_sharded_chain_against_the_reference(nranks):
    """300 cameras: n32 = 1824, 57 blocks of 32 columns (the last 64-column block is half a block)."""
    c = case(300)
    assert (c.n32 // 32) % 2 == 1
    for r, (status, dpa) in enumerate(_sharded(c, nranks, c.buf)):
        assert status & PSBA_NOT_SPD == 0
        c.check(PSBA_OK, dpa, what=f"sharded rank {r} of {nranks}")
    k = 2 * 256 + 100  # a bad pivot in the third super-panel
    A = c.A
    row, dkk = A[k, :].copy(), A[k, k]
    try:
        A[k, :] = 0.0
        A[:, k] = 0.0
        A[k, k] = -1.0
        res = _sharded(c, nranks, c.buf)
    finally:
        A[k, :] = row
        A[:, k] = row
        A[k, k] = dkk
    for r, (status, _) in enumerate(res):
        assert status & PSBA_NOT_SPD, f"rank {r} of {nranks}: pivot {k} = -1 not flagged"
