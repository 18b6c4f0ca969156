"""The S-assembly schedule of the 16-parameter camera block (psba_blockprod_plan_*, host only): every product
Y_a W_b^T exactly once in the block of its camera pair, segments that tile each block's list, ascending points."""
import numpy as np
import pytest

from freekd_twin import tiny_problem
from test_freekd_twin import P54


@pytest.mark.parametrize("make", [P54, tiny_problem])
@pytest.mark.parametrize("L", [1, 4, 1000])
def test_blockprod_plan(make, L):
    from psba_amd.capi import blockprod_plan
    p = make()
    ii, jj = np.asarray(p["iidx"]), np.asarray(p["jidx"])
    plan = blockprod_plan(p["nC"], p["nP"], ii, jj, L)
    blocks, segs, prods = plan["blocks"], plan["segs"], plan["prods"]
    # every product b <= a of every point exactly once
    first = np.searchsorted(ii, ii)          # first observation of each observation's point
    want = {(a, b) for a in range(ii.size) for b in range(first[a], a + 1)}
    got = [tuple(x) for x in prods.tolist()]
    assert len(got) == len(want) and set(got) == want
    # blocks: distinct, ascending (j, k), lower triangle
    keys = blocks[:, 0].astype(np.int64) * p["nC"] + blocks[:, 1]
    assert np.all(np.diff(keys) > 0) and np.all(blocks[:, 1] <= blocks[:, 0])
    # segments tile each block's list in order, none longer than L, and cover the whole list
    assert segs[0, 1] == 0 and segs[-1, 2] == len(prods)
    assert np.array_equal(segs[1:, 1], segs[:-1, 2]) and np.all(np.diff(segs[:, 0]) >= 0)
    assert np.array_equal(np.unique(segs[:, 0]), np.arange(len(blocks)))
    length = segs[:, 2] - segs[:, 1]
    assert length.min() >= 1 and length.max() <= L
    tiles = 0
    for b in range(len(blocks)):
        mine = segs[segs[:, 0] == b]
        lo, hi = mine[0, 1], mine[-1, 2]
        assert np.all(mine[:-1, 2] - mine[:-1, 1] == L)   # only a block's last segment may be short
        a, bb = prods[lo:hi, 0], prods[lo:hi, 1]
        assert np.all(jj[a] == blocks[b, 0]) and np.all(jj[bb] == blocks[b, 1])   # in the block of its camera pair
        assert np.all(ii[a] == ii[bb]) and np.all(np.diff(ii[a]) > 0)             # ascending by point
        tiles += len(mine) if len(mine) > 1 else 0
    assert plan["tiles"] == tiles
