"""The staging of an exchange call (engine.hip: pair_exchange_stage) at its smallest sizes.  smolmc_exchange_grid and
smolmc_exchange_wl cut one buffer of 2 * half + half / 2 + 1 doubles, half = R / 2, into log u | pairs | accept flags:
on handles of 2 and of 3 walkers that is 3 doubles, every part is one pair long, and an off-by-one of a part's start
lands in its neighbour.  (Both kernel families take handles this small; at 3 walkers one walker is in no pair.)

Per handle: a refused call before anything was staged leaves the map the identity; one attempt of R // 2 pairs with
`stats` gives the accept flags and the map of `decide`; one more without `stats` on the same handle -- the buffer is
reused -- gives the map of `decide` again (the grid then takes a third, forced one with `stats`, so that a flag of 1
is read back on either handle).  The cases are those of tests/test_gpu_grid_exchange.py and
tests/test_gpu_wl_windows.py."""

import numpy as np
import pytest

from smol_amd import capi, parallel
from tests import test_gpu_grid_exchange as tg
from tests import test_gpu_wl_windows as tw

pytestmark = pytest.mark.gpu


def _refused_calls(exchange, R, noun):
    err = tg._errors() + tw.REFUSED
    with pytest.raises(err, match="%s %d of pair 0 is out of range 0 .. %d" % (noun, R, R - 1)):
        exchange([[0, R]], [0.0])
    with pytest.raises(err, match="%s 1 appears in two pairs of one call" % noun):
        exchange([[1, 1]], [0.0])
    with pytest.raises(err, match=r"log_u must be finite or -inf \(pair 0\)"):
        exchange([[0, 1]], [np.nan], np.zeros((1, 2), dtype=np.int64))


# R = 2: one temperature x two rows, the move along mu; R = 3: three temperatures x one row, both moves along T
@pytest.mark.parametrize("R,name", [(2, "fcc_prim666_triplets-corr"), (3, "rocksalt333_two_sublattices-int")])
def test_grid_exchange_on_the_smallest_handles(R, name):
    case = tg.CASES[name]()
    if R == 2:
        gx = parallel.GridExchange([case.T], case.rows[[0, -1]], seed=2)
        moves = (("mu", 0), ("mu", 0))
    else:
        gx = parallel.GridExchange(case.T * np.array([1.0, 1.1, 1.2]), case.rows[:1], seed=3)
        moves = (("T", 0), ("T", 1))
    assert gx.npoints == R and all(len(gx.pairs(m)) == R // 2 == 1 for m in moves)
    eng, _ = tg._engine(case, gx)
    assert eng.kernel_info().startswith(case.family + " ")
    eng.run(300)
    _refused_calls(eng.exchange_grid, R, "state point")
    assert np.array_equal(eng.state_points()[0], np.arange(R))
    # with stats, against the log u of the grid
    st = eng.get_state()
    res = gx.decide(st["enthalpy"], eng.species_counts(st["occupancy"]), np.arange(R), moves[0], 0)
    stats = np.zeros((1, 2), dtype=np.int64)
    eng.exchange_grid(gx.pairs(moves[0]), gx.log_u(0, 1), stats)
    print(name, R, moves[0], "exponent", res["exponent"], "log u", gx.log_u(0, 1), "stats", stats.tolist())
    assert stats[0, 0] == 1 and bool(stats[0, 1]) == bool(res["accept"][0])
    assert np.array_equal(eng.state_points()[0], res["point_of"])
    tg._check_priced(eng, gx, res["point_of"], eng.get_state())
    # without stats, on the staging of the first call; log u = -inf: the pair swaps whatever the exponent
    eng.run(50)
    st = eng.get_state()
    res2 = gx.decide(st["enthalpy"], eng.species_counts(st["occupancy"]), res["point_of"], moves[1], 1, log_u=[-np.inf])
    assert res2["accept"].all() and not np.array_equal(res2["point_of"], res["point_of"])
    eng.exchange_grid(gx.pairs(moves[1]), [-np.inf])
    assert np.array_equal(eng.state_points()[0], res2["point_of"])
    st = eng.get_state()
    tg._check_priced(eng, gx, res2["point_of"], st)
    np.testing.assert_allclose(st["enthalpy"], res2["enthalpy"], rtol=tg.RTOL, atol=tg.ATOL)
    # with stats again and log u = -inf: the flag read back is a 1 whatever the first call's was
    res3 = gx.decide(st["enthalpy"], eng.species_counts(st["occupancy"]), res2["point_of"], moves[0], 2, log_u=[-np.inf])
    eng.exchange_grid(gx.pairs(moves[0]), [-np.inf], stats)
    assert res3["accept"].all() and stats.tolist() == [[2, 1 + int(res["accept"][0])]]
    assert np.array_equal(eng.state_points()[0], res3["point_of"])
    eng.close()


def _windows(n):
    """n windows of 16 bins at a stride of 4, one copy each, laid out as tests/test_gpu_wl_windows.py's _windowed_engine
    does (centred on the median enthalpy of random half-filled occupancies; every estimator starts from the pool
    occupancy nearest to its window's middle)."""
    tab, c = tw.tables_for(tw.FCC, tw.INT), tw.load_case(tw.FCC)
    pool = (np.random.default_rng(11).random((96, c["sc"].num_sites)) < 0.5).astype(np.int32)
    h = tw._enthalpies(tab, pool)
    L = 16 + 4 * (n - 1)
    lo = float(np.median(h)) - 0.5 * L * tw.BIN
    wx = parallel.WLWindows(lo, lo + (L - 0.5) * tw.BIN, tw.BIN, n, seed=4, window_bins=16, stride_bins=4)
    assert (wx.L, wx.Lw, wx.Ls, wx.R) == (L, 16, 4, n)
    occ0 = np.zeros((n, pool.shape[1]), dtype=np.int32)
    free = np.ones(len(pool), dtype=bool)
    for e in range(n):
        k = int(np.argmin(np.where(free, np.abs(h - 0.5 * (wx.vmin[e] + wx.vmax[e])), np.inf)))
        assert wx.vmin[e] <= h[k] < wx.vmax[e]
        occ0[e], free[k] = pool[k], False
    cfg = capi.make_config(n, capi.KERNEL_WANGLANDAU, min_enthalpy=wx.vmin[0], max_enthalpy=wx.vmax[0],
                           step_type=capi.STEP_SWAP, bin_size=tw.BIN, check_period=64)
    return tab, cfg, wx, occ0


@pytest.mark.parametrize("R", [2, 3])
def test_wl_exchange_on_the_smallest_handles(R, monkeypatch):
    tw._clean(monkeypatch)
    tab, cfg, wx, occ0 = _windows(R)
    moves = (0, 0) if R == 2 else (0, 1)
    assert all(len(wx.pairs(m)) == R // 2 == 1 for m in moves)
    eng = tw._engine(tab, cfg)
    eng.set_wl_windows(wx.vmin, wx.vmax)
    eng.set_state(occ0, np.arange(R, dtype=np.uint64) + np.uint64(7))
    _refused_calls(eng.exchange_wl, R, "estimator")
    assert np.array_equal(eng.wl_windows()[2], np.arange(R))
    # with stats, at step 0: every entropy is zero, so the pair swaps if and only if both enthalpies lie in both windows
    before = tw._snapshot(eng)
    res = wx.decide(before["enthalpy"], before["entropy"], np.arange(R), moves[0], 0)
    stats = np.zeros((1, 2), dtype=np.int64)
    eng.exchange_wl(wx.pairs(moves[0]), wx.log_u(0, 1), stats)
    assert stats[0, 0] == 1 and bool(stats[0, 1]) == bool(res["accept"][0]) == bool(res["in_window"][0])
    assert res["accept"].all(), "the start occupancies of a neighbouring pair lie in both windows by the layout"
    assert np.array_equal(eng.wl_windows()[2], res["estimator_of"]) and not np.array_equal(res["estimator_of"], np.arange(R))
    tw._assert_identical(before, tw._snapshot(eng))
    # without stats, on the staging of the first call, after the walkers moved
    eng.run(600)
    before = tw._snapshot(eng)
    res2 = wx.decide(before["enthalpy"], before["entropy"], res["estimator_of"], moves[1], 1)
    eng.exchange_wl(wx.pairs(moves[1]), wx.log_u(1, 1))
    print(R, "in window", res2["in_window"], "exponent", res2["exponent"], "log u", wx.log_u(1, 1), "accept", res2["accept"])
    vmin, vmax, est = eng.wl_windows()
    assert np.array_equal(est, res2["estimator_of"])
    assert np.array_equal(vmin, wx.vmin[est]) and np.array_equal(vmax, wx.vmax[est])
    tw._assert_identical(before, tw._snapshot(eng))
    eng.close()
