"""Replica-exchange Wang-Landau on the device: per-walker energy windows in one handle (smolmc_set_wl_windows; the
window variants of mc_wl_kernel and of mc_lean_multi_kernel's Wang-Landau kernel) and the exchange between them
(smolmc_exchange_wl, wl_exchange.hip).  A walker with its own window is compared bit for bit with an unmodified
one-walker oracle that was given the identical (min, max, bin); the exchange decisions with parallel.WLWindows.decide;
the joined density of states with exact enumeration."""

import numpy as np
import pytest

from smol_amd import capi, parallel
from tests import wl_windows_case as wc
from tests.cases import load_case, tables_for
from tests.wl_window_oracle import enthalpies as _enthalpies, one_walker_oracle as _oracle, same as _same, top as _top

pytestmark = pytest.mark.gpu
INT = capi.FEATURES_INTERACTIONS
ENV = ("SMOLMC_FORCE_GENERAL", "SMOLMC_FORCE_UNIVERSAL", "SMOLMC_NO_WL_MULTI", "SMOLMC_NO_LEAN_MULTI", "SMOLMC_MULTI_PHI_HBM",
       "SMOLMC_MULTI_PHI_LDS", "SMOLMC_WL_RUNNING_MEAN", "SMOLMC_LAUNCH_CHUNK", "SMOLMC_FAST_EPS_SCALE", "SMOLMC_NO_ROTATE")
FCC, SALT = "fcc_prim666_triplets", "rocksalt333_two_sublattices"
BIN = 0.11
REFUSED = (RuntimeError, ValueError)  # (Engine._chk raises ValueError for messages about ranges and enthalpies)


def _clean(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _engine(tab, cfg):
    from smol_amd.engine import Engine

    return Engine(tab, cfg)


def _rand_occ(sc, rng, R):
    nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    return (rng.random((R, sc.num_sites)) * nsp).astype(np.int32)


# ---- 5. per-walker windows against the oracle, bit for bit -----------------------------------------------------------
@pytest.mark.parametrize("scale", ["1", "3000"])
def test_per_walker_windows_match_one_oracle_per_window(scale, monkeypatch):
    """Six walkers (a partly filled four-walker workgroup), each with its own narrow window of 12 bins placed a
    non-integer number of bins below its start enthalpy: every walker hits both ends of its window.  SMOLMC_FAST_EPS_SCALE
    interleaves the float32 pre-test and the exact path at both rates."""
    _clean(monkeypatch)
    monkeypatch.setenv("SMOLMC_FAST_EPS_SCALE", scale)
    tab, c = tables_for(FCC, INT), load_case(FCC)
    R, L = 6, 12
    occ0 = (np.random.default_rng(77).random((R, c["sc"].num_sites)) < 0.5).astype(np.int32)
    h0 = _enthalpies(tab, occ0)
    vmin = h0 - np.array([2.3, 3.7, 5.1, 6.4, 7.9, 8.6]) * BIN
    vmax = np.array([_top(v, L, BIN) for v in vmin])
    kw = dict(step_type=capi.STEP_SWAP, bin_size=BIN, check_period=64)
    eng = _engine(tab, capi.make_config(R, capi.KERNEL_WANGLANDAU, min_enthalpy=vmin[2], max_enthalpy=vmax[2], **kw))
    assert eng.L == L
    eng.set_wl_windows(vmin, vmax)
    info = eng.kernel_info()
    assert info.startswith("lean") and "wl_windows=1" in info, info
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(4242)
    eng.set_state(occ0, seeds)
    oras = [_oracle(tab, occ0[r], seeds[r], vmin[r], vmax[r], **kw) for r in range(R)]
    w = eng.wl_windows()
    assert np.array_equal(w[0], vmin) and np.array_equal(w[1], vmax) and np.array_equal(w[2], np.arange(R))
    for chunk in (1, 17, 700, 2500):
        eng.run(chunk)
        a, x = eng.get_state(), eng.get_wl()
        for r in range(R):
            oras[r].run(chunk)
            _same(a, x, r, r, oras[r])
    assert (x["occurrences"] > 0).sum(axis=1).min() > 3 and (x["mod_factor"] < 1.0).all()  # (flatness checks fired)
    eng.set_wl_windows(None, None)
    assert "wl_windows" not in eng.kernel_info()


@pytest.mark.parametrize("update_period", [1, 3])
def test_per_walker_windows_multi_class_kernel(update_period, monkeypatch):
    """The same on mc_lean_multi_kernel's Wang-Landau kernel (two active sublattices + Ewald field in LDS; per-bin sums at
    update_period 1, running means at 3), with the settings of tests/test_gpu_wl_multi.py and windows of 100 bins."""
    _clean(monkeypatch)
    monkeypatch.setenv("SMOLMC_MULTI_PHI_LDS", "1")
    tab, c = tables_for(SALT, INT), load_case(SALT)
    R, L, b = 6, 100, 0.0517
    occ0 = _rand_occ(c["sc"], np.random.default_rng(21), R)
    h0 = _enthalpies(tab, occ0)
    vmin = h0 - np.array([21.3, 33.7, 45.1, 52.4, 61.9, 68.6]) * b
    vmax = np.array([_top(v, L, b) for v in vmin])
    kw = dict(step_type=capi.STEP_SWAP, bin_size=b, check_period=50, update_period=update_period, flatness=0.2)
    eng = _engine(tab, capi.make_config(R, capi.KERNEL_WANGLANDAU, min_enthalpy=vmin[0], max_enthalpy=vmax[0], **kw))
    eng.set_wl_windows(vmin, vmax)
    info = eng.kernel_info()
    assert info.startswith("lean-multi") and "wl=multi" in info and "wl_windows=1" in info, info
    assert ("wl=multi-mean" in info) == (update_period != 1), info
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(300)
    eng.set_state(occ0, seeds)
    oras = [_oracle(tab, occ0[r], seeds[r], vmin[r], vmax[r], **kw) for r in range(R)]
    for chunk in (1, 2, 13, 64, 400, 1500):
        eng.run(chunk)
        a, x = eng.get_state(), eng.get_wl()
        for r in range(R):
            oras[r].run(chunk)
            _same(a, x, r, r, oras[r])
    assert (x["occurrences"] > 0).sum(axis=1).min() > 3 and (x["mod_factor"] < 1.0).all()


# ---- 6. exchange at step 0 -------------------------------------------------------------------------------------------
def _close_pair(tab, sc, L):
    """Two random 50 % occupancies (of a pool of 64) whose enthalpies are closest, and two different windows of L bins
    that both contain both."""
    pool = (np.random.default_rng(5).random((64, sc.num_sites)) < 0.5).astype(np.int32)
    h = _enthalpies(tab, pool)
    order = np.argsort(h)
    k = int(np.argmin(np.diff(h[order])))
    i, j = order[k], order[k + 1]
    assert h[j] - h[i] < BIN
    vmin = np.array([h[i] - 3.3 * BIN, h[i] - 6.6 * BIN])
    vmax = np.array([_top(v, L, BIN) for v in vmin])
    assert ((h[[i, j]][:, None] >= vmin) & (h[[i, j]][:, None] < vmax)).all()
    return pool[[i, j]], vmin, vmax


def test_exchange_at_step_zero_continues_as_the_oracle_in_the_other_window(monkeypatch):
    """Right after set_state all entropies are zero, so an in-window pair is accepted at log u = -inf: from then on
    walker a must be the chain of an oracle that has a's occupancy and seed and window t from step 0, and b likewise.
    This pins the estimator indirection and the swapped window records in the sampling kernel."""
    _clean(monkeypatch)
    tab, c = tables_for(FCC, INT), load_case(FCC)
    L = 12
    pair, wmin, wmax = _close_pair(tab, c["sc"], L)
    # (walkers 0 and 1 are the pair; 2 and 3 hold copies of the windows and do not exchange: they must not notice)
    occ0 = pair[[0, 1, 0, 1]]
    vmin, vmax = wmin[[0, 1, 0, 1]], wmax[[0, 1, 0, 1]]
    kw = dict(step_type=capi.STEP_SWAP, bin_size=BIN, check_period=64)
    eng = _engine(tab, capi.make_config(4, capi.KERNEL_WANGLANDAU, min_enthalpy=vmin[0], max_enthalpy=vmax[0], **kw))
    eng.set_wl_windows(vmin, vmax)
    seeds = np.arange(4, dtype=np.uint64) + np.uint64(99)
    eng.set_state(occ0, seeds)
    stats = np.zeros((1, 2), dtype=np.int64)
    eng.exchange_wl([[0, 1]], [-np.inf], stats)
    assert stats.tolist() == [[1, 1]]
    w = eng.wl_windows()
    assert w[2].tolist() == [1, 0, 2, 3] and np.array_equal(w[0], vmin[[1, 0, 2, 3]]) and np.array_equal(w[1], vmax[[1, 0, 2, 3]])
    holds = [1, 0, 2, 3]
    oras = [_oracle(tab, occ0[r], seeds[r], vmin[holds[r]], vmax[holds[r]], **kw) for r in range(4)]
    for chunk in (1, 499, 2500):
        eng.run(chunk)
        a, x = eng.get_state(), eng.get_wl()
        for r in range(4):
            oras[r].run(chunk)
            _same(a, x, r, holds[r], oras[r])
    assert (x["occurrences"] > 0).sum(axis=1).min() > 3


# ---- 7 / 8. decisions against the mirror; continuation -----------------------------------------------------------------
def _windowed_engine(seed=3):
    """fcc 6x6x6, 4 windows of 16 bins at a stride of 4 (75 % overlap) x 2 copies around the enthalpies of random 50 %
    occupancies; every estimator starts from a pool occupancy inside its window (nearest to the window's middle)."""
    tab, c = tables_for(FCC, INT), load_case(FCC)
    pool = (np.random.default_rng(11).random((96, c["sc"].num_sites)) < 0.5).astype(np.int32)
    h = _enthalpies(tab, pool)
    lo = float(np.median(h)) - 14 * BIN
    wx = parallel.WLWindows(lo, lo + 27.5 * BIN, BIN, 4, copies=2, seed=seed, window_bins=16, stride_bins=4)
    assert (wx.L, wx.Lw, wx.Ls, wx.R) == (28, 16, 4, 8)
    occ0 = np.zeros((wx.R, pool.shape[1]), dtype=np.int32)
    free = np.ones(len(pool), dtype=bool)
    for e in range(wx.R):
        d = np.where(free, np.abs(h - 0.5 * (wx.vmin[e] + wx.vmax[e])), np.inf)
        k = int(np.argmin(d))
        assert wx.vmin[e] <= h[k] < wx.vmax[e]
        occ0[e], free[k] = pool[k], False
    kw = dict(step_type=capi.STEP_SWAP, bin_size=BIN, check_period=64)
    cfg = capi.make_config(wx.R, capi.KERNEL_WANGLANDAU, min_enthalpy=wx.vmin[0], max_enthalpy=wx.vmax[0], **kw)
    return tab, cfg, wx, occ0


def _snapshot(eng):
    st, wl = eng.get_state(), eng.get_wl()
    return {**{k: st[k] for k in ("occupancy", "enthalpy", "features", "n_steps", "n_accepted")}, **wl}


def _assert_identical(a, b, keys=None):
    for k in keys or a:
        assert np.array_equal(a[k], b[k]), k


def test_exchange_decisions_equal_the_numpy_mirror(monkeypatch):
    """2000 steps, then an even and an odd move with the Philox log u of WLWindows: accept flags and the walker ->
    estimator map equal WLWindows.decide exactly; get_wl (estimator order), occupancies, enthalpies and counters are
    untouched by the call; stats counts attempts and accepts; a pair outside the windows is rejected at -inf."""
    _clean(monkeypatch)
    tab, cfg, wx, occ0 = _windowed_engine()
    eng = _engine(tab, cfg)
    eng.set_wl_windows(wx.vmin, wx.vmax)
    eng.set_state(occ0, np.arange(wx.R, dtype=np.uint64) + np.uint64(7))
    eng.run(2000)
    est = np.arange(wx.R)
    n_acc = n_rej = 0
    for attempt, move in enumerate((0, 1, 0, 1)):
        before = _snapshot(eng)
        pairs = wx.pairs(move)
        res = wx.decide(before["enthalpy"], before["entropy"], est, move, attempt)
        stats = np.zeros((len(pairs), 2), dtype=np.int64)
        stats[:, 0] = 5
        eng.exchange_wl(pairs, wx.log_u(attempt, len(pairs)), stats)
        assert np.array_equal(stats[:, 0], np.full(len(pairs), 6)) and np.array_equal(stats[:, 1], res["accept"].astype(np.int64))
        vmin, vmax, est_dev = eng.wl_windows()
        assert np.array_equal(est_dev, res["estimator_of"])
        assert np.array_equal(vmin, wx.vmin[est_dev]) and np.array_equal(vmax, wx.vmax[est_dev])
        _assert_identical(before, _snapshot(eng))
        est = res["estimator_of"]
        n_acc, n_rej = n_acc + int(res["accept"].sum()), n_rej + int((~res["accept"]).sum())
        eng.run(300)
    print(f"accepted {n_acc}, rejected {n_rej} of {n_acc + n_rej} attempts; estimator_of {est.tolist()}")
    assert n_acc > 0  # (the exchanges did happen: the map is no longer the identity)
    # windows 0 and 3 share bins 12 .. 15 only: a pair of their estimators with an enthalpy outside is rejected at -inf
    st, S = eng.get_state(), eng.get_wl()["entropy"]
    far = np.array([[0, 6], [1, 7]], dtype=np.int32)
    res = wx.decide(st["enthalpy"], S, est, 0, 0, log_u=np.full(2, -np.inf), record=False, pairs=far)
    stats = np.zeros((2, 2), dtype=np.int64)
    eng.exchange_wl(far, np.full(2, -np.inf), stats)
    assert np.array_equal(stats[:, 1], res["accept"].astype(np.int64)) and np.array_equal(res["accept"], res["in_window"])
    assert not res["in_window"].all(), "both far pairs happen to lie inside both windows: choose other settings"
    assert np.array_equal(eng.wl_windows()[2], res["estimator_of"])


def test_continuation_with_physically_permuted_windows(monkeypatch):
    """Engine A runs, exchanges and runs on.  Engine B is fresh: it is given A's state after the exchange with the
    windows physically permuted to where the walkers hold them (set_wl_windows makes that the identity map), the rows
    of the Wang-Landau arrays permuted the same way.  Both must agree bit for bit in every array: the estimator
    indirection of A is the physical layout of B, which test_per_walker_windows_match_one_oracle_per_window anchors."""
    _clean(monkeypatch)
    tab, cfg, wx, occ0 = _windowed_engine()
    seeds = np.arange(wx.R, dtype=np.uint64) + np.uint64(7)
    A = _engine(tab, cfg)
    A.set_wl_windows(wx.vmin, wx.vmax)
    A.set_state(occ0, seeds)
    A.run(1500)
    for attempt, move in enumerate((0, 1)):
        pairs = wx.pairs(move)
        A.exchange_wl(pairs, wx.log_u(attempt, len(pairs)))
    vmin, vmax, est = A.wl_windows()
    assert not np.array_equal(est, np.arange(wx.R)), "no exchange was accepted: choose other settings"
    mid = _snapshot(A)
    B = _engine(tab, cfg)
    B.set_wl_windows(vmin, vmax)  # walker r of B holds the window walker r of A holds: B's estimator r is A's estimator est[r]
    B.set_state(mid["occupancy"], seeds)
    B.set_counters(mid["n_steps"], mid["n_accepted"])
    B.set_wl(entropy=mid["entropy"][est], histogram=mid["histogram"][est], occurrences=mid["occurrences"][est],
             mean_features=mid["mean_features"][est], mod_factor=mid["mod_factor"][est])
    A.run(1500)
    B.run(1500)
    a, b = _snapshot(A), _snapshot(B)
    _assert_identical(a, b, ("occupancy", "n_steps", "n_accepted"))
    np.testing.assert_allclose(a["enthalpy"], b["enthalpy"], rtol=1e-12, atol=1e-10)  # (B's start enthalpy is evaluated afresh)
    for k in ("entropy", "histogram", "occurrences", "mod_factor"):
        assert np.array_equal(a[k][est], b[k]), k
    np.testing.assert_allclose(a["mean_features"][est], b["mean_features"], rtol=1e-10, atol=1e-9)
    # a continuation of A keeps the map, a reset returns it to the identity
    A.set_state(a["occupancy"], seeds, reset_aux=False)
    assert np.array_equal(A.wl_windows()[2], est)
    start = np.empty_like(occ0)
    start[:] = occ0  # (estimator e's start lies in window e: after the reset walker e holds it again)
    A.set_state(start, seeds)
    assert np.array_equal(A.wl_windows()[2], np.arange(wx.R)) and np.array_equal(A.wl_windows()[0], wx.vmin)


# ---- 9. statistics on the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [5])
def test_device_replica_exchange_converges_to_the_exact_density_of_states(seed, monkeypatch):
    """The 16-site model, windows and bound of tests/test_wl_windows_host.py through run_wl_exchange with the decisions
    taken on the device."""
    _clean(monkeypatch)
    c = wc.case()
    wx = wc.windows(seed)
    eng = _engine(c["tab"], wc.config(wx.R, wx.vmin[0], wx.vmax[0]))
    info = eng.kernel_info()
    assert info.startswith("lean"), info  # (else: the condition that kept the lean kernel off is in the message)
    eng.set_wl_windows(wx.vmin, wx.vmax)
    eng.set_state(wc.start_occupancies(wx, seed), np.arange(wx.R, dtype=np.uint64) + np.uint64(100 * seed))
    hist = []
    parallel.run_wl_exchange(eng, wx, wc.ROUNDS, wc.STEPS, history=hist)
    assert len(hist) == wc.ROUNDS and all(sorted(h.tolist()) == list(range(wx.R)) for h in hist)
    ln_g, per_copy, visited = wx.join(eng.get_wl()["entropy"])
    rms = [wc.rms_vs_exact(per_copy[i], per_copy[i] != 0) for i in range(wx.copies)]
    print(f"seed {seed}: {info}; acceptance {wx.acceptance:.3f}, rms per copy {rms}, joined {wc.rms_vs_exact(ln_g, visited):.4f}")
    assert (visited >= c["occupied"]).all() and wx.acceptance > 0.05
    assert max(rms) < wc.RMS_BOUND and wc.rms_vs_exact(ln_g, visited) < wc.RMS_BOUND, (rms, wc.RMS_BOUND)


# ---- 10. refusals, each with its reason --------------------------------------------------------------------------------
def test_refusals_name_their_reason(monkeypatch):
    _clean(monkeypatch)
    tab, cfg, wx, occ0 = _windowed_engine()
    seeds = np.arange(wx.R, dtype=np.uint64)
    met = _engine(tab, capi.make_config(wx.R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    with pytest.raises(REFUSED, match="not a Wang-Landau kernel"):
        met.set_wl_windows(wx.vmin, wx.vmax)
    with pytest.raises(REFUSED, match="not a Wang-Landau kernel"):
        met.exchange_wl([[0, 1]], [0.0])
    eng = _engine(tab, cfg)
    with pytest.raises(REFUSED, match="no per-walker windows are set"):
        eng.exchange_wl([[0, 2]], [0.0])
    bad = wx.vmax.copy()
    bad[3] += 1.5 * BIN
    with pytest.raises(REFUSED, match=r"window of walker 3 has 18 bins, the handle has L = 16"):
        eng.set_wl_windows(wx.vmin, bad)
    assert "wl_windows" not in eng.kernel_info()
    eng.set_wl_windows(wx.vmin, wx.vmax)
    outside = occ0[::-1].copy()  # estimator 0 (lowest window) gets the start of estimator 7 (highest window)
    h = _enthalpies(tab, outside)
    assert not (wx.vmin[0] <= h[0] < wx.vmax[0])
    with pytest.raises(REFUSED, match=r"walker 0 is outside the Wang-Landau window .* the walker holds"):
        eng.set_state(outside, seeds)
    eng.set_state(occ0, seeds)
    eng.run(10)
    with pytest.raises(REFUSED, match="smolmc_replay while per-walker windows are set"):
        eng.replay(np.full((wx.R, 1, 4), -1, dtype=np.int32), np.full((wx.R, 1), 0.5))
    with pytest.raises(REFUSED, match="SMOLMC_SAMPLE_WL while per-walker windows are set"):
        eng.run_sampled(2, 5, occupancy=False, wl=True)
    with pytest.raises(REFUSED, match="estimator 2 appears in two pairs"):
        eng.exchange_wl([[0, 2], [2, 4]], [0.0, 0.0])
    with pytest.raises(REFUSED, match="out of range"):
        eng.exchange_wl([[0, wx.R]], [0.0])
    with pytest.raises(REFUSED, match="finite or -inf"):
        eng.exchange_wl([[0, 2]], [np.inf])
    monkeypatch.setenv("SMOLMC_FORCE_GENERAL", "1")
    gen = _engine(tab, cfg)
    assert gen.kernel_info().startswith("general")
    with pytest.raises(REFUSED, match="mc_kernel"):
        gen.set_wl_windows(wx.vmin, wx.vmax)


def test_other_wang_landau_families_refuse_and_name_themselves(monkeypatch):
    """The KF variant (several correlation functions per orbit) runs without windows; it says so."""
    _clean(monkeypatch)
    tab, c = tables_for(SALT, capi.FEATURES_CORRELATIONS), load_case(SALT)
    occ = _rand_occ(c["sc"], np.random.default_rng(21), 4)
    h = _enthalpies(tab, occ)
    lo, hi = float(h.min() - 3), float(h.max() + 3)
    eng = _engine(tab, capi.make_config(4, capi.KERNEL_WANGLANDAU, capi.STEP_SWAP, min_enthalpy=lo, max_enthalpy=hi, bin_size=0.05,
                                        check_period=50))
    assert "kf=1" in eng.kernel_info()
    with pytest.raises(REFUSED, match="KF variant"):
        eng.set_wl_windows(np.full(4, lo), np.full(4, hi))


# ---- 11. Sampler level -------------------------------------------------------------------------------------------------
def test_sampler_run_exchange_traces_the_estimators(monkeypatch):
    from smol_amd import moca

    _clean(monkeypatch)
    c = wc.case()
    wx = wc.windows(6)
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    sampler = moca.Sampler.from_ensemble(ens, kernel_type="Wang-Landau", min_enthalpy=c["lo"], max_enthalpy=c["hi"], bin_size=c["bin"],
                                         check_period=wc.CHECK_PERIOD, windows=wx, seeds=list(range(60, 60 + wx.R)))
    out = sampler.run_exchange(30, 200, wc.start_occupancies(wx, 6), windows=wx)
    assert out is wx and wx.calls == 30 and "wl_windows=1" in sampler.engine.kernel_info()
    est = sampler.samples.get_trace_value("wl_estimator", flat=False)
    assert est.shape == (30, wx.R, 1) and est.dtype == np.int32
    assert all(sorted(row[:, 0].tolist()) == list(range(wx.R)) for row in est)  # a permutation at every sample
    assert np.array_equal(est[0, :, 0], np.arange(wx.R)) and wx.acceptance > 0 and not np.array_equal(est[-1, :, 0], np.arange(wx.R))
    # occupancies stay with the walkers: walker w's enthalpy lies in the window of the estimator it held
    H = sampler.samples.get_enthalpies(flat=False).reshape(30, wx.R)
    assert ((H >= wx.vmin[est[:, :, 0]]) & (H < wx.vmax[est[:, :, 0]])).all()
    levels, ln_g, visited = sampler.wl_joined_entropy()
    ref = wx.join(sampler.engine.get_wl()["entropy"])
    assert np.array_equal(levels, wx.levels()) and np.array_equal(ln_g, ref[0]) and np.array_equal(visited, ref[2])
    assert np.array_equal(sampler.samples.get_trace_value("entropy", flat=False)[-1], sampler.engine.get_wl()["entropy"])
    with pytest.raises(ValueError, match="was built with"):
        sampler.run_exchange(1, 10, windows=wc.windows(6))
