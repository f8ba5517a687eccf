"""The merge of a window's copies on the device (smolmc_wl_synchronise: the merge mode of wl_exchange_kernel) against
its definition, parallel.WLWindows.synchronise, bit for bit: planted arrays that take every branch, the estimator
order after exchanges, a device merge against a host merge on three kernel families, the refusals, the scheme against
the exact density of states, and the Sampler.

On the MI355X (seed 5, 2 copies, 400 rounds of 500 steps, a merge attempt after every exchange): RMS per copy 0.0559 /
0.0562, joined 0.0560 (bound 0.2046), merges per window 17, 52, 32, 29 % of the exchanges accepted."""

import numpy as np
import pytest

from smol_amd import capi, parallel
from tests import wl_sync_case as sc
from tests import wl_windows_case as wc
from tests.cases import load_case, tables_for
from tests.wl_window_oracle import enthalpies as _enthalpies

pytestmark = pytest.mark.gpu
WL_KEYS = ("entropy", "histogram", "occurrences", "mod_factor")
ENV = ("SMOLMC_FORCE_GENERAL", "SMOLMC_FORCE_UNIVERSAL", "SMOLMC_NO_WL_MULTI", "SMOLMC_NO_LEAN_MULTI", "SMOLMC_MULTI_PHI_HBM",
       "SMOLMC_MULTI_PHI_LDS", "SMOLMC_WL_RUNNING_MEAN", "SMOLMC_LAUNCH_CHUNK", "SMOLMC_FAST_EPS_SCALE", "SMOLMC_NO_ROTATE")
SALT = "rocksalt333_two_sublattices"
REFUSED = (RuntimeError, ValueError)


def _rand_occ(sc_, rng, R):
    nsp = np.array([sc_.model.prim.nspecies[b] for b in sc_.site_b])
    return (rng.random((R, sc_.num_sites)) * nsp).astype(np.int32)


def _clean(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _engine(tab, cfg):
    from smol_amd.engine import Engine

    return Engine(tab, cfg)


def _windows(R, copies, seed=5):
    """Windows of 12 bins over the 24 global bins of the 16-site case with R estimators in groups of `copies`."""
    c = wc.case()
    n = R // copies
    return parallel.WLWindows(c["lo"], c["hi"], c["bin"], n, copies=copies, seed=seed, window_bins=12, stride_bins=12 // (n - 1))


def _windowed(R, copies, seed=5, check_period=0):
    c = wc.case()
    wx = _windows(R, copies, seed)
    assert (wx.R, wx.Lw, wx.L) == (R, 12, 24)
    eng = _engine(c["tab"], sc.config(R, wx.vmin[0], wx.vmax[0], check_period=check_period))
    assert eng.L == 12 and eng.kernel_info().startswith("lean"), eng.kernel_info()
    eng.set_wl_windows(wx.vmin, wx.vmax)
    eng.set_state(wc.start_occupancies(wx, seed), np.arange(R, dtype=np.uint64) + np.uint64(100 * seed))
    return eng, wx


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_as_definition(eng, wx, copies, S, hist, m):
    """Plant the arrays, merge on the device, compare everything with the definition; returns the status."""
    eng.set_wl(entropy=S, histogram=hist, mod_factor=m)
    before = eng.get_wl()
    res = eng.wl_synchronise(copies)
    ref = wx.synchronise(S, hist, m, copies=copies, flatness=sc.FLATNESS, divisor=sc.DIVISOR)
    after = eng.get_wl()
    assert res["status"].dtype == np.int32 and np.array_equal(res["status"], ref["status"]), (res["status"], ref["status"])
    for k in ("entropy", "histogram", "mod_factor"):
        assert np.array_equal(_bits(after[k]), _bits(ref[k])), k
    assert np.array_equal(_bits(res["mod_factor"]), _bits(ref["mod_factor"][::copies]))
    assert np.array_equal(after["occurrences"], before["occurrences"])
    assert np.array_equal(_bits(after["mean_features"]), _bits(before["mean_features"]))
    return res["status"]


# ---- planted arrays, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,copies", [(6, 2), (15, 3), (15, 5)])
def test_planted_arrays_merge_as_the_definition_says(R, copies, monkeypatch):
    """R = 15: groups of 3 and 5 copies are no multiple of the workgroup's 4 waves, and the sampling kernel's last
    four-walker workgroup is partly filled."""
    _clean(monkeypatch)
    eng, wx = _windowed(R, copies)
    for third in ("single", "factors"):
        for at_threshold in (True, False):
            S, hist, m, want = sc.planted(R, copies, at_threshold=at_threshold, third=third)
            status = _same_as_definition(eng, wx, copies, S, hist, m)
            assert np.array_equal(status, want), (third, at_threshold, status, want)
    # with fetch=False the call only queues the work: the arrays afterwards are the same
    S, hist, m, want = sc.planted(R, copies)
    eng.set_wl(entropy=S, histogram=hist, mod_factor=m)
    assert eng.wl_synchronise(copies, fetch=False) is None
    ref = wx.synchronise(S, hist, m, copies=copies, flatness=sc.FLATNESS, divisor=sc.DIVISOR)
    after = eng.get_wl()
    assert all(np.array_equal(_bits(after[k]), _bits(ref[k])) for k in ("entropy", "histogram", "mod_factor"))


@pytest.mark.parametrize("R,copies", [(6, 2), (6, 3), (6, 1), (6, 6)])
def test_three_hundred_bins_without_windows(R, copies, monkeypatch):
    """A global window of 300 bins on the same model, no per-walker windows: two trips of the 256-thread bin loop, five
    of the 64-lane loops, L no multiple of 64; random arrays, seeded."""
    _clean(monkeypatch)
    c = wc.case()
    L = 300
    cfg = capi.make_config(R, capi.KERNEL_WANGLANDAU, capi.STEP_SWAP, min_enthalpy=c["lo"], max_enthalpy=c["hi"],
                           bin_size=(c["hi"] - c["lo"]) / L * (1.0 + 1e-12), check_period=0, flatness=sc.FLATNESS, mod_update=sc.DIVISOR)
    eng = _engine(c["tab"], cfg)
    assert eng.L == L
    rng = np.random.default_rng(300 + copies)
    eng.set_state(c["states"][rng.choice(len(c["states"]), R)], np.arange(R, dtype=np.uint64))
    wx = parallel.WLWindows(0.0, 1.0, 1.0, 1, copies=copies)
    seen = set()
    for trial in range(4):
        S = rng.uniform(0.1, 50.0, size=(R, L)) * (rng.random((R, L)) < 0.9)
        hist = rng.integers(900, 1100, size=(R, L))
        m = np.full(R, 2.0 ** -(trial + 1))
        G = R // copies
        if trial == 1:  # one low count in the last bin a copy of the last group visited, beyond the first 256 bins
            e = R - 1
            hist[e, np.flatnonzero(S[e] > 0)[-1]] = 700
            assert np.flatnonzero(S[e] > 0)[-1] >= 256
        if trial == 2 and copies > 1:
            m[0] = np.nextafter(m[0], 0.0)
        if trial == 3:  # the last lane-strided trip alone decides: only bin 299 is low
            S[0, L - 1], hist[0, L - 1] = 3.0, 10
        seen |= set(_same_as_definition(eng, wx, copies, S, hist, m).tolist())
        assert len(eng.wl_synchronise(copies)["status"]) == G
    assert seen == ({0, 1, 2} if copies > 1 else {0, 1}), seen


# ---- estimator order, not walker order -------------------------------------------------------------------------------
def test_the_merge_is_in_estimator_order(monkeypatch):
    """After forced exchanges (log u = -inf accepts every in-window pair) the walkers hold other estimators; the merge
    groups ESTIMATORS: the same planted arrays give the same result as on a handle whose map is the identity, and the
    walker -> estimator map is not touched."""
    _clean(monkeypatch)
    A, wx = _windowed(6, 2)
    B, _ = _windowed(6, 2)
    A.run(2000)
    for move in (0, 1, 0, 1):
        pairs = wx.pairs(move)
        A.exchange_wl(pairs, np.full(len(pairs), -np.inf))
        A.run(300)
    est = A.wl_windows()[2].copy()
    assert not np.array_equal(est, np.arange(6)), "no exchange was accepted: choose other settings"
    S, hist, m, want = sc.planted(6, 2, third="factors")
    assert np.array_equal(_same_as_definition(A, wx, 2, S, hist, m), want)
    assert np.array_equal(_same_as_definition(B, wx, 2, S, hist, m), want)
    a, b = A.get_wl(), B.get_wl()
    for k in ("entropy", "histogram", "mod_factor"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(A.wl_windows()[2], est) and np.array_equal(B.wl_windows()[2], np.arange(6))


# ---- a device merge is indistinguishable from a host merge -----------------------------------------------------------
def _snapshot(eng):
    st, wl = eng.get_state(), eng.get_wl()
    return {**{k: st[k] for k in ("occupancy", "enthalpy", "features", "n_steps", "n_accepted")}, **wl}


def _device_merge_equals_host_merge(make, copies, steps, rounds, flatness):
    """Two handles with the same states, seeds and counters; after every `steps` steps handle A merges on the device and
    handle B is given the arrays of the definition through set_wl.  Both are read with get_wl before every merge (the
    read brings the mean features to running means on both).  After the first round with a merge and 300 more steps
    everything the handles return is bitwise equal."""
    A, B = make(), make()
    wx = parallel.WLWindows(0.0, 1.0, 1.0, 1, copies=copies)
    merged = 0
    for rnd in range(rounds):
        A.run(steps)
        B.run(steps)
        a, b = A.get_wl(), B.get_wl()
        ref = wx.synchronise(b["entropy"], b["histogram"], b["mod_factor"], flatness=flatness, divisor=sc.DIVISOR)
        res = A.wl_synchronise(copies)
        assert np.array_equal(res["status"], ref["status"]), (rnd, res["status"], ref["status"])
        B.set_wl(entropy=ref["entropy"], histogram=ref["histogram"], mod_factor=ref["mod_factor"])
        merged += int((ref["status"] == 1).sum())
        if merged:
            break
    assert merged, f"no group merged in {rounds} rounds of {steps} steps: choose other settings"
    A.run(300)
    B.run(300)
    a, b = _snapshot(A), _snapshot(B)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert (a["histogram"].sum(axis=1) <= 300).any()  # (a merged copy started an empty histogram)
    print(f"first merge in round {rnd}: status {ref['status'].tolist()}, factors {a['mod_factor'].tolist()}")


def test_device_merge_equals_host_merge_windowed_lean_kernel(monkeypatch):
    _clean(monkeypatch)
    _device_merge_equals_host_merge(lambda: _windowed(6, 2)[0], 2, 500, 80, sc.FLATNESS)


def test_device_merge_equals_host_merge_mc_kernel_without_windows(monkeypatch):
    """mc_kernel (SMOLMC_FORCE_GENERAL), no windows, R = 4 walkers that are the 4 copies of the one group."""
    _clean(monkeypatch)
    monkeypatch.setenv("SMOLMC_FORCE_GENERAL", "1")
    c = wc.case()
    flat = 0.5

    def make():
        eng = _engine(c["tab"], capi.make_config(4, capi.KERNEL_WANGLANDAU, capi.STEP_SWAP, min_enthalpy=c["lo"], max_enthalpy=c["hi"],
                                                 bin_size=c["bin"], check_period=0, flatness=flat, mod_update=sc.DIVISOR))
        assert eng.kernel_info().startswith("general"), eng.kernel_info()
        eng.set_state(c["states"][np.random.default_rng(44).choice(len(c["states"]), 4)], np.arange(4, dtype=np.uint64) + np.uint64(9))
        return eng

    _device_merge_equals_host_merge(make, 4, 1000, 60, flat)


def test_device_merge_equals_host_merge_kf_family(monkeypatch):
    """The KF variant of the multi-class Wang-Landau kernel (the rocksalt case of
    test_other_wang_landau_families_refuse_and_name_themselves), no windows; a low flatness and short rounds, so that
    the copies of a group are flat together early."""
    _clean(monkeypatch)
    tab, c = tables_for(SALT, capi.FEATURES_CORRELATIONS), load_case(SALT)
    occ = _rand_occ(c["sc"], np.random.default_rng(21), 4)
    h = _enthalpies(tab, occ)
    lo, hi, flat = float(h.min() - 3), float(h.max() + 3), 0.01

    def make():
        eng = _engine(tab, capi.make_config(4, capi.KERNEL_WANGLANDAU, capi.STEP_SWAP, min_enthalpy=lo, max_enthalpy=hi, bin_size=0.05,
                                            check_period=0, flatness=flat, mod_update=sc.DIVISOR))
        assert "kf=1" in eng.kernel_info(), eng.kernel_info()
        eng.set_state(occ, np.arange(4, dtype=np.uint64) + np.uint64(300))
        return eng

    _device_merge_equals_host_merge(make, 2, 100, 40, flat)


# ---- refusals, each with its reason ----------------------------------------------------------------------------------
def test_refusals_name_their_reason(monkeypatch):
    _clean(monkeypatch)
    c = wc.case()
    met = _engine(c["tab"], capi.make_config(6, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    with pytest.raises(REFUSED, match="smolmc_wl_synchronise: the handle is not a Wang-Landau kernel"):
        met.wl_synchronise(2)
    eng, wx = _windowed(6, 2)
    for copies in (0, 4):
        with pytest.raises(REFUSED, match=rf"copies = {copies} is not a divisor of the handle's 6 estimators"):
            eng.wl_synchronise(copies)
    with pytest.raises(REFUSED, match=r"group 0 does not have one window: estimator 2 differs from estimator 0"):
        eng.wl_synchronise(3)
    before = eng.get_wl()
    assert eng.wl_synchronise(2)["status"].tolist() == [0, 0, 0]  # (nothing sampled yet: no copy has two visited bins)
    after = eng.get_wl()
    assert all(np.array_equal(_bits(before[k]), _bits(after[k])) for k in before)
    checked, _ = _windowed(6, 2, check_period=500)
    with pytest.raises(REFUSED, match=r"every 500 steps.*create the handle with check period 0"):
        checked.wl_synchronise(2)


# ---- the scheme on the device ----------------------------------------------------------------------------------------
def test_merged_copies_converge_on_the_device(monkeypatch):
    """The run of tests/test_wl_sync_host.py (seed 5, 2 copies, 400 rounds of 500 steps, a merge attempt after every
    exchange) on the device, under the same four conditions."""
    _clean(monkeypatch)
    eng, wx = _windowed(6, 2, seed=5)
    assert (wx.n_windows, wx.Ls) == (wc.N_WINDOWS, 6)
    parallel.run_wl_exchange(eng, wx, wc.ROUNDS, wc.STEPS, sync_every=1)
    wl = eng.get_wl()
    ln_g, per_copy, visited = wx.join(wl["entropy"])
    rms = [wc.rms_vs_exact(per_copy[i], per_copy[i] != 0) for i in range(wx.copies)]
    joined = wc.rms_vs_exact(ln_g, visited)
    print(f"seed 5, 2 copies, merged on the device: rms per copy {rms}, joined {joined:.4f}, merges {wx.merges.tolist()}, "
          f"factors {wx.mod_factor.tolist()}, acceptance {wx.acceptance:.3f}")
    assert (visited >= wc.case()["occupied"]).all()
    mw = wl["mod_factor"].reshape(wx.n_windows, wx.copies)
    assert np.array_equal(_bits(mw), _bits(np.repeat(mw[:, :1], wx.copies, axis=1))) and np.array_equal(_bits(mw[:, 0]), _bits(wx.mod_factor))
    assert wx.merges.min() >= 7
    assert max(rms) < wc.RMS_BOUND and joined < wc.RMS_BOUND, (rms, joined, wc.RMS_BOUND)


def test_host_route_of_the_loop_gives_the_same_arrays(monkeypatch):
    """20 rounds of 500 steps with an exchange and a merge attempt after each.  The merge route is what is compared: the
    exchanges run on the device on both handles, handle A merges through Engine.wl_synchronise, handle B through get_wl,
    WLWindows.synchronise and set_wl (sync_attempt(host=True)), and get_wl is bitwise the same afterwards.

    run_wl_exchange(host_decide=True) takes the host route for the exchanges as well; those move configurations between
    walkers whose random streams stay where they are, so that chain is another realisation of the same process (NOTES:
    the two exchange routes agree statistically, not bit for bit) and cannot be compared bitwise with the device chain.
    It runs here too, and what must hold for it does: the host merges keep the factors of a window's copies equal."""
    _clean(monkeypatch)
    A, wa = _windowed(6, 2, seed=5)
    B, wb = _windowed(6, 2, seed=5)
    parallel.run_wl_exchange(A, wa, 20, wc.STEPS, sync_every=1)
    for _ in range(20):
        B.run(wc.STEPS)
        wb.attempt(B)
        wb.sync_attempt(B, host=True)
    a, b = A.get_wl(), B.get_wl()
    for k in WL_KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    np.testing.assert_allclose(a["mean_features"], b["mean_features"], rtol=1e-10, atol=1e-9)  # (B's were read as means and summed again)
    assert np.array_equal(wa.merges, wb.merges) and np.array_equal(_bits(wa.mod_factor), _bits(wb.mod_factor))
    assert np.array_equal(A.wl_windows()[2], B.wl_windows()[2])
    print(f"20 rounds: merges {wa.merges.tolist()}, factors {wa.mod_factor.tolist()}, acceptance {wa.acceptance:.3f}")
    C, wc3 = _windowed(6, 2, seed=5)
    parallel.run_wl_exchange(C, wc3, 20, wc.STEPS, host_decide=True, sync_every=1)
    mw = C.get_wl()["mod_factor"].reshape(wc3.n_windows, wc3.copies)
    assert np.array_equal(_bits(mw), _bits(np.repeat(mw[:, :1], 2, axis=1))) and np.array_equal(_bits(mw[:, 0]), _bits(wc3.mod_factor))
    assert np.array_equal(mw[:, 0], 0.5 ** wc3.merges)


# ---- Sampler -----------------------------------------------------------------------------------------------------------
def _sampler(seed=6, **kw):
    from smol_amd import moca

    c = wc.case()
    wx = wc.windows(seed)
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    sampler = moca.Sampler.from_ensemble(ens, kernel_type="Wang-Landau", min_enthalpy=c["lo"], max_enthalpy=c["hi"], bin_size=c["bin"],
                                         check_period=wc.CHECK_PERIOD, windows=wx, seeds=list(range(60, 60 + wx.R)), synchronise=True, **kw)
    return sampler, wx


def test_sampler_run_exchange_merges_and_records(monkeypatch):
    _clean(monkeypatch)
    sampler, wx = _sampler()
    out = sampler.run_exchange(60, 500, wc.start_occupancies(wx, 6), windows=wx, sync_every=1)
    assert out is wx and wx.calls == 60 and sampler.engine.config.wl_check_period == 0
    assert all(k.check_period == wc.CHECK_PERIOD for k in sampler.mckernels)
    m = sampler.samples.get_trace_value("mod_factor", flat=False)[-1].reshape(wx.n_windows, wx.copies)
    assert np.array_equal(_bits(m), _bits(np.repeat(m[:, :1], wx.copies, axis=1)))
    meta = sampler.samples.metadata["wl_synchronise"]
    assert meta == dict(sync_every=1, merges=wx.merges.tolist(), mod_factor=wx.mod_factor.tolist())
    assert wx.merges.sum() > 0 and np.array_equal(wx.mod_factor, 0.5 ** wx.merges)
    est = sampler.samples.get_trace_value("wl_estimator", flat=False)
    assert est.shape == (60, wx.R, 1)
    print(f"sampler: merges {wx.merges.tolist()}, factors {wx.mod_factor.tolist()}")


def test_sampler_final_mod_factor_ends_the_run_early(monkeypatch):
    _clean(monkeypatch)
    sampler, wx = _sampler()
    sampler.run_exchange(400, 500, wc.start_occupancies(wx, 6), windows=wx, sync_every=1, final_mod_factor=2.0 ** -3)
    assert wx.calls < 400 and wx.converged(2.0 ** -3) and (wx.mod_factor <= 2.0 ** -3).all()
    assert len(sampler.samples.get_trace_value("wl_estimator", flat=False)) == wx.calls
    print(f"every window at or below 2^-3 after {wx.calls} attempts: factors {wx.mod_factor.tolist()}")
