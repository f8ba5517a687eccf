"""Replica-exchange Wang-Landau, host side (parallel.WLWindows): the window geometry under the engine's ceil rule, the
pair lists, `decide` -- the NumPy definition the device kernel is tested against (tests/test_gpu_wl_windows.py) --
`join`, and the whole scheme on the CPU oracle against exact enumeration."""

import numpy as np
import pytest

from smol_amd import parallel
from tests import wl_windows_case as wc


# ---- geometry and pair lists ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("vmin,bin_size,L,n,overlap,copies", [
    (-0.1633973721973, 0.2723964996846, 24, 3, 0.5, 2),
    (-0.1633973721973, 0.2723964996846, 512, 16, 0.75, 4),
    (-7.3, 0.1, 60, 5, 0.5, 1),
    (1e3 + 0.1, 0.11, 37, 4, 0.3, 3),
    (-31.337, 0.0517, 200, 2, 0.9, 2),
    (0.0, 1.0 / 3.0, 12, 1, 0.5, 2),
])
def test_geometry_and_pairs(vmin, bin_size, L, n, overlap, copies):
    wx = parallel.WLWindows(vmin, vmin + (L - 0.5) * bin_size, bin_size, n, overlap=overlap, copies=copies)
    assert wx.L == L and (n - 1) * wx.Ls + wx.Lw == L and wx.R == n * copies
    assert wx.vmin.shape == wx.vmax.shape == (wx.R,)
    for e in range(wx.R):  # the engine's rule, window by window
        assert int(np.ceil((wx.vmax[e] - wx.vmin[e]) / bin_size)) == wx.Lw, e
        k = e // copies
        assert wx.window_of[e] == k and wx.copy_of[e] == e % copies
        assert wx.vmin[e] == vmin + k * wx.Ls * bin_size
        assert abs(wx.vmax[e] - (vmin + (k * wx.Ls + wx.Lw) * bin_size)) <= 64 * np.spacing(abs(wx.vmax[e]))
    seen = set()
    for move in wx.MOVES:
        pairs = wx.pairs(move)
        assert pairs.dtype == np.int32 and pairs.shape == (len(pairs), 2)
        assert len(np.unique(pairs)) == pairs.size  # disjoint
        for s, t in pairs:
            assert t - s == copies and (s // copies) % 2 == move  # neighbouring windows, copy i with copy i
            seen.add((int(s), int(t)))
    assert seen == {(k * copies + i, (k + 1) * copies + i) for k in range(n - 1) for i in range(copies)}


def test_log_u_is_a_function_of_seed_and_attempt():
    a, b = parallel.WLWindows(0, 24, 1, 3, seed=5), parallel.WLWindows(0, 24, 1, 3, seed=5)
    assert np.array_equal(a.log_u(3, 4), b.log_u(3, 4)) and not np.array_equal(a.log_u(3, 4), a.log_u(4, 4))
    assert np.array_equal(a.log_u(3, 4), np.log(parallel._philox_uniforms(5, 3, 4)))
    assert len(a.log_u(0, 0)) == 0


# ---- decide ---------------------------------------------------------------------------------------------------------
def _wx():
    return parallel.WLWindows(-0.1633973721973, -0.1633973721973 + 23.7 * 0.2723964996846, 0.2723964996846, 3, copies=2, seed=3)


def test_decide_rejects_out_of_window_even_at_minus_infinity():
    wx = _wx()
    rng = np.random.default_rng(0)
    S = rng.random((wx.R, wx.Lw)) * 5
    mid = 0.5 * (wx.vmin + wx.vmax)
    E = mid.copy()
    E[0] = wx.vmin[0] + 1.5 * wx.bin_size  # walker 0 (estimator 0, window 0) below window 1
    E[1] = wx.vmin[3] + 0.3 * wx.bin_size  # walker 1 (estimator 1, window 0) inside the overlap with window 1
    E[3] = wx.vmax[1] - 0.3 * wx.bin_size  # walker 3 (estimator 3, window 1) inside the overlap with window 0
    E[2] = wx.vmax[0] - 0.3 * wx.bin_size  # walker 2 (estimator 2, window 1) inside window 0: its partner 0 is not in window 1
    res = wx.decide(E, S, np.arange(wx.R), 0, 0, log_u=np.full(2, -np.inf))
    assert res["pairs"].tolist() == [[0, 2], [1, 3]]
    assert res["in_window"].tolist() == [False, True] and res["accept"].tolist() == [False, True]
    assert res["estimator_of"].tolist() == [0, 3, 2, 1, 4, 5]
    assert wx.attempted[0].tolist() == [1, 1] and wx.accepted[0].tolist() == [0, 1]
    E[0], E[2] = E[2], wx.vmin[0] - 1.0  # the other enthalpy outside
    res = wx.decide(E, S, np.arange(wx.R), 0, 0, log_u=np.full(2, -np.inf))
    assert res["accept"].tolist() == [False, True]


def test_decide_accepts_at_zero_entropies_and_is_symmetric_in_the_roles():
    wx = _wx()
    mid = 0.5 * (wx.vmin + wx.vmax)
    for move in (0, 1):
        pairs = wx.pairs(move)
        E = mid.copy()
        for s, t in pairs:  # both walkers of a pair in the middle of the overlap of their windows
            E[[s, t]] = wx.vmin[t] + 0.5 * (wx.Lw - wx.Ls) * wx.bin_size
        res = wx.decide(E, np.zeros((wx.R, wx.Lw)), np.arange(wx.R), move, 7, log_u=np.full(len(pairs), -1e-300))
        assert res["in_window"].all() and (res["exponent"] == 0).all() and res["accept"].all()
    # (s, t) -> (t, s): the same exponent.  The walkers are relabelled so that the estimators change roles.
    rng = np.random.default_rng(4)
    S = rng.random((wx.R, wx.Lw)) * 9 + 0.1
    E4 = np.array([wx.vmin[2] + 1.7 * wx.bin_size, 0, wx.vmax[0] - 2.2 * wx.bin_size, 0, 0, 0])
    E4[[1, 3, 4, 5]] = 0.5 * (wx.vmin + wx.vmax)[[1, 3, 4, 5]]
    fwd = wx.decide(E4, S, np.arange(wx.R), 0, 0, log_u=np.zeros(2), record=False)
    est = np.array([2, 1, 0, 3, 4, 5])  # walker 0 holds estimator 2 and walker 2 estimator 0, each with its enthalpy
    rev = wx.decide(E4[est], S, est, 0, 0, log_u=np.zeros(2), record=False)
    assert fwd["in_window"][0] and rev["in_window"][0]
    ia = wx.bins  # the exponent with the roles of s and t written the other way round
    s, t, Ea, Eb = 0, 2, E4[0], E4[2]
    swapped = ((S[t, ia(Eb, wx.vmin[t])] - S[t, ia(Ea, wx.vmin[t])]) + S[s, ia(Ea, wx.vmin[s])]) - S[s, ia(Eb, wx.vmin[s])]
    assert fwd["exponent"][0] != 0 and np.isclose(fwd["exponent"][0], swapped, rtol=0, atol=1e-13)
    assert rev["exponent"][0] == fwd["exponent"][0]  # (which walker holds which estimator does not matter)


# ---- join -----------------------------------------------------------------------------------------------------------
def test_join_recovers_a_known_ln_g_and_ignores_unvisited_bins():
    wx = parallel.WLWindows(-3.0, 21.0, 1.0, 4, overlap=0.5, copies=3)
    assert (wx.L, wx.Lw, wx.Ls) == (24, 9, 5) or (wx.n_windows - 1) * wx.Ls + wx.Lw == 24
    x = np.arange(wx.L)
    truth = 40.0 - 0.25 * (x - 11.3) ** 2 + np.sin(x) + 50.0
    rng = np.random.default_rng(9)
    S = np.zeros((wx.R, wx.Lw))
    for e in range(wx.R):
        k = wx.window_of[e]
        S[e] = truth[k * wx.Ls:k * wx.Ls + wx.Lw] - 20.0 + rng.uniform(0.0, 15.0)  # a different constant everywhere, S > 0
    assert (S > 0).all()
    ln_g, per_copy, visited = wx.join(S)
    assert visited.all() and per_copy.shape == (wx.copies, wx.L)
    d = ln_g - truth
    assert np.abs(d - d.mean()).max() < 1e-12
    for i in range(wx.copies):
        di = per_copy[i] - truth
        assert np.abs(di - di.mean()).max() < 1e-12
    # an unvisited bin (S = 0) inside an overlap: ignored, not averaged in; unvisited in every window: not visited
    S2 = S.copy()
    hole = wx.Ls + 1                                   # global bin inside the overlap of windows 0 and 1
    S2[wx.window_of == 1, hole - wx.Ls] = 0.0          # ... not visited by window 1 (any copy)
    S2[wx.window_of == 0, 0] = 0.0                     # global bin 0 belongs to window 0 alone: nobody visited it
    ln_g2, _, visited2 = wx.join(S2)
    assert not visited2[0] and visited2[1:].all() and ln_g2[0] == 0.0
    d2 = (ln_g2 - truth)[1:]
    assert np.abs(d2 - d2.mean()).max() < 1e-12


def test_config15_is_config4_cut_into_windows():
    from smol_amd import workloads

    assert workloads.BUILDERS[15] is workloads.config15
    w4, w15 = workloads.config4(count=64, dim=4, h0=12.5), workloads.config15(count=64, dim=4, h0=12.5)
    wx = w15.extras["wl_windows"]
    g = w15.extras["global_window"]
    assert {k: g[k] for k in ("min_enthalpy", "max_enthalpy", "bin_size")} == {k: w4.config_kwargs[k] for k in ("min_enthalpy", "max_enthalpy", "bin_size")}
    assert (wx.L, wx.n_windows, wx.copies, wx.R) == (512, 16, 4, 64) and 0.7 < 1 - wx.Ls / wx.Lw < 0.8
    assert (w15.config_kwargs["min_enthalpy"], w15.config_kwargs["max_enthalpy"]) == (wx.vmin[0], wx.vmax[0])
    assert np.array_equal(w15.occupancy, w4.occupancy) and w15.key == 15
    with pytest.raises(ValueError, match="multiple of 16"):
        workloads.config15(count=40, dim=4)


# ---- the Sampler is built from the windows (no engine needed) ----------------------------------------------------------
def test_sampler_from_ensemble_with_windows():
    from smol_amd import moca

    c = wc.case()
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    wx = wc.windows(5)
    kw = dict(kernel_type="Wang-Landau", min_enthalpy=c["lo"], max_enthalpy=c["hi"], bin_size=c["bin"], check_period=500)
    s = moca.Sampler.from_ensemble(ens, windows=wx, seeds=list(range(wx.R)), **kw)
    assert len(s.mckernels) == wx.R and s.samples._schema["wl_estimator"] == (np.dtype(np.int32), (wx.R, 1))
    assert s.samples._schema["entropy"][1] == (wx.R, wx.Lw)
    for e, k in enumerate(s.mckernels):
        assert k._window == (wx.vmin[e], wx.vmax[e], wx.bin_size) and len(k._levels) == wx.Lw and k._levels[0] == wx.vmin[e]
    with pytest.raises(ValueError, match="Wang-Landau"):
        moca.Sampler.from_ensemble(ens, windows=wx, **dict(kw, kernel_type="Metropolis"))
    with pytest.raises(ValueError, match="global range"):
        moca.Sampler.from_ensemble(ens, windows=wx, **dict(kw, max_enthalpy=c["hi"] + 1.0))
    with pytest.raises(ValueError, match="estimators"):
        moca.Sampler.from_ensemble(ens, windows=wx, nwalkers=wx.R + 1, **kw)
    with pytest.raises(ValueError, match="wl_joined_entropy needs"):
        moca.Sampler.from_ensemble(ens, c["lo"], c["hi"], c["bin"], kernel_type="Wang-Landau").wl_joined_entropy()


# ---- the scheme on the CPU oracle against exact enumeration ---------------------------------------------------------
def run_oracle_rewl(seed):
    """Replica-exchange Wang-Landau on one-walker oracles, one per estimator with its window, driven by
    WLWindows.decide; an accepted exchange moves the two occupancies (set_state without resetting the aux state)."""
    from oracle import oracle as orc

    c = wc.case()
    wx = wc.windows(seed)
    occ = wc.start_occupancies(wx, seed)
    oras = []
    for e in range(wx.R):
        o = orc.OracleMC(c["tab"], wc.config(1, wx.vmin[e], wx.vmax[e]))
        assert o.L == wx.Lw
        o.set_state(occ[e:e + 1], np.array([100 * seed + e], dtype=np.uint64), 0.0)
        oras.append(o)
    identity = np.arange(wx.R)
    for _ in range(wc.ROUNDS):
        for o in oras:
            o.run(wc.STEPS)
        st = [o.get_state() for o in oras]
        H = np.array([s["enthalpy"][0] for s in st])
        S = np.stack([o.get_wl()["entropy"][0] for o in oras])
        res = wx.decide(H, S, identity, wx.move_of(wx.calls), wx.calls)
        for (s, t), acc in zip(res["pairs"], res["accept"]):
            if acc:
                oras[s].set_state(st[t]["occupancy"], np.zeros(1, dtype=np.uint64), 0.0, reset_aux=False)
                oras[t].set_state(st[s]["occupancy"], np.zeros(1, dtype=np.uint64), 0.0, reset_aux=False)
        wx.calls += 1
    S = np.stack([o.get_wl()["entropy"][0] for o in oras])
    return wx, S


# Measured (CPU oracle, this test's settings): seed -> acceptance, RMS of copy 0, copy 1, of the mean over copies
#   5 -> 0.276, 0.0305, 0.0481, 0.0291    6 -> 0.280, 0.0510, 0.0414, 0.0222    7 -> 0.255, 0.0675, 0.0794, 0.0558
# against the bound of 0.2046 (tests/wl_windows_case.py); all 21 occupied bins visited in every run.
@pytest.mark.parametrize("seed", [5, 6, 7])
def test_replica_exchange_wang_landau_converges_to_the_exact_density_of_states(seed):
    c = wc.case()
    assert len(c["E"]) == 12870 and c["occupied"].sum() == 21
    wx, S = run_oracle_rewl(seed)
    ln_g, per_copy, visited = wx.join(S)
    rms = [wc.rms_vs_exact(per_copy[i], per_copy[i] != 0) for i in range(wx.copies)]
    print(f"seed {seed}: acceptance {wx.acceptance:.3f}, rms per copy {rms}, joined {wc.rms_vs_exact(ln_g, visited):.4f}, "
          f"visited {int((visited & c['occupied']).sum())} of {int(c['occupied'].sum())} occupied bins")
    assert (visited >= c["occupied"]).all()  # every occupied bin was reached
    assert wx.acceptance > 0.05
    for r in rms:
        assert r < wc.RMS_BOUND, (rms, wc.RMS_BOUND)
    assert wc.rms_vs_exact(ln_g, visited) < wc.RMS_BOUND
