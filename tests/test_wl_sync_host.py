"""The merge of a window's copies (parallel.WLWindows.synchronise, smolmc_wl_synchronise) without a device: the
definition on hand-made arrays that take every branch, the scheme in a plain Python chain (tests/wl_sync_case.py:
numpy_rewl) against the exact density of states, and the Python layers around the call.

The chain on the enumerated 16-site case, 3 windows of 12 bins at a stride of 6, 400 rounds of 500 steps, flatness 0.8,
divisor 2 (python -m tests.wl_sync_case; "independent": every estimator checks itself after each round, the scheme of
the sampling kernels; "merged": one synchronise after each round; RMS of ln g against the exact counts, bound 0.2046):

  copies seed scheme       RMS per copy    joined  final factors          merges per window
  2      5    independent  0.056 - 0.066   0.038   6.9e-18 .. 3.8e-06     -
  2      5    merged       0.034 - 0.050   0.040   equal in each window   14, 49, 26
  2      6    independent  0.059 - 0.075   0.031   6.8e-21 .. 4.8e-07     -
  2      6    merged       0.033 - 0.039   0.036   equal in each window   15, 58, 28
  2      7    independent  0.057 - 0.059   0.045   8.7e-19 .. 1.2e-10     -
  2      7    merged       0.048 - 0.048   0.048   equal in each window   22, 40, 34
  4      5    independent  0.036 - 0.078   0.022   4.2e-22 .. 1.9e-06     -
  4      5    merged       0.011 - 0.014   0.011   equal in each window   15, 47, 26
  4      6    independent  0.036 - 0.108   0.037   6.8e-21 .. 1.5e-05     -
  4      6    merged       0.022 - 0.023   0.022   equal in each window   17, 37, 30
  4      7    independent  0.048 - 0.080   0.030   2.7e-20 .. 3.8e-06     -
  4      7    merged       0.019 - 0.025   0.019   equal in each window   14, 44, 29

Every occupied bin was visited in all twelve runs; 25 - 30 % of the exchanges were accepted.  With merging every copy
is about as good as the join over all independent copies."""

import os
import re

import numpy as np
import pytest

from smol_amd import capi, engine, moca, parallel
from tests import wl_sync_case as sc
from tests import wl_windows_case as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(6, 2), (15, 3), (15, 5)]


def _wx(copies):
    return parallel.WLWindows(0.0, 12.0, 1.0, 1, copies=copies)


# ---- the definition on hand-made arrays ------------------------------------------------------------------------------
@pytest.mark.parametrize("R,copies", SHAPES)
@pytest.mark.parametrize("third", ["single", "factors"])
def test_synchronise_takes_every_branch_of_the_definition(R, copies, third):
    S, hist, m, want = sc.planted(R, copies, third=third)
    S0, hist0, m0 = S.copy(), hist.copy(), m.copy()
    res = _wx(copies).synchronise(S, hist, m, copies=copies, flatness=sc.FLATNESS, divisor=sc.DIVISOR)
    assert np.array_equal(S, S0) and np.array_equal(hist, hist0) and np.array_equal(m, m0)  # (the inputs are not written)
    assert res["status"].dtype == np.int32 and np.array_equal(res["status"], want), (res["status"], want)
    assert want[0] == 1 and want[1] == 0 and want[2] == (0 if third == "single" else 2)
    for g, st in enumerate(want):
        e = slice(g * copies, (g + 1) * copies)
        if st == 1:
            a = S0[g * copies].copy()
            for c in range(1, copies):
                a = a + S0[g * copies + c]
            assert np.array_equal(res["entropy"][e], np.broadcast_to(a / copies, (copies, S.shape[1])))
            assert not res["histogram"][e].any() and np.array_equal(res["mod_factor"][e], m0[e] / sc.DIVISOR)
        else:  # left alone, bit for bit
            assert np.array_equal(res["entropy"][e], S0[e]) and np.array_equal(res["histogram"][e], hist0[e])
            assert np.array_equal(res["mod_factor"][e].view(np.uint64), m0[e].view(np.uint64))
    # a bin one copy visited takes the plain mean with the other copies' zeros, and counts as visited in every copy
    assert (S0[:copies, 3] > 0).sum() == 1 and np.array_equal(res["entropy"][:copies, 3], np.full(copies, 7.25 / copies))
    # a bin no copy visited stays 0; a group whose status is 2 is flat all the same (the factors are looked at first)
    assert not res["entropy"][:copies, 7].any()
    for g in np.flatnonzero(want == 2):
        assert all(parallel.WLWindows.flat(S0[e], hist0[e], sc.FLATNESS) for e in range(g * copies, (g + 1) * copies))


@pytest.mark.parametrize("R,copies", SHAPES)
def test_strict_threshold_and_single_bin(R, copies):
    """The count exactly at flatness x mean keeps its copy not flat (strict >); one more and the group merges.  A copy
    with one visited bin is never flat, whatever its histogram."""
    wx = _wx(copies)
    at = sc.planted(R, copies, at_threshold=True)
    above = sc.planted(R, copies, at_threshold=False)
    e = 2 * copies - 1  # the last copy of group 1
    V = at[0][e] > 0
    assert V.sum() == 2 and np.float64(sc.FLATNESS) * (np.float64(at[1][e][V].sum()) / 2.0) == at[1][e][V].min() == 1000.0
    assert not wx.flat(at[0][e], at[1][e], sc.FLATNESS) and wx.flat(above[0][e], above[1][e], sc.FLATNESS)
    assert (above[1] - at[1]).sum() == 1
    r_at = wx.synchronise(*at[:3], copies=copies, flatness=sc.FLATNESS, divisor=sc.DIVISOR)
    r_above = wx.synchronise(*above[:3], copies=copies, flatness=sc.FLATNESS, divisor=sc.DIVISOR)
    assert (r_at["status"][1], r_above["status"][1]) == (0, 1) == (at[3][1], above[3][1])
    single = copies * 2 + copies // 2
    assert (at[0][single] > 0).sum() == 1 and not wx.flat(at[0][single], np.full(12, 1000), 0.0)
    assert not wx.flat(np.zeros(12), np.full(12, 1000), 0.0)


@pytest.mark.parametrize("values", [sc.ORDER_3, sc.ORDER_5], ids=["3", "5"])
def test_the_copy_sum_runs_in_ascending_order(values):
    """Group 0's bin 5 holds entropies whose sum depends on the order; the merge gives the ascending one."""
    copies = len(values)
    S, hist, m, want = sc.planted(15, copies)
    assert np.array_equal(S[:copies, 5], values)
    res = _wx(copies).synchronise(S, hist, m, copies=copies, flatness=sc.FLATNESS, divisor=sc.DIVISOR)
    up, down = sc.ascending_mean(values), sc.ascending_mean(values[::-1])
    assert up != down, "the input has no teeth: both orders give the same sum"
    assert res["status"][0] == 1 and np.array_equal(res["entropy"][:copies, 5], np.full(copies, up))
    assert up == 1.0 / copies and down == (1.0 + (copies - 1) * 2.0 ** -53) / copies


def test_synchronise_refuses_shapes_that_do_not_fit():
    wx = _wx(2)
    with pytest.raises(ValueError, match="does not divide"):
        wx.synchronise(np.zeros((6, 12)), np.zeros((6, 12), dtype=np.int64), np.ones(6), copies=4)
    with pytest.raises(ValueError, match="do not belong together"):
        wx.synchronise(np.zeros((6, 12)), np.zeros((5, 12), dtype=np.int64), np.ones(6))
    assert wx.merges.tolist() == [0] and np.isnan(wx.mod_factor).all() and not wx.converged(1.0)
    wx.mod_factor = np.array([2.0 ** -10])
    assert wx.converged(2.0 ** -10) and not wx.converged(2.0 ** -11)


# ---- the scheme against the exact density of states ----------------------------------------------------------------------
def test_merged_copies_converge_to_the_exact_density_of_states():
    r = sc.numpy_rewl(5, 2, True)
    wx, m = r["wx"], r["mod_factor"]
    print(f"seed 5, 2 copies, merged: rms per copy {r['rms']}, joined {r['joined']:.4f}, merges {r['merges'].tolist()}, "
          f"factors {m[::2].tolist()}, acceptance {wx.acceptance:.3f}")
    assert (r["visited"] >= wc.case()["occupied"]).all()
    mw = m.reshape(wx.n_windows, wx.copies)
    assert np.array_equal(mw.view(np.uint64), np.repeat(mw[:, :1], wx.copies, axis=1).view(np.uint64))
    assert r["merges"].min() >= 7  # (half of the smallest count, 14, of the six merged runs in the table above)
    assert max(r["rms"]) < wc.RMS_BOUND and r["joined"] < wc.RMS_BOUND, (r["rms"], r["joined"], wc.RMS_BOUND)


# ---- the Python layers without a device ------------------------------------------------------------------------------
class _NoDevice(Exception):
    pass


def _sampler(monkeypatch, seen, **kw):
    def fake_engine(tables, cfg, distance=None):
        seen.append(cfg)
        raise _NoDevice()

    monkeypatch.setattr(moca, "Engine", fake_engine)
    c = wc.case()
    wx = wc.windows(6)
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    sampler = moca.Sampler.from_ensemble(ens, kernel_type="Wang-Landau", min_enthalpy=c["lo"], max_enthalpy=c["hi"], bin_size=c["bin"],
                                         check_period=wc.CHECK_PERIOD, windows=wx, seeds=list(range(60, 60 + wx.R)), **kw)
    return sampler, wx, ens


def test_sampler_synchronise_creates_the_handle_with_check_period_zero(monkeypatch):
    seen = []
    sampler, wx, _ = _sampler(monkeypatch, seen, synchronise=True)
    with pytest.raises(_NoDevice):
        sampler._get_engine()
    assert len(seen) == 1 and seen[0].wl_check_period == 0 and seen[0].kernel_type == capi.KERNEL_WANGLANDAU
    assert all(k.check_period == wc.CHECK_PERIOD and k.spec["check_period"] == wc.CHECK_PERIOD for k in sampler.mckernels)
    plain, _, ens = _sampler(monkeypatch, seen)
    with pytest.raises(_NoDevice):
        plain._get_engine()
    assert seen[1].wl_check_period == wc.CHECK_PERIOD
    with pytest.raises(ValueError, match="synchronise=True needs windows="):
        moca.Sampler.from_ensemble(ens, kernel_type="Wang-Landau", min_enthalpy=0.0, max_enthalpy=1.0, bin_size=0.1, synchronise=True)


def test_sync_every_without_synchronise_is_refused_and_names_the_argument(monkeypatch):
    seen = []
    sampler, wx, _ = _sampler(monkeypatch, seen)
    with pytest.raises(ValueError, match=r"sync_every= needs a sampler built with .*synchronise=True"):
        sampler.run_exchange(4, 100, wc.start_occupancies(wx, 6), windows=wx, sync_every=1)
    synced, wx2, _ = _sampler(monkeypatch, seen, synchronise=True)
    with pytest.raises(ValueError, match="final_mod_factor= needs sync_every="):
        synced.run_exchange(4, 100, wc.start_occupancies(wx2, 6), windows=wx2, final_mod_factor=0.5)
    assert not seen  # (refused before a handle is made)
    with pytest.raises(ValueError, match="final_mod_factor needs sync_every"):
        parallel.run_wl_exchange(type("E", (), {"R": wx.R})(), wx, 1, 1, final_mod_factor=0.5)


def test_header_capi_and_library_agree_on_the_prototype():
    import ctypes as C

    text = open(os.path.join(ROOT, "include", "smolmc.h")).read()
    proto = re.search(r"int smolmc_wl_synchronise\((.*?)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["smolmc_handle *h", "int copies", "int32_t *status_out", "double *mod_factor_out"]
    restype, argtypes = engine.SYMBOLS["smolmc_wl_synchronise"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    assert capi.ABI_VERSION == int(re.search(r"#define SMOLMC_ABI_VERSION (\d+)", text).group(1)) == 8
    for word in ("bitwise equal", "a = a + S_e0+c[i]", "wl_check_period != 0", "every bin i"):
        assert word in text, word  # (the header states the definition in full)
    import __graft_entry__ as g

    if not os.path.exists(engine.LIB_PATH):
        g.build()
    lib = engine.load_library()
    assert hasattr(lib, "smolmc_wl_synchronise") and lib.smolmc_wl_synchronise.argtypes == argtypes
    assert hasattr(engine.Engine, "wl_synchronise")
