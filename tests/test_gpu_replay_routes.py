"""smolmc_replay: the route each kind of call takes (engine.hip: replay_route) and what it returns there.

One case per row of the rule -- handle x records x the two environment switches -> lean | lean-table | general |
universal -- with the route read from the SMOLMC_DEBUG line and the result held against oracle.OracleMC.replay on the
same records and uniforms: accept flags and final occupancies exact, enthalpies and returned a-priori factors 1e-10
relative (tests/test_gpu_replay_v6.py's tolerance).  Records are the first steps of the golden trajectories
(tests/v6_cases.py), edited by hand where a row needs it; R = 3 walkers, 8 records each.

The row "a lean Flip handle, records of two flips, general_ok false" (two flips -> the universal kernel because
mc_kernel refused the model at smolmc_create) is not constructible on these cells: every model of tests/v6_cases.py
that a lean family takes is one mc_kernel takes too.  It has no case here.

BG_hyp_flip_int is a lean-multi handle with a hyperplane bias, not an mc_kernel handle: its own steps take the lean
route, and the row "an mc_kernel handle, its own steps -> general" is the same trajectory under SMOLMC_FORCE_GENERAL.

Then the refusals, each by its full text, a distance handle's replay against the NumPy definition of
tests/test_gpu_sqs.py, and the empty call.  (nsteps >= 2^30 keeps a lean handle off its own kernels; that arm cannot be
run and is left to review.)"""

import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from smol_amd import capi
from tests.v6_cases import T6, build

pytestmark = pytest.mark.gpu
R, N_REC = 3, 8
SWITCHES = ("SMOLMC_REPLAY_GENERAL", "SMOLMC_REPLAY_UNIVERSAL", "SMOLMC_FORCE_GENERAL", "SMOLMC_FORCE_UNIVERSAL")


def _engine(tab, cfg, **kw):
    from smol_amd.engine import Engine

    return Engine(tab, cfg, **kw)


# ---- the edits: (steps (N_REC, 16), trajectory's steps, occ0) -> (steps, log_priori (N_REC,) or None) ------------------
def plain(st, more, occ0):
    return st, None


def two_single_flips(st, more, occ0):
    """Record 1 becomes records 1 and 2 in one: two single flips on different sites."""
    assert st[1, 0] != st[2, 0]
    st[1, 2:4] = st[2, 0:2]
    return st, None


def third_flip(st, more, occ0):
    """Record 0 (a swap) gains a third flip: the first flip of a later record on a site the swap does not name."""
    site, code = next((int(s), int(c)) for s, c in more[N_REC:, 0:2] if s not in st[0, 0:4:2] and occ0[s] != c)
    st[0, 4:6] = site, code
    return st, None


def priori_nan_or_zero(st, more, occ0):
    return st, np.where(np.arange(N_REC) % 2, 0.0, np.nan)


def priori_one_value(st, more, occ0):
    lp = np.where(np.arange(N_REC) % 2, 0.0, np.nan)
    lp[0] = -0.35
    return st, lp


def site_twice(st, more, occ0):
    """Record 0 (a row of the flip table on three sites) names its first site twice: to another code first, then to the
    code of the table step -- the same net change, evaluated flip by flip."""
    s, c = int(st[0, 0]), int(st[0, 1])
    other = next(k for k in range(3) if k not in (c, int(occ0[s])))
    st[0, 2:8] = st[0, 0:6].copy()
    st[0, 0:2] = s, other
    return st, None


# (id, trajectory, switches set, edit, route)
ROWS = [
    ("flip-single", "BC_fug_flip_int", (), plain, "lean"),
    ("flip-two-single-flips", "BC_fug_flip_int", (), two_single_flips, "general"),
    ("swap-swaps", "BG_sqc_swap_int", (), plain, "lean"),
    ("swap-three-flips", "BG_sqc_swap_int", (), third_flip, "universal"),
    ("swap-priori-nan-or-zero", "BG_sqc_swap_int", (), priori_nan_or_zero, "lean"),
    ("swap-priori-one-value", "BG_sqc_swap_int", (), priori_one_value, "universal"),
    ("swap-env-general", "BG_sqc_swap_int", ("SMOLMC_REPLAY_GENERAL",), plain, "general"),
    ("swap-env-universal", "BG_sqc_swap_int", ("SMOLMC_REPLAY_UNIVERSAL",), plain, "universal"),
    ("swap-env-both", "BG_sqc_swap_int", ("SMOLMC_REPLAY_GENERAL", "SMOLMC_REPLAY_UNIVERSAL"), plain, "universal"),
    ("table-steps", "TC_tf_int", (), plain, "lean-table"),
    ("table-env-general-ignored", "TC_tf_int", ("SMOLMC_REPLAY_GENERAL",), plain, "lean-table"),
    ("table-site-twice", "TC_tf_int", (), site_twice, "universal"),
    ("table-bias-no-replay-kernel", "TC_tffug_int", (), plain, "universal"),
    ("table-wl-no-replay-kernel", "TC_tfwl_int", (), plain, "universal"),
    ("hyperplane-flip-single", "BG_hyp_flip_int", (), plain, "lean"),
    ("mc-kernel-handle", "BG_hyp_flip_int", ("SMOLMC_FORCE_GENERAL",), plain, "general"),
] + [(f"force-universal-{tag}", tag, ("SMOLMC_FORCE_UNIVERSAL",), plain, "universal")
     for tag in ("BC_fug_flip_int", "BG_sqc_swap_int", "TC_tf_int", "TC_tffug_int", "TC_tfwl_int", "BG_hyp_flip_int")]
# what kernel_info() of the handle starts with (the switches of the row in force at smolmc_create)
FAMILY = {"BC_fug_flip_int": "lean ", "BG_sqc_swap_int": "lean-multi", "TC_tf_int": "lean ", "TC_tffug_int": "lean ",
          "TC_tfwl_int": "lean ", "BG_hyp_flip_int": "lean-multi"}


@functools.lru_cache(maxsize=None)
def case(tag, edit):
    """(tables, config, occ0 (R, N), temperature, steps (R, n, 16), uniforms (R, n), log_priori (R, n) or None) and the
    oracle's side of it, computed once: accepted, H, log_priori out, final state."""
    tab, cfg, occ0, temp = build(tag, n_replicas=R)
    more = T6[f"{tag}_steps"]
    st, lp = edit(more[:N_REC].copy(), more, occ0)
    steps = np.ascontiguousarray(np.tile(st[None], (R, 1, 1)))
    us = np.tile(T6[f"{tag}_u"][None, :N_REC], (R, 1))
    lp = None if lp is None else np.tile(lp[None], (R, 1))
    occ = np.tile(occ0, (R, 1))
    ora = orc.OracleMC(tab, cfg)
    ora.set_state(occ, np.arange(R, dtype=np.uint64), temp)
    acc, H, lpo = ora.replay(steps, us, log_priori=lp, with_priori=True)
    return dict(tab=tab, cfg=cfg, occ=occ, temp=temp, steps=steps, us=us, lp=lp, acc=acc, H=H, lpo=lpo, final=ora.get_state())


def _route(capfd):
    err = capfd.readouterr().err
    return [ln.split("path=")[1].split()[0] for ln in err.splitlines() if "replay path=" in ln][-1]


@pytest.mark.parametrize("rid,tag,env,edit,route", ROWS, ids=[r[0] for r in ROWS])
def test_route_and_result(rid, tag, env, edit, route, monkeypatch, capfd):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k in env:
        monkeypatch.setenv(k, "1")
    monkeypatch.setenv("SMOLMC_DEBUG", "1")  # the engine names the replay path on stderr
    c = case(tag, edit)
    eng = _engine(c["tab"], c["cfg"])
    info = eng.kernel_info()
    assert info.startswith("universal" if "SMOLMC_FORCE_UNIVERSAL" in env else "general" if "SMOLMC_FORCE_GENERAL" in env
                           else FAMILY[tag]), info
    eng.set_state(c["occ"], temperature=c["temp"])
    acc, H, lpo = eng.replay(c["steps"], c["us"], log_priori=c["lp"], with_priori=True)
    assert _route(capfd) == route, info
    assert np.array_equal(acc, c["acc"])
    assert 0 < acc.sum() < acc.size  # (both branches of the step ran)
    np.testing.assert_allclose(H, c["H"], rtol=1e-10, atol=1e-9)
    ok = ~np.isnan(c["lpo"])  # (Wang-Landau never computes it for steps the window rejects)
    np.testing.assert_allclose(lpo[ok], c["lpo"][ok], rtol=1e-10, atol=1e-10)
    if edit is priori_one_value:
        assert (lpo[:, 0] == -0.35).all() and (c["lpo"][:, 0] == -0.35).all()
    st = eng.get_state()
    assert np.array_equal(st["occupancy"], c["final"]["occupancy"])
    assert np.array_equal(st["n_accepted"], c["final"]["n_accepted"])
    np.testing.assert_allclose(st["enthalpy"], c["final"]["enthalpy"], rtol=1e-10, atol=1e-9)
    eng.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _refused(eng, steps, us, text, lp=None):
    with pytest.raises(Exception) as e:
        eng.replay(steps, us, log_priori=lp)
    assert str(e.value) == text


def test_range_refusals(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    c = case("TC_tf_int", plain)
    eng = _engine(c["tab"], c["cfg"])
    eng.set_state(c["occ"], temperature=c["temp"])
    N = eng.N
    inactive = next(s for s in range(N) if s not in np.concatenate(c["tab"].active_sites()))

    def with_record(rec):
        st = c["steps"].copy()
        st[R - 1, N_REC - 1] = -1  # (the last record of the last walker: the scan reads every record)
        st[R - 1, N_REC - 1, :len(rec)] = rec
        return st

    _refused(eng, with_record([N, 0]), c["us"], "replay step out of range")
    _refused(eng, with_record([inactive, 0]), c["us"],
             "replay step out of range: the site is not changeable (not on an active sublattice)")
    site = int(c["steps"][0, 0, 0])
    _refused(eng, with_record([site, 3]), c["us"], "replay step out of range (species code)")
    _refused(eng, with_record([site, -1 - 1]), c["us"], "replay step out of range (species code)")
    st = eng.get_state()  # nothing ran
    assert np.array_equal(st["occupancy"], c["occ"]) and not st["n_steps"].any()
    eng.close()


def test_refused_while_walker_mu_is_set(monkeypatch):
    from tests import dispatch_matrix as dm

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    cell = next(x for x in dm.CASES if x.id == "fcc-22-flip-m-u-int-wmu-auto-R3")
    tab = dm.case_tables(cell)
    occ, seeds, temps = dm.start(cell)
    eng = _engine(tab, dm.config(cell))
    eng.set_walker_mu(dm.walker_rows(cell))
    eng.set_state(occ, seeds, temps)
    site = int(tab.active_sites()[0][0])
    steps = np.tile(np.array([site, 1 - occ[0, site]], dtype=np.int32), (cell.R, 1, 1))
    text = ("smolmc_replay while per-walker chemical potentials are set: the replay kernels price every walker with the "
            "handle's own table (smolmc_set_walker_mu(h, NULL) first)")
    _refused(eng, steps, np.full((cell.R, 1), 0.5), text)
    eng.set_walker_mu(None)
    eng.replay(steps, np.full((cell.R, 1), 0.5))
    eng.close()


def test_refused_while_windows_are_set(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    c = case("B_wlup3", plain)
    eng = _engine(c["tab"], c["cfg"])
    lo, hi = c["cfg"].wl_min_enthalpy, c["cfg"].wl_max_enthalpy
    eng.set_wl_windows(np.full(R, lo), np.full(R, hi))
    eng.set_state(c["occ"], temperature=c["temp"])
    text = ("smolmc_replay while per-walker windows are set: the replay kernels give every walker the config's window "
            "(smolmc_set_wl_windows(h, NULL, NULL) first)")
    _refused(eng, c["steps"], c["us"], text)
    eng.set_wl_windows(None, None)
    acc, H = eng.replay(c["steps"], c["us"])
    assert np.array_equal(acc, c["acc"])
    eng.close()


# ---- a distance handle -------------------------------------------------------------------------------------------------
def _distance_case():
    """The smallest handle of tests/test_gpu_sqs.py (8 sites, aliased) and a swap trajectory through its NumPy definition."""
    from smol_amd import sqs as sqs_mod
    from tests import test_gpu_sqs as sq

    T = 0.1
    m, sc, tab, _, cfg = sq.setup("binary222", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP, R)
    oe = orc.OracleEvaluator(tab)
    spec = sqs_mod.distance_spec(m, capi.FEATURES_CORRELATIONS, sq.ordered_target(oe, sc, 0)[1], None, 1.0, 1e-5, 1.0)
    occ0 = sq.random_occ(sc, R, 11)
    rng = np.random.default_rng(5)
    steps = np.full((R, N_REC, capi.STEP_ROW), -1, dtype=np.int32)
    us = rng.random((R, N_REC))
    acc, Hs, occ_final = np.zeros((R, N_REC), bool), np.zeros((R, N_REC)), occ0.copy()
    for r in range(R):
        occ = occ0[r].copy()
        H = sq.ref_distance(oe, occ, spec, 0)[1]
        for i in range(N_REC):
            while True:
                s1, s2 = rng.integers(0, sc.num_sites, 2)
                if occ[s1] != occ[s2]:
                    break
            steps[r, i, :4] = [s1, occ[s2], s2, occ[s1]]
            new = occ.copy()
            new[s1], new[s2] = occ[s2], occ[s1]
            H2 = sq.ref_distance(oe, new, spec, 0)[1]
            expo = -(H2 - H) / T
            if expo >= 0 or expo > np.log(us[r, i]):
                occ, H, acc[r, i] = new, H2, True
            Hs[r, i] = H
        occ_final[r] = occ
    return tab, cfg, spec, occ0, T, steps, us, acc, Hs, occ_final


def test_distance_handle_replay_and_its_priori_refusal():
    tab, cfg, spec, occ0, T, steps, us, acc_ref, H_ref, occ_ref = _distance_case()
    eng = _engine(tab, cfg, distance=spec)
    assert eng.kernel_info().startswith("dist")
    eng.set_state(occ0, None, T)
    lp = np.full((R, N_REC), np.nan)
    lp[1, ::2] = 0.0
    lp[R - 1, N_REC - 1] = 0.25
    _refused(eng, steps, us, "a distance handle takes no a-priori factor (Flip / Swap: 0, mcusher.py:118-134)", lp=lp)
    lp[R - 1, N_REC - 1] = 0.0  # (NaN and 0 are no factor)
    acc, H, lpo = eng.replay(steps, us, log_priori=lp, with_priori=True)
    assert np.array_equal(acc, acc_ref) and 0 < acc.sum() < acc.size
    np.testing.assert_allclose(H, H_ref, rtol=1e-10, atol=1e-10)
    assert not lpo.any()
    assert np.array_equal(eng.get_state()["occupancy"], occ_ref)
    eng.close()


# ---- the empty call ----------------------------------------------------------------------------------------------------
def test_no_steps_returns_zero_and_writes_nothing(monkeypatch):
    from smol_amd.engine import _p

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    c = case("BG_sqc_swap_int", plain)
    eng = _engine(c["tab"], c["cfg"])
    eng.set_state(c["occ"], temperature=c["temp"])
    before = eng.get_state()
    acc = np.full((R, N_REC), 7, dtype=np.uint8)
    H, lpo = np.full((R, N_REC), 7.5), np.full((R, N_REC), 7.5)
    for n in (0, -1):
        rc = eng._lib.smolmc_replay(eng._h, n, _p(c["steps"], C.c_int32), _p(c["us"], C.c_double), None, _p(acc, C.c_uint8),
                                    _p(H, C.c_double), _p(lpo, C.c_double))
        assert rc == 0
    assert (acc == 7).all() and (H == 7.5).all() and (lpo == 7.5).all()
    after = eng.get_state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    eng.close()
