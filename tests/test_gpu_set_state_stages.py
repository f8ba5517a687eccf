"""smolmc_set_state stage by stage (engine.hip: apply_temperatures, reset_counters, initial_bias, init_ewald_field,
initial_trace, wl_reset, wl_check_window) against oracle.OracleMC.set_state, on one handle per stage that has work to do:
the three MCBias terms, Wang-Landau, a lean handle with the Ewald field in LDS, per-walker chemical potentials.

R = 3 walkers on the cells of tests/v6_cases.py and the two smallest fitting cells of tests/dispatch_targets.py.
Occupancies, counters and flags are exact; features, enthalpies and bias values are held to the suite's 1e-10 relative
(with its absolute floors for entries that are zero: 1e-8 on features, 1e-9 on enthalpy and bias)."""

import collections
import functools
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import dispatch_matrix as dm
from tests.v6_cases import build
from tests.wl_window_oracle import enthalpies

pytestmark = pytest.mark.gpu
R = 3
RTOL, ATOL, FEATURE_ATOL = dm.RTOL, dm.ATOL, dm.FEATURE_ATOL
EWALD_LDS = "salt1-22-flip-m-e-int-run-auto-R6"  # the smallest cell whose kernel_info() reads "lean ... field=1"
WALKER_MU = "fcc-22-flip-m-u-int-wmu-auto-R3"
HANDLES = ["BC_fug_flip_int", "BG_sqc_swap_int", "BG_hyp_flip_int", "B_wlup3", EWALD_LDS, WALKER_MU]
SWITCHES = ("SMOLMC_REPLAY_GENERAL", "SMOLMC_REPLAY_UNIVERSAL", "SMOLMC_FORCE_GENERAL", "SMOLMC_FORCE_UNIVERSAL",
            "SMOLMC_NO_EWALD_FIELD")

Handle = collections.namedtuple("Handle", "tab cfg occ_a occ_b temps temps_b rows oracle wl bias")
SEEDS_A = np.arange(R, dtype=np.uint64) * np.uint64(7919) + np.uint64(1001)
SEEDS_B = SEEDS_A + np.uint64(17)


class _PerWalker(dm._Walkers):
    """R one-walker oracles, each with its own chemical-potential table (per-walker rows), as one object."""

    def set_state(self, occ, seeds, temps, reset_aux=True):
        for r, w in enumerate(self.walkers):
            w.set_state(occ[r:r + 1], seeds[r:r + 1], temps[r:r + 1], reset_aux)


@functools.lru_cache(maxsize=None)
def handle(name):
    """Tables, config, two sets of starting occupancies (the second: the oracle's states after 12 steps from the first),
    two sets of temperatures, the per-walker rows or None, and a factory of fresh oracles."""
    rows = None
    if name in dm.TARGETS:
        cell = next(x for x in dm.CASES if x.id == name)
        tab, cfg = dm.case_tables(cell), dm.config(cell, R=R)
        occ_a, temps = dm.start(cell)[0][:R].copy(), np.linspace(1500.0, 6000.0, R)
        wl, bias = False, cell.bias
        if cell.drive == "wmu":
            rows, scales = dm.walker_rows(cell), np.linspace(-2.0, 2.0, R)
            assert cell.R == R
            one = dm.config(cell, R=1)
            oracle = lambda: _PerWalker([orc.OracleMC(dm.case_tables(cell, float(s)), one) for s in scales])  # noqa: E731
        else:
            oracle = lambda: orc.OracleMC(tab, cfg)  # noqa: E731
    else:
        tab, cfg, occ0, temp = build(name, n_replicas=R)
        occ_a, temps = np.tile(occ0, (R, 1)), np.full(R, float(temp))
        wl, bias = name == "B_wlup3", name != "B_wlup3"
        oracle = lambda: orc.OracleMC(tab, cfg)  # noqa: E731
    ora = oracle()
    ora.set_state(occ_a, SEEDS_A, temps)
    ora.run(12)
    occ_b = ora.get_state()["occupancy"].copy()
    assert (occ_b != occ_a).any()
    temps_b = temps if wl else temps * np.array([1.0, 1.5, 2.0])
    return Handle(tab, cfg, occ_a, occ_b, temps, temps_b, rows, oracle, wl, bias)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _engine(hd):
    from smol_amd.engine import Engine

    eng = Engine(hd.tab, hd.cfg)
    if hd.rows is not None:
        eng.set_walker_mu(hd.rows)
    return eng


def same(eng, ora, hd):
    a, b = eng.get_state(), ora.get_state()
    for k in ("occupancy", "n_steps", "n_accepted", "accepted"):
        assert np.array_equal(a[k], b[k]), k
    np.testing.assert_allclose(a["features"], b["features"], rtol=RTOL, atol=FEATURE_ATOL)
    np.testing.assert_allclose(a["enthalpy"], b["enthalpy"], rtol=RTOL, atol=ATOL)
    if hd.bias:
        np.testing.assert_allclose(eng.get_bias(), ora.get_bias(), rtol=RTOL, atol=ATOL)
    if hd.wl:
        x, y = eng.get_wl(), ora.get_wl()
        for k in ("entropy", "histogram", "occurrences"):
            assert np.array_equal(x[k], y[k]), k
        np.testing.assert_allclose(x["mod_factor"], y["mod_factor"])
        np.testing.assert_allclose(x["mean_features"], y["mean_features"], rtol=RTOL, atol=ATOL)
    return a


def test_the_handles_are_what_the_stages_need():
    want = {"BC_fug_flip_int": "lean ", "BG_sqc_swap_int": "lean-multi", "BG_hyp_flip_int": "lean-multi", "B_wlup3": "lean-multi",
            EWALD_LDS: "lean ", WALKER_MU: "lean "}
    for name in HANDLES:
        eng = _engine(handle(name))
        info = eng.kernel_info()
        assert info.startswith(want[name]), info
        if name == EWALD_LDS:  # (a lean handle's field=1: the potential field lives in LDS)
            assert " field=1" in info, info
        assert ("walker_mu=1" in info) == (name == WALKER_MU), info
        eng.close()


@pytest.mark.parametrize("name", HANDLES)
def test_reset_equals_the_oracles_set_state(name):
    hd = handle(name)
    eng, ora = _engine(hd), hd.oracle()
    eng.set_state(hd.occ_a, SEEDS_A, hd.temps)
    eng.run(9)
    assert eng.get_state()["n_steps"].all()
    eng.set_state(hd.occ_b, SEEDS_B, hd.temps_b)
    ora.set_state(hd.occ_b, SEEDS_B, hd.temps_b)
    a = same(eng, ora, hd)
    assert np.array_equal(a["occupancy"], hd.occ_b)
    assert not a["n_steps"].any() and not a["n_accepted"].any() and a["accepted"].all()
    if hd.wl:
        wl = eng.get_wl()
        assert not wl["histogram"].any() and not wl["entropy"].any() and not wl["occurrences"].any()
        assert (wl["mod_factor"] == hd.cfg.wl_mod_factor).all()
    eng.run(7)  # the new seeds, from step 0, at the new temperatures
    ora.run(7)
    same(eng, ora, hd)
    eng.close()


@pytest.mark.parametrize("name", HANDLES)
def test_continuation_keeps_counters_and_estimate_and_recomputes_the_trace(name):
    hd = handle(name)
    eng, ora = _engine(hd), hd.oracle()
    eng.set_state(hd.occ_a, SEEDS_A, hd.temps)
    ora.set_state(hd.occ_a, SEEDS_A, hd.temps)
    eng.run(9)
    ora.run(9)
    before, wl_before = eng.get_state(), eng.get_wl() if hd.wl else None
    assert (before["n_steps"] == 9).all() and before["n_accepted"].any()
    eng.set_state(hd.occ_b, SEEDS_B, hd.temps_b, reset_aux=False)
    ora.set_state(hd.occ_b, SEEDS_B, hd.temps_b, reset_aux=False)
    a = same(eng, ora, hd)
    assert np.array_equal(a["n_steps"], before["n_steps"]) and np.array_equal(a["n_accepted"], before["n_accepted"])
    assert a["accepted"].all()
    full = eng.eval_full(hd.occ_b)
    if hd.rows is not None:  # (eval_full prices the handle's own table: the chemical work of the rows is the last column)
        full[:, -1] = eng.chemical_work(hd.occ_b, hd.rows)
    np.testing.assert_allclose(a["features"], full, rtol=RTOL, atol=FEATURE_ATOL)
    np.testing.assert_allclose(a["enthalpy"], full @ eng.natural_parameters, rtol=RTOL, atol=ATOL)
    if hd.wl:
        wl = eng.get_wl()
        assert wl_before["histogram"].any()
        for k in wl_before:
            assert np.array_equal(wl[k], wl_before[k]), k
    eng.run(7)  # the old seeds go on from step 9
    ora.run(7)
    b = same(eng, ora, hd)
    assert (b["n_steps"] == 16).all()
    eng.close()


WINDOW_TEXT = re.compile(r"initial enthalpy (-?\d+\.\d{6}) of walker (\d+) is outside the Wang-Landau window "
                         r"\[min_enthalpy, max_enthalpy\) = \[(-?\d+\.\d{6}), (-?\d+\.\d{6})\)(.*)")


def _window_refusal(eng, occ, walker, H, lo, hi, suffix):
    with pytest.raises(ValueError) as e:
        eng.set_state(occ, SEEDS_A)
    m = WINDOW_TEXT.fullmatch(str(e.value))
    assert m, str(e.value)
    assert int(m.group(2)) == walker and m.group(5) == suffix
    assert m.group(3) == f"{lo:.6f}" and m.group(4) == f"{hi:.6f}"
    assert abs(float(m.group(1)) - H) <= 1e-6 + 1e-10 * abs(H)


def test_an_initial_enthalpy_outside_the_window_is_refused():
    hd = handle("B_wlup3")
    lo, hi = hd.cfg.wl_min_enthalpy, hd.cfg.wl_max_enthalpy
    rng = np.random.default_rng(3)
    outside = next(o for o in (rng.permutation(hd.occ_a[0]) for _ in range(200))
                   if not lo <= enthalpies(hd.tab, o[None])[0] < hi)
    H = enthalpies(hd.tab, outside[None])[0]
    occ = hd.occ_a.copy()
    occ[1] = outside
    eng = _engine(hd)
    _window_refusal(eng, occ, 1, H, lo, hi, "")  # the config's window
    # per-walker windows of the same width: walker 2's lies above its enthalpy
    H0 = enthalpies(hd.tab, hd.occ_a)
    width = hi - lo
    vmin = np.array([lo, lo, H0[2] + 5 * hd.cfg.wl_bin_size])
    vmax = vmin + width
    assert (np.ceil((vmax - vmin) / hd.cfg.wl_bin_size) == eng.L).all()
    eng.set_wl_windows(vmin, vmax)
    _window_refusal(eng, hd.occ_a, 2, H0[2], vmin[2], vmax[2], " the walker holds (smolmc_set_wl_windows)")
    eng.set_wl_windows(None, None)
    eng.set_state(hd.occ_a, SEEDS_A)
    eng.close()


def test_set_temperature_names_the_state_points_as_set_state_does():
    """On a grid handle (per-walker rows, one exchange behind it): set_temperature and set_state with the same
    temperatures leave the same state points, and the same chains."""
    hd = handle(WALKER_MU)
    engines = []
    for via_set_state in (False, True):
        eng = _engine(hd)
        eng.set_state(hd.occ_a, SEEDS_A, hd.temps)
        stats = np.zeros((1, 2), dtype=np.int64)
        eng.exchange_grid([[0, 2]], [-1e300], stats)
        assert stats.tolist() == [[1, 1]]
        point_of, temp = eng.state_points()
        assert point_of.tolist() == [2, 1, 0] and np.array_equal(temp, hd.temps[[2, 1, 0]])
        if via_set_state:
            eng.set_state(hd.occ_a, SEEDS_A, hd.temps_b)
        else:
            eng.set_temperature(hd.temps_b)
        point_of, temp = eng.state_points()
        assert point_of.tolist() == [0, 1, 2] and np.array_equal(temp, hd.temps_b)
        engines.append(eng)
    assert np.array_equal(engines[0].get_walker_mu(), engines[1].get_walker_mu())
    for steps in (0, 7):  # (set_state evaluates the trace afresh, set_temperature keeps the re-priced one: to rounding)
        for eng in engines:
            eng.run(steps)
        a, b = engines[0].get_state(), engines[1].get_state()
        for k in ("occupancy", "n_steps", "n_accepted", "accepted"):
            assert np.array_equal(a[k], b[k]), k
        np.testing.assert_allclose(a["features"], b["features"], rtol=RTOL, atol=FEATURE_ATOL)
        np.testing.assert_allclose(a["enthalpy"], b["enthalpy"], rtol=RTOL, atol=ATOL)
    for eng in engines:
        eng.close()
