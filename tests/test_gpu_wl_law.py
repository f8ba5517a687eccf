"""The device's native Wang-Landau chains against their exact transition law (tests/wl_law.py): the frozen tier
(entropies set through ``Engine.set_wl``, modification factor 2^-64) and the live tier (paths of two and three steps),
one launch per (case, tier, n, update period), the kernel family asserted from ``kernel_info``.  Under the same seeds the
device's outcomes are also the CPU oracle's, walker for walker: the first native parity check that starts from a set,
non-trivial entropy.  ``test_set_wl_then_sampling_matches_the_oracle`` runs 200 live steps from set entropies on one case
of every kernel family."""

import numpy as np
import pytest

from smol_amd import capi
from tests import wl_law as wl

pytestmark = pytest.mark.gpu

PARITY = ["fcc222-flip", "fcc223-swap", "rocksalt224-ewald-swap", "fcc223-swap-windows", "rocksalt322-two-sublattices",
          "rocksalt322-two-sublattices-windows", "fcc223-ternary-corr-kf", "rocksalt222-table-flip",
          "rocksalt222-table-flip-two-sublattices", "fcc222-flip-general", "fcc223-swap-general", "rocksalt322-general",
          "fcc222-flip-universal", "fcc223-swap-universal", "rocksalt322-universal"]


def _clean(monkeypatch, case):
    for v in wl.DISPATCH_SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


def _engine(case, R, run):
    from smol_amd.engine import Engine

    return Engine(case.built["tab"], wl.config_for(case, list(range(case.law.G)), R, run))


def _family(case, eng, period):
    info = eng.kernel_info()  # (after the launch: the windows are part of the dispatch)
    print(f"[wl law] {case.name}: {info}")
    assert case.family_ok(info, period), (case.want, case.wont, period, info)
    if "table-flip" in case.name:  # (one tag for the multi families: TableFlip on lean-multi without kf is K_MULTI_TABLE_WL)
        assert eng.config.step_type == capi.STEP_TABLE_FLIP and " kf=1" not in info
    if " wl=multi" in info:  # per-bin sums at update period 1, running means otherwise
        assert (" wl=multi-mean" in info) == (period != 1), info


@pytest.mark.parametrize("name,tier,n,period", wl.DEVICE_RUNS)
def test_device_chain_follows_its_law(name, tier, n, period, monkeypatch, record_property):
    case, run = wl.CASES[name], (tier, n, period)
    _clean(monkeypatch, case)
    law, R = case.law, case.R
    wl.assert_pooling_cap(case, R)
    Rh = wl.host_R(case, run)  # the oracle's walkers: the same seeds as the first Rh of every group here
    eng = _engine(case, R, run)
    try:
        samples, heads = wl.run_handle(case, eng, list(range(law.G)), R, run, head=Rh)
        _family(case, eng, period)
        for g, s in enumerate(samples):  # the law's H is the handle's H, on the states the walkers ended in
            rows = s.rows[:8, :law.N].astype(np.int32)
            want = np.array([law.enthalpy(g, r) for r in rows])
            np.testing.assert_allclose(eng.eval_full(rows) @ eng.natural_parameters, want, rtol=1e-10, atol=1e-9)
    finally:
        eng.close()
    for a, b in zip(heads, wl.oracle_samples(name, run, Rh)):
        assert a.same_as(b), "the device's outcomes are not the oracle's under the same seeds"
    bad = []
    for g, s in enumerate(samples):
        key = (tier, g, n, period)
        res = wl.evaluate(case.expected(key), s)
        record_property(f"wl_law_{name}_{tier}_g{g}_n{n}_p{period}", wl.report(case, key, res, "device"))
        if not wl.passes(res, wl.ALPHA):
            bad.append((g, res))
    assert not bad, bad


@pytest.mark.parametrize("period", [1, 2])
@pytest.mark.parametrize("name", PARITY)
def test_set_wl_then_sampling_matches_the_oracle(name, period, monkeypatch):
    """``Engine.set_wl(entropy=S0, mod_factor=m)`` against ``OracleMC.set_wl`` with the same arguments, then 200 native
    steps with a modification factor of the order of the entropy differences: occupancies, counters, histogram and
    occurrences equal; entropy and mean features within the tolerance of tests/test_gpu_long_streams.py."""
    from oracle import oracle as orc

    case, R, n = wl.CASES[name], 48, 200
    run = ("parity", n, period)
    _clean(monkeypatch, case)
    groups = list(range(case.law.G))
    eng = _engine(case, R, run)
    try:
        wl.prepare(case, eng, groups, R, run, wl.M_LIVE)
        eng.run(n)
        _family(case, eng, period)
        a, x = eng.get_state(), eng.get_wl()
    finally:
        eng.close()
    for g in groups:  # (the oracle has one window: one oracle per state point)
        ora = orc.OracleMC(case.built["tab"], wl.config_for(case, [g], R, run))
        wl.prepare(case, ora, [g], R, run, wl.M_LIVE)
        ora.run(n)
        b, y = ora.get_state(), ora.get_wl()
        sl = slice(g * R, (g + 1) * R)
        assert np.array_equal(a["occupancy"][sl], b["occupancy"])
        assert np.array_equal(a["n_accepted"][sl], b["n_accepted"]) and np.array_equal(a["n_steps"][sl], b["n_steps"])
        assert 0.05 < b["n_accepted"].mean() / n < 0.95  # (the entropy rule both accepts and rejects)
        assert np.array_equal(x["histogram"][sl], y["histogram"]) and np.array_equal(x["occurrences"][sl], y["occurrences"])
        assert np.all(y["histogram"].sum(axis=1) == n // period)
        np.testing.assert_allclose(a["enthalpy"][sl], b["enthalpy"], rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(x["entropy"][sl], y["entropy"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(x["mean_features"][sl], y["mean_features"], rtol=1e-12, atol=1e-12)
        assert np.array_equal(x["mod_factor"][sl], y["mod_factor"])
