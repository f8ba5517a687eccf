"""The CPU oracle's native Wang-Landau chains against their exact transition law (tests/wl_law.py): the frozen tier
(entropies set through ``OracleMC.set_wl``, modification factor 2^-64) and the live tier (the law over paths of two and
three steps), and the properties of the laws that need no chain: the conditions on the inputs, the power of every case
at its walker count, detailed balance with pi ~ exp(-S0[b])."""

import numpy as np
import pytest

from tests import wl_law as wl

HOST = wl.HOST_RUNS
OWN = [c.name for c in wl.CASES.values() if not c.twin]


def test_the_statistics_are_counted():
    """three per (case, state point, launch) and module; the level is this tier's own"""
    n = 3 * sum(wl.CASES[r[0]].law.G for r in wl.HOST_RUNS + wl.DEVICE_RUNS)
    assert n == wl.N_STATISTICS and wl.ALPHA == wl.FAMILY_ALPHA / n


def test_set_wl_is_the_inverse_of_get_wl():
    from oracle import oracle as orc
    from smol_amd import capi

    case = wl.CASES["fcc222-flip"]
    ora = orc.OracleMC(case.built["tab"], wl.config_for(case, [0], 3, ("frozen", 1, 1)))
    ora.set_state(np.tile(case.law.start.astype(np.int32), (3, 1)), np.arange(3, dtype=np.uint64), 0.0)
    rng = np.random.default_rng(5)
    want = dict(entropy=rng.random((3, ora.L)) + 1.0, histogram=rng.integers(0, 9, (3, ora.L)), occurrences=rng.integers(0, 9, (3, ora.L)),
                mean_features=rng.random((3, ora.L, ora.F)), mod_factor=np.array([0.5, 2.0 ** -64, 3.0]))
    ora.set_wl(**want)
    got = ora.get_wl()
    assert all(np.array_equal(got[k], v) for k, v in want.items())
    ora.set_wl(entropy=want["entropy"] + 1.0)  # None leaves alone
    got = ora.get_wl()
    assert np.array_equal(got["entropy"], want["entropy"] + 1.0) and np.array_equal(got["histogram"], want["histogram"])
    with pytest.raises(ValueError, match="mod_factor must be greater than 0"):
        ora.set_wl(entropy=want["entropy"], mod_factor=np.array([0.5, 0.0, 1.0]))
    assert np.array_equal(ora.get_wl()["entropy"], want["entropy"] + 1.0)  # (a refused call writes nothing)
    metro = orc.OracleMC(case.built["tab"], capi.make_config(3, capi.KERNEL_METROPOLIS, case.law.step))
    with pytest.raises(RuntimeError):
        metro.set_wl(mod_factor=np.ones(3))


@pytest.mark.parametrize("name", OWN)
def test_conditions_on_the_inputs(name):
    """Conditions, not measurements: see ``wl_law.conditions``; and the pooling cap at the device's R and the CPU
    tier's."""
    case = wl.CASES[name]
    print(f"[wl law] {name}: start quantile {case.law.start_quantile} bins {case.law.windows[0].L} {wl.conditions(case)}")
    wl.assert_pooling_cap(case, case.R)
    wl.assert_pooling_cap(case, wl.host_R(case))


@pytest.mark.parametrize("name", OWN)
def test_power(name):
    """From the law alone: at the case's R every defect the case detects at the cap is detected with probability >= 0.99
    by one of its statistics."""
    case = wl.CASES[name]
    R, power, beyond = wl.choose_R(case)
    states = len(case.law.structure(None)["states"])
    print(f"[wl law] {name}: R=2^{int(np.log2(case.R))} (power alone 2^{int(np.log2(R))}) states={states} "
          f"pooled={wl.pooled_mass(case, case.R):.4f} "
          + " ".join(f"{d}={p:.3f}@{k[0]}/n{k[2]}/p{k[3]}" for d, (p, k) in sorted(power.items()))
          + (f" | not detected at 2^{int(np.log2(case.r_cap))}: {beyond}" if beyond else ""))
    assert wl.R_MIN <= R <= case.R <= case.r_cap and case.r_cap * case.law.G <= wl.R_CAP
    at_R = wl.power_of(case, case.R)
    assert all(at_R[d][0] >= 0.99 for d in power if d not in beyond), at_R


def test_every_defect_is_detected_by_some_case():
    """A defect no case detects at its R would have to be named in the docstring of tests/wl_law.py."""
    best = {}
    for case in wl.CASES.values():
        if case.twin:
            continue
        for d, (p, key) in wl.power_of(case, case.R).items():
            if p > best.get(d, (0.0,))[0]:
                best[d] = (p, case.name, key)
    print("[wl law] best detection per defect:", best)
    assert set(best) == set(wl.DEFECTS)
    assert all(v[0] >= 0.99 for v in best.values()), best


@pytest.mark.parametrize("name", [c.name for c in wl.CASES.values() if not c.twin and max(c.ns) > 2])
def test_the_frozen_law_is_stationary_under_exp_minus_entropy(name):
    law = wl.CASES[name].law
    assert law.depth is None
    for g in range(law.G):
        assert law.stationary_residual(g) < 1e-12
        for n in (1, 64):
            e = law.expected(g, n)
            assert abs(e.p.sum() - 1.0) < 1e-12 and e.p.min() >= 0.0


def _judge(case, run, samples, record_property, where):
    tier, n, period = run
    bad = []
    for g, s in enumerate(samples):
        key = (tier, g, n, period)
        res = wl.evaluate(case.expected(key), s)
        record_property(f"wl_law_{case.name}_{tier}_g{g}_n{n}_p{period}", wl.report(case, key, res, where))
        if not wl.passes(res, wl.ALPHA):
            bad.append((g, res))
    assert not bad, bad


@pytest.mark.parametrize("name,tier,n,period", HOST)
def test_oracle_chain_follows_its_law(name, tier, n, period, record_property):
    """(the per-walker identities are asserted inside ``wl_law.run_handle``)"""
    case = wl.CASES[name]
    _judge(case, (tier, n, period), wl.oracle_samples(name, (tier, n, period)), record_property, "oracle")


@pytest.mark.parametrize("defect", wl.DEFECTS)
def test_a_defect_in_the_expected_law_fails_a_case(defect):
    """Each defect as a mutation of the EXPECTED distribution only, against the counts sampled above: at least one
    law must fail."""
    failed = []
    for name, tier, n, period in HOST:
        case = wl.CASES[name]
        for g, s in enumerate(wl.oracle_samples(name, (tier, n, period))):
            key = (tier, g, n, period)
            if defect in case.applicable(key) and not wl.passes(wl.evaluate(case.expected(key, defect), s), wl.ALPHA):
                failed.append((name,) + key)
    print(f"[wl law] {defect}: {len(failed)} laws fail, first {failed[:6]}")
    assert failed, defect
