"""The CPU oracle's Flip / Swap Metropolis chains against their exact transition law (tests/chain_law.py), and the
properties of the law itself that need no chain: the power of every case at the walker count the device runs, the
pooling cap, detailed balance.  The oracle runs 2^16 walkers per state point (more where the pooling cap needs it);
one tiny-cell case runs at the full R of the device test, which compares its histogram with the device's."""

import numpy as np
import pytest

from tests import chain_law as cl

HOST = cl.HOST_RUNS
oracle_samples, host_R = cl.oracle_samples, cl.host_R


def test_the_statistics_are_counted():
    """three per (case, state point, n) and module"""
    n = 3 * sum(cl.CASES[name].law.G for name, _ in HOST) + 3 * sum(cl.CASES[name].law.G for name, _ in cl.DEVICE_RUNS)
    assert n == cl.N_STATISTICS and cl.ALPHA == cl.FAMILY_ALPHA / n


@pytest.mark.parametrize("name", [c.name for c in cl.CASES.values() if not c.twin])
def test_power_and_pooling_cap(name):
    """From the law alone: at the case's R every defect the case can detect at all is detected with probability
    >= 0.99 by one of its statistics, and the pooled cell holds at most 5 % of the mass (at the device's R and at
    the CPU tier's)."""
    case = cl.CASES[name]
    R, power, beyond = cl.choose_R(case)
    print(f"[chain law] {name}: R=2^{int(np.log2(case.R))} (power alone 2^{int(np.log2(R))}) "
          + " ".join(f"{d}={p:.3f}" for d, p in sorted(power.items())) + (f" | not detected at 2^21: {beyond}" if beyond else ""))
    assert cl.R_MIN <= R <= cl.R_CAP
    at_R = cl.power_of(case, case.R)
    if case.R >= R:
        assert all(at_R[d] >= 0.99 for d in power if d not in beyond), at_R
    else:  # the Sampler's case, capped at 2^16 walkers: what it does detect there; beta x 1.02 is left to its direct twin
        assert name == "fcc222-swap-sampler" and case.R == case.r_cap
        assert {d for d, p in at_R.items() if p >= 0.99} == {"last-site-never", "partner-any-site"}, at_R
    cl.assert_pooling_cap(case, case.R)
    if case.host:
        cl.assert_pooling_cap(case, host_R(case))


def test_every_defect_is_detected_by_some_case():
    """A defect no case detects at its R would have to be named in the docstring of tests/chain_law.py."""
    best = {}
    for case in cl.CASES.values():
        if case.twin or case.R < cl.choose_R(case)[0]:
            continue
        for d, p in cl.power_of(case, case.R).items():
            if p > best.get(d, (0.0, None))[0]:
                best[d] = (p, case.name)
    print("[chain law] best detection per defect:", best)
    assert set(best) == set(cl.DEFECTS)
    assert all(p >= 0.99 for p, _ in best.values()), best


@pytest.mark.parametrize("name", [c.name for c in cl.CASES.values() if not c.twin and max(c.ns) > 2])
def test_the_law_is_stationary_under_boltzmann(name):
    law = cl.CASES[name].law
    assert law.depth is None
    for g in range(law.G):
        assert law.stationary_residual(g) < 1e-12
        for n in (1, 64):  # ... and a law is a distribution
            e = law.expected(g, n)
            assert abs(e.p.sum() - 1.0) < 1e-12 and e.p.min() >= 0.0


@pytest.mark.parametrize("name,n", HOST)
def test_oracle_chain_follows_its_law(name, n, record_property):
    case = cl.CASES[name]
    samples = oracle_samples(name, n)
    bad = []
    for g, s in enumerate(samples):
        res = cl.evaluate(case.law.expected(g, n), s)
        record_property(f"chain_law_{name}_g{g}_n{n}", cl.report(case, g, n, res, "oracle"))
        if not cl.passes(res, cl.ALPHA):
            bad.append((g, res))
    assert not bad, bad


def test_empty_and_zero_energy_steps_count_as_accepted():
    """metropolis.py:41-48: exponent 0 >= 0 is accepted, the empty step of Swap (mcusher.py:197-199) included: with
    one species only the occupancy never changes and every step is accepted; with all-zero coefficients the accepted
    count equals the number of steps exactly."""
    for name in ("fcc444-swap-one-species", "fcc444-swap-zero", "fcc444-flip-zero", "fcc333-swap-zero", "fcc444-swap-skewed-zero"):
        case = cl.CASES[name]
        for n in case.ns:
            for s in oracle_samples(name, n):
                assert np.all(s.nacc == n), (name, n)
                if "one-species" in name:
                    assert len(s.counts) == 1 and np.array_equal(s.rows[0], case.law.start)


@pytest.mark.parametrize("defect", cl.DEFECTS)
def test_a_defect_in_the_expected_law_fails_a_case(defect):
    """Each defect as a mutation of the EXPECTED distribution only, against the counts sampled above: at least one
    case must fail."""
    failed = []
    for name, n in HOST:
        case = cl.CASES[name]
        if defect not in case.law.applicable(n):
            continue
        for g, s in enumerate(oracle_samples(name, n)):
            if not cl.passes(cl.evaluate(case.law.expected(g, n, defect), s), cl.ALPHA):
                failed.append((name, n, g))
    print(f"[chain law] {defect}: {len(failed)} laws fail, first {failed[:6]}")
    assert failed, defect
