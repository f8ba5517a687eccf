"""The device's Flip / Swap Metropolis chains against their exact transition law (tests/chain_law.py): every case at
the walker count its power calculation asks for, one launch per (case, n), the kernel family asserted from
``kernel_info``.  p-values, z-scores, R and degrees of freedom go into the junit record and are printed."""

import numpy as np
import pytest

from smol_amd import capi
from tests import chain_law as cl

pytestmark = pytest.mark.gpu

DEVICE = [(name, n) for name, n in cl.DEVICE_RUNS if name != "fcc222-swap-sampler"]


def _clean(monkeypatch, case):
    for v in cl.DISPATCH_SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


def _judge(case, n, samples, record_property, where="device"):
    bad = []
    for g, s in enumerate(samples):
        res = cl.evaluate(case.law.expected(g, n), s)
        record_property(f"chain_law_{case.name}_g{g}_n{n}", cl.report(case, g, n, res, where))
        if not cl.passes(res, cl.ALPHA):
            bad.append((g, res))
    assert not bad, bad


def _enthalpy_of_the_handle(case, eng, g, rows):
    """H of states as the handle prices them: eval_full @ natural_parameters, the chemical work (last feature) from
    the walker's own row where per-walker chemical potentials are set (eval_full keeps the create-time table)."""
    feat = eng.eval_full(rows.astype(np.int32))
    mu = case.built["mu_rows"]
    if mu is not None:
        feat[:, -1] = eng.chemical_work(rows.astype(np.int32), np.repeat(mu[g:g + 1], len(rows), axis=0))
    return feat @ eng.natural_parameters


@pytest.mark.parametrize("name,n", DEVICE)
def test_device_chain_follows_its_law(name, n, monkeypatch, record_property):
    from smol_amd.engine import Engine

    case = cl.CASES[name]
    _clean(monkeypatch, case)
    law, R = case.law, case.R
    cl.assert_pooling_cap(case, R)
    eng = Engine(case.built["tab"], capi.make_config(law.G * R, capi.KERNEL_METROPOLIS, law.step))
    try:
        st, samples = cl.run_handle(case, eng, R, n)
        info = eng.kernel_info()  # (after the launch: the per-walker rows are part of the dispatch)
        print(f"[chain law] {name}: {info}")
        assert case.family_ok(info), (case.want, case.wont, info)
        for g, s in enumerate(samples):  # the law's H is the handle's H, on the states the walkers ended in
            rows = s.rows[:8]
            want = np.array([law.enthalpy(g, r) for r in rows])
            np.testing.assert_allclose(_enthalpy_of_the_handle(case, eng, g, rows), want, rtol=1e-10, atol=1e-9)
    finally:
        eng.close()
    if (name, n) == cl.FULL_R:  # the case the CPU tier runs at this R: same seeds, so the same counts
        for a, b in zip(samples, cl.oracle_samples(name, n, R)):
            assert a.same_as(b)
    _judge(case, n, samples, record_property)


def test_sampler_sample_row_follows_the_law(monkeypatch, record_property):
    """moca.Sampler.from_ensemble(...).run(n, occ, thin_by=n) with one walker per draw: the single sample row is the
    outcome, so the device ring and the walker order are inside the check."""
    from smol_amd import moca

    case = cl.CASES["fcc222-swap-sampler"]
    _clean(monkeypatch, case)
    law, R, n = case.law, case.R, case.ns[0]
    cl.assert_pooling_cap(case, R)
    seeds = [int(s) for s in cl.seeds_for(case, R)]
    sampler = moca.Sampler.from_ensemble(case.built["ensemble"], temperature=float(law.temperatures[0]), step_type="swap",
                                         nwalkers=R, seeds=seeds)
    sampler.run(n, np.tile(law.start.astype(np.int32), (R, 1)), thin_by=n)
    assert case.family_ok(sampler.engine.kernel_info()), sampler.engine.kernel_info()
    c = sampler.samples
    assert c.num_samples == 1
    occ = c.get_occupancies(flat=False)[0]
    # (the sample row carries no accept counter; the law of n = 8 is over the final state alone)
    _judge(case, n, [cl.Sample(occ, np.zeros(R, dtype=np.int64), c.get_enthalpies(flat=False)[0, :, 0])], record_property,
           where="Sampler")
