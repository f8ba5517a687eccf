"""The solo rows variants of mc_lean_kernel (mc_lean.h: ROWS; lean_rows_n2.hip): per-slot gather widths, index rows
addressed by LDS address, the first site's species kept in its VGPR.  Same random stream, proposals and accept rule as
the plain solo kernel, so against the CPU oracle and against the same handle under SMOLMC_NO_SOLO_ROWS=1 the accept
counters and occupancies are EQUAL; the lane sums run over the same lanes (with fewer zero terms), enthalpies and
features are compared at the bounds of tests/test_gpu_fullsize.py (enthalpy 1e-10 purely relative; features
rtol 1e-10 / atol 1e-8)."""

import numpy as np
import pytest

from smol_amd import capi
from tests.cases import load_case, tables_for

pytestmark = pytest.mark.gpu

CASES = [("fcc_prim666_triplets", capi.STEP_SWAP, False, 21),
         ("fcc_prim666_triplets", capi.STEP_FLIP, True, 21),
         ("fcc_conv444_pairs", capi.STEP_SWAP, False, 11)]


def _engine(tab, cfg):
    from smol_amd.engine import Engine

    return Engine(tab, cfg)


def _tables(name, with_mu):
    c = load_case(name)
    mu = None
    if with_mu:
        mu = np.zeros((c["sc"].num_sites, 2))
        mu[:] = np.array([-0.3, 0.4])[None, :]
    return c, tables_for(name, capi.FEATURES_INTERACTIONS, mu_table=mu)


def _start(c, R, seed):
    rng = np.random.default_rng(seed)
    nsp = np.array([c["model"].prim.nspecies[b] for b in c["sc"].site_b])
    occ0 = (rng.random((R, c["sc"].num_sites)) * nsp).astype(np.int32)
    return occ0, np.arange(R, dtype=np.uint64) * np.uint64(31) + np.uint64(9)


def _same_chain(a, b, what):
    """accept counters and occupancies equal; enthalpy purely relative 1e-10, features rtol 1e-10 / atol 1e-8"""
    assert np.array_equal(a["n_accepted"], b["n_accepted"]), what
    assert np.array_equal(a["occupancy"], b["occupancy"]), what
    got, want = np.asarray(a["enthalpy"], float), np.asarray(b["enthalpy"], float)
    m = np.abs(want) > 1e-6
    assert m.sum() >= max(1, got.size // 2), what
    worst = float(np.max(np.abs(got[m] - want[m]) / np.abs(want[m])))
    fworst = float(np.max(np.abs(a["features"] - b["features"])))
    print(f"[{what}] max relative enthalpy difference {worst:.2e} over {int(m.sum())} walkers; max absolute feature difference {fworst:.2e}")
    assert worst < 1e-10, (what, worst)
    np.testing.assert_allclose(a["features"], b["features"], rtol=1e-10, atol=1e-8)


def _clean(monkeypatch):
    for v in ("SMOLMC_FORCE_GENERAL", "SMOLMC_NO_SOLO", "SMOLMC_NO_OCC6", "SMOLMC_NO_SOLO_ROWS"):
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("name,step,with_mu,shape", CASES)
def test_rows_variant_is_taken_and_follows_the_oracle(name, step, with_mu, shape, monkeypatch):
    from oracle import oracle as orc

    _clean(monkeypatch)
    c, tab = _tables(name, with_mu)
    R = 9
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, step)
    rows = _engine(tab, cfg)
    info = rows.kernel_info()
    assert "solo=1" in info and f" rows={shape}" in info, info
    monkeypatch.setenv("SMOLMC_NO_SOLO_ROWS", "1")
    plain = _engine(tab, cfg)
    assert "solo=1" in plain.kernel_info() and "rows=" not in plain.kernel_info().split(" env=")[0], plain.kernel_info()
    monkeypatch.delenv("SMOLMC_NO_SOLO_ROWS")
    ora = orc.OracleMC(tab, cfg)
    occ0, seeds = _start(c, R, 77)
    temps = np.linspace(600.0, 4000.0, R)
    for e in (rows, plain, ora):
        e.set_state(occ0, seeds, temps)
    for chunk in (1, 15, 16, 64, 65, 300, 2000):
        for e in (rows, plain, ora):
            e.run(chunk)
        a = rows.get_state()
        _same_chain(a, ora.get_state(), f"{name} rows vs oracle after +{chunk}")
        _same_chain(a, plain.get_state(), f"{name} rows vs plain solo after +{chunk}")
        assert np.array_equal(a["accepted"], ora.get_state()["accepted"])
    sa, sb = rows.run_sampled(5, 21, occupancy=True), plain.run_sampled(5, 21, occupancy=True)
    assert np.array_equal(sa["occupancy"], sb["occupancy"]) and np.array_equal(sa["accepted"], sb["accepted"])
    np.testing.assert_allclose(sa["enthalpy"], sb["enthalpy"], rtol=1e-10, atol=1e-9)


@pytest.mark.parametrize("name,step,with_mu,shape", CASES)
def test_same_handle_with_and_without_the_switch(name, step, with_mu, shape, monkeypatch):
    """64 walkers at three temperatures, 20 000 steps: a walker that differs is a bug unless it is shown to be a
    last-bit tie on the exact path."""
    _clean(monkeypatch)
    c, tab = _tables(name, with_mu)
    R = 64
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, step)
    rows = _engine(tab, cfg)
    assert f" rows={shape}" in rows.kernel_info(), rows.kernel_info()
    monkeypatch.setenv("SMOLMC_NO_SOLO_ROWS", "1")
    plain = _engine(tab, cfg)
    assert "rows=" not in plain.kernel_info().split(" env=")[0]
    occ0, seeds = _start(c, R, 5)
    temps = np.repeat(np.array([400.0, 1500.0, 6000.0]), [22, 21, 21])
    for e in (rows, plain):
        e.set_state(occ0, seeds, temps)
        e.run(20000)
    a, b = rows.get_state(), plain.get_state()
    assert np.all(a["n_steps"] == 20000) and a["n_accepted"].sum() > 0
    _same_chain(a, b, f"{name} rows vs plain solo, 20000 steps")


def test_more_walkers_than_four_waves_per_simd_reach_the_occ6_instantiation(monkeypatch):
    import torch
    from oracle import oracle as orc

    _clean(monkeypatch)
    c, tab = _tables("fcc_prim666_triplets", False)
    R = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP)
    six = _engine(tab, cfg)
    assert "solo=1 occ=6 rows=21" in six.kernel_info(), six.kernel_info()
    monkeypatch.setenv("SMOLMC_NO_SOLO_ROWS", "1")
    plain = _engine(tab, cfg)
    assert "solo=1 occ=6" in plain.kernel_info() and "rows=" not in plain.kernel_info().split(" env=")[0]
    occ0, seeds = _start(c, R, 78)
    temps = np.linspace(500.0, 5000.0, R)
    k = 8
    ora = orc.OracleMC(tab, capi.make_config(k, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    ora.set_state(occ0[:k], seeds[:k], temps[:k])
    for e in (six, plain):
        e.set_state(occ0, seeds, temps)
    for chunk in (1, 63, 400):
        for e in (six, plain, ora):
            e.run(chunk)
    a = six.get_state()
    _same_chain(a, plain.get_state(), "occ=6 rows vs occ=6 plain")
    _same_chain({n: a[n][:k] for n in ("n_accepted", "occupancy", "enthalpy", "features")}, ora.get_state(), "occ=6 rows vs oracle")
