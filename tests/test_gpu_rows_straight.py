"""The straight-line step of the solo rows kernels (mc_lean.h: ROWS; lean_rows_n2.hip): the first proposal round
falls through to one take, rounds 1-3, the second-round fallback and its empty-step census sit in a cold region, the
decision is a select with the exact float64 path as its one unlikely branch, and the step loop is bottom-tested.  The
inputs here force what moved out of line: walkers with 1, 2, 4, 8, 27 and 108 minority sites (with one minority site of
216 the first round misses on ~98.6 % of the steps and all twelve candidates on ~94.6 %), pure walkers (every step
empty; the reference accepts an empty step, so their accept counter is the step count while the occupancy stays),
SMOLMC_FAST_EPS_SCALE = 0 / 1e9 (every step exact), run() lengths around the 16-step batch, the 64-step batch and
the chunk edges, and more walkers than four waves per SIMD hold (the OCC 6 instantiations).  The straight form is in
the swap kernels without chemical potentials at the default occupancy; the other cases run kernels in the parent's form.

Comparison of tests/test_gpu_solo_rows.py: n_accepted and occupancies EQUAL to the CPU oracle and to the same handle
under SMOLMC_NO_SOLO_ROWS=1; enthalpy purely relative 1e-10; features rtol 1e-10 / atol 1e-8 (the change reorders no
arithmetic)."""

import numpy as np
import pytest

from smol_amd import capi
from tests.test_gpu_solo_rows import _clean, _engine, _same_chain, _tables

pytestmark = pytest.mark.gpu

# (case, step, chemical potentials, rows shape)
SWAP21 = ("fcc_prim666_triplets", capi.STEP_SWAP, False, 21)
SWAP21_MU = ("fcc_prim666_triplets", capi.STEP_SWAP, True, 21)
SWAP11 = ("fcc_conv444_pairs", capi.STEP_SWAP, False, 11)
FLIP21_MU = ("fcc_prim666_triplets", capi.STEP_FLIP, True, 21)
MINORITY = (1, 2, 4, 8, 27, 108, 0)  # 0: a pure walker, every step is empty
KEYS = ("n_accepted", "occupancy", "enthalpy", "features")


def _minority_start(c, R, seed):
    """walker r: all sites of one species (alternating with r) except MINORITY[r % 7] random sites of the other"""
    rng = np.random.default_rng(seed)
    n = c["sc"].num_sites
    occ0 = np.zeros((R, n), np.int32)
    for r in range(R):
        occ0[r] = r & 1
        occ0[r, rng.choice(n, MINORITY[r % len(MINORITY)], replace=False)] = 1 - (r & 1)
    return occ0, np.arange(R, dtype=np.uint64) * np.uint64(97) + np.uint64(5)


def _random_start(c, R, seed):
    rng = np.random.default_rng(seed)
    occ0 = (rng.random((R, c["sc"].num_sites)) < 0.5).astype(np.int32)
    return occ0, np.arange(1, R + 1, dtype=np.uint64) * np.uint64(104729)


def _pair(tab, cfg, shape, monkeypatch):
    """the rows handle and the same handle under SMOLMC_NO_SOLO_ROWS=1"""
    rows = _engine(tab, cfg)
    assert "solo=1" in rows.kernel_info() and f" rows={shape}" in rows.kernel_info(), rows.kernel_info()
    monkeypatch.setenv("SMOLMC_NO_SOLO_ROWS", "1")
    plain = _engine(tab, cfg)
    assert "rows=" not in plain.kernel_info().split(" env=")[0], plain.kernel_info()
    monkeypatch.delenv("SMOLMC_NO_SOLO_ROWS")
    return rows, plain


def _head(state, k):
    return {n: state[n][:k] for n in KEYS}


@pytest.mark.parametrize("name,step,with_mu,shape", [SWAP21, SWAP21_MU, SWAP11])
def test_cold_proposal_rounds_fallback_and_empty_steps(name, step, with_mu, shape, monkeypatch):
    from oracle import oracle as orc

    _clean(monkeypatch)
    c, tab = _tables(name, with_mu)
    R, steps = 64, 3000
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, step)
    rows, plain = _pair(tab, cfg, shape, monkeypatch)
    ora = orc.OracleMC(tab, cfg)
    occ0, seeds = _minority_start(c, R, 11)
    temps = np.linspace(800.0, 6000.0, R)
    for e in (rows, plain, ora):
        e.set_state(occ0, seeds, temps)
        e.run(steps)
    a, b, p = rows.get_state(), ora.get_state(), plain.get_state()
    assert np.all(a["n_steps"] == steps)
    _same_chain(a, b, f"{name} mu={with_mu} minority start, rows vs oracle")
    _same_chain(a, p, f"{name} mu={with_mu} minority start, rows vs plain solo")
    pure = np.arange(R) % len(MINORITY) == len(MINORITY) - 1
    assert pure.sum() >= 9
    # the empty-step exit of the fallback's census: nothing moved and the run ended.  The accept counter is the
    # oracle's (asserted equal above), which counts every empty step: its exponent is 0 and metropolis.py:46-48
    # accepts exponent >= 0 -- the counter of a pure walker is the number of steps, not 0
    assert np.array_equal(a["occupancy"][pure], occ0[pure])
    assert np.all(a["n_accepted"][pure] == steps) and np.all(b["n_accepted"][pure] == steps)
    # and the walkers with ONE minority site did move (every site is equivalent, so moving it costs nothing; their
    # proposals come from rounds 1-3 and the fallback)
    assert np.all(a["n_accepted"][np.arange(R) % len(MINORITY) == 0] > 0)


@pytest.mark.parametrize("scale", ["0", "3e3", "1e9"], ids=["always-exact-0", "wide-band", "always-exact-1e9"])
@pytest.mark.parametrize("name,step,with_mu,shape", [SWAP21, SWAP11, FLIP21_MU])
def test_exact_decision_path(name, step, with_mu, shape, scale, monkeypatch):
    from oracle import oracle as orc

    _clean(monkeypatch)
    monkeypatch.setenv("SMOLMC_FAST_EPS_SCALE", scale)
    c, tab = _tables(name, with_mu)
    R, steps = 64, 3000
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, step)
    rows, plain = _pair(tab, cfg, shape, monkeypatch)
    ora = orc.OracleMC(tab, cfg)
    occ0, seeds = _random_start(c, R, 17)
    temps = np.geomspace(30.0, 30000.0, R)  # from almost-always-reject to almost-always-accept
    for e in (rows, plain, ora):
        e.set_state(occ0, seeds, temps)
        e.run(steps)
    a = rows.get_state()
    assert 0 < a["n_accepted"].sum() < a["n_steps"].sum()
    _same_chain(a, ora.get_state(), f"{name} eps scale {scale}, rows vs oracle")
    _same_chain(a, plain.get_state(), f"{name} eps scale {scale}, rows vs plain solo")


@pytest.mark.parametrize("name,step,with_mu,shape", [SWAP21, SWAP11, FLIP21_MU])
def test_loop_boundaries(name, step, with_mu, shape, monkeypatch):
    """consecutive runs around the 16-step batch, the 64-step batch and the chunk edges against ONE oracle run"""
    from oracle import oracle as orc

    _clean(monkeypatch)
    c, tab = _tables(name, with_mu)
    R = 64
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, step)
    rows, plain = _pair(tab, cfg, shape, monkeypatch)
    ora = orc.OracleMC(tab, cfg)
    occ0, seeds = _random_start(c, R, 23)
    occ0[:7], _ = _minority_start(c, 7, 24)  # (cold proposals across the edges too)
    temps = np.linspace(500.0, 5000.0, R)
    for e in (rows, plain, ora):
        e.set_state(occ0, seeds, temps)
    chunks = (1, 15, 17, 63, 65, 1000)
    for n in chunks:
        rows.run(n)
        plain.run(n)
    ora.run(sum(chunks))
    a = rows.get_state()
    assert np.all(a["n_steps"] == sum(chunks))
    _same_chain(a, ora.get_state(), f"{name} runs of {chunks}, rows vs one oracle run")
    _same_chain(a, plain.get_state(), f"{name} runs of {chunks}, rows vs plain solo")


@pytest.mark.parametrize("with_mu", [False, True], ids=["plain", "mu"])
def test_six_waves_per_simd_with_the_minority_start(with_mu, monkeypatch):
    import torch
    from oracle import oracle as orc

    _clean(monkeypatch)
    c, tab = _tables("fcc_prim666_triplets", with_mu)
    R = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP)
    six = _engine(tab, cfg)
    assert "solo=1 occ=6 rows=21" in six.kernel_info(), six.kernel_info()
    monkeypatch.setenv("SMOLMC_NO_SOLO_ROWS", "1")
    plain = _engine(tab, cfg)
    assert "solo=1 occ=6" in plain.kernel_info() and "rows=" not in plain.kernel_info().split(" env=")[0]
    monkeypatch.delenv("SMOLMC_NO_SOLO_ROWS")
    occ0, seeds = _minority_start(c, R, 31)
    temps = np.linspace(800.0, 6000.0, R)
    k = 2 * len(MINORITY)
    ora = orc.OracleMC(tab, capi.make_config(k, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    ora.set_state(occ0[:k], seeds[:k], temps[:k])
    for e in (six, plain):
        e.set_state(occ0, seeds, temps)
    for chunk in (1, 63, 1500):
        for e in (six, plain, ora):
            e.run(chunk)
    a = six.get_state()
    _same_chain(a, plain.get_state(), f"occ=6 mu={with_mu} rows vs occ=6 plain")
    _same_chain(_head(a, k), ora.get_state(), f"occ=6 mu={with_mu} rows vs oracle")
    pure = np.arange(R) % len(MINORITY) == len(MINORITY) - 1
    assert np.array_equal(a["occupancy"][pure], occ0[pure]) and np.all(a["n_accepted"][pure] == 1 + 63 + 1500)
