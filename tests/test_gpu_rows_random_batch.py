"""The random batch of the straight rows swap kernels (mc_lean.h: STRAIGHT; lean_rows_n2.hip): no 64-step batch any more.
The two float32 thresholds of a step come from lane 4k of the 16-step batch (rows_thresholds.h) and the exact path forms
log(u) from the two raw words of that lane only when it runs.
What that can break: a threshold or a word read from the wrong lane (the first and last step of a batch, the first step
of a launch that begins inside a batch, the lane index that runs one step ahead in the rows = 21 kernel).  So the chains
are run in launches of 1, 15, 16, 17, 47, 1, 63, 64, 65 and then 3 x 16 steps and compared after
EVERY launch with the CPU oracle and with the same handle under SMOLMC_NO_SOLO_ROWS=1 (which keeps the 64-step batch) --
at ordinary temperatures, at 300 K and at 40000 K (thresholds of both magnitudes), with every step on the exact path
(SMOLMC_FAST_EPS_SCALE=0: log(u) is then taken at every lane index), and through run_sampled cutting every 1, 16 and 17
steps.  Smallest shapes that reach the two kernels, 64 walkers, as tests/test_gpu_rows_tail.py (whose helpers these are).

n_accepted and occupancies EQUAL; enthalpy purely relative 1e-10 (features rtol 1e-10 / atol 1e-8)."""

import numpy as np
import pytest

from smol_amd import capi
from tests.test_gpu_rows_tail import R, SHAPES, _pair, _random_start
from tests.test_gpu_solo_rows import _clean, _same_chain, _tables

pytestmark = pytest.mark.gpu

SPLIT = (1, 15, 16, 17, 47, 1, 63, 64, 65) + (16, 16, 16)


def _split(name, shape, temps, monkeypatch, what, seed=41):
    from oracle import oracle as orc

    c, tab = _tables(name, False)
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP)
    rows, plain = _pair(tab, cfg, shape, monkeypatch)
    ora = orc.OracleMC(tab, cfg)
    occ0, seeds = _random_start(c, seed)
    for e in (rows, plain, ora):
        e.set_state(occ0, seeds, temps)
    done = 0
    for n in SPLIT:
        for e in (rows, plain, ora):
            e.run(n)
        done += n
        a, b = rows.get_state(), ora.get_state()
        assert np.all(a["n_steps"] == done)
        _same_chain(a, b, f"{name} {what}, rows vs oracle after +{n} = {done}")
        _same_chain(a, plain.get_state(), f"{name} {what}, rows vs plain solo after +{n} = {done}")
        assert np.array_equal(a["accepted"], b["accepted"]), (what, done)
    return rows.get_state()


def test_the_split_begins_and_ends_launches_at_the_batch_edges():
    begin, end, s = set(), set(), 0
    for n in SPLIT:
        begin.add(s & 15)
        end.add((s + n - 1) & 15)
        s += n
    # (launches begin at the first and second step of a batch and end at its first and last; every other lane index
    # is reached in mid-launch, and tests/test_gpu_rows_tail.py begins and ends launches at l4 = 4, 56, 60 as well)
    assert {0, 1} <= begin and {0, 15} <= end


@pytest.mark.parametrize("name,shape", SHAPES)
def test_split_launches(name, shape, monkeypatch):
    _clean(monkeypatch)
    a = _split(name, shape, np.linspace(500.0, 5000.0, R), monkeypatch, "split launches")
    assert 0 < a["n_accepted"].sum() < a["n_steps"].sum()


@pytest.mark.parametrize("T", [300.0, 40000.0])
@pytest.mark.parametrize("name,shape", SHAPES)
def test_split_launches_cold_and_hot(name, shape, T, monkeypatch):
    _clean(monkeypatch)
    a = _split(name, shape, np.full(R, T), monkeypatch, f"split launches at {T} K", seed=43)
    assert 0 < a["n_accepted"].sum() < a["n_steps"].sum()


@pytest.mark.parametrize("temps", ["ordinary", 300.0, 40000.0])
@pytest.mark.parametrize("name,shape", SHAPES)
def test_split_launches_with_every_step_on_the_exact_path(name, shape, temps, monkeypatch):
    _clean(monkeypatch)
    monkeypatch.setenv("SMOLMC_FAST_EPS_SCALE", "0")
    t = np.geomspace(30.0, 30000.0, R) if temps == "ordinary" else np.full(R, temps)
    a = _split(name, shape, t, monkeypatch, f"split launches, exact path, {temps}", seed=47)
    assert 0 < a["n_accepted"].sum() < a["n_steps"].sum()


@pytest.mark.parametrize("scale", [None, "0"], ids=["default-band", "exact-path"])
@pytest.mark.parametrize("thin", [1, 16, 17])
@pytest.mark.parametrize("name,shape", SHAPES)
def test_sampled_runs_cut_the_batches(name, shape, thin, scale, monkeypatch):
    from oracle import oracle as orc

    _clean(monkeypatch)
    if scale is not None:
        monkeypatch.setenv("SMOLMC_FAST_EPS_SCALE", scale)
    c, tab = _tables(name, False)
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP)
    rows, plain = _pair(tab, cfg, shape, monkeypatch)
    ora = orc.OracleMC(tab, cfg)
    occ0, seeds = _random_start(c, 53)
    temps = np.geomspace(300.0, 40000.0, R)
    for e in (rows, plain, ora):
        e.set_state(occ0, seeds, temps)
    ns = 136 // thin
    sa, sp = rows.run_sampled(ns, thin, occupancy=True), plain.run_sampled(ns, thin, occupancy=True)
    H, acc, occ = np.zeros((ns, R)), np.zeros((ns, R), bool), np.zeros((ns, R, occ0.shape[1]), np.int32)
    for k in range(ns):
        ora.run(thin)
        b = ora.get_state()
        H[k], acc[k], occ[k] = b["enthalpy"], b["accepted"], b["occupancy"]
    assert np.array_equal(sa["accepted"], acc) and np.array_equal(sa["accepted"], sp["accepted"])
    assert np.array_equal(sa["occupancy"], occ) and np.array_equal(sa["occupancy"], sp["occupancy"])
    m = np.abs(H) > 1e-6
    assert m.sum() >= H.size // 2
    worst = float(np.max(np.abs(sa["enthalpy"][m] - H[m]) / np.abs(H[m])))
    worst_p = float(np.max(np.abs(sa["enthalpy"][m] - sp["enthalpy"][m]) / np.abs(H[m])))
    print(f"[{name} thin {thin}] max relative sample enthalpy difference: oracle {worst:.2e}, plain solo {worst_p:.2e}")
    assert worst < 1e-10 and worst_p < 1e-10, (worst, worst_p)
    _same_chain(rows.get_state(), ora.get_state(), f"{name} after {ns} samples every {thin}, rows vs oracle")
