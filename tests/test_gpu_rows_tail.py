"""The tail of the step of the straight rows swap kernels (mc_lean.h: STRAIGHT; lean_rows_n2.hip): the thresholds of
the float32 pre-test are read as scalars from lane l64 at the head of the step and the decision is bit 63 of two
compares against the wave sum in lane 63, and the bookkeeping of the NEXT step (its address, its lane mask, the lane
indices l4 / l64 and the chunk counter) may be issued before this step has ended.  What that can break is at the edges of
a chunk: the last step of a chunk must not use lane indices of a batch that does not exist yet, the first must read its
thresholds from the lane the chunk starts at, and the exact path must still take log(u) from lane l64.  So the runs here
are split into launches of 1, 1, 13, 1, 15, 16, 17, 47, 1, 62, 1, 1, 64, 65 and then 13, 1, 1 steps (chunks then end
and begin at l4 = 0, 4, 56, 60 and l64 = 0, 62, 63) and compared after EVERY launch; the same split with every step on the exact
path (SMOLMC_FAST_EPS_SCALE = 0 / 1e9) and from near-pure and pure starts (the cold proposal region and the empty step
on the last step of a chunk); and sampled runs whose sample rows cut the chunks every 1, 3, 16, 17 and 100 steps.

Comparison of tests/test_gpu_rows_straight.py: n_accepted and occupancies EQUAL to the CPU oracle and to the same handle
under SMOLMC_NO_SOLO_ROWS=1; enthalpy purely relative 1e-10; features rtol 1e-10 / atol 1e-8."""

import numpy as np
import pytest

from smol_amd import capi
from tests.test_gpu_solo_rows import _clean, _engine, _same_chain, _tables

pytestmark = pytest.mark.gpu

SHAPES = [("fcc_prim666_triplets", 21), ("fcc_conv444_pairs", 11)]
# (the last three launches begin and end at l64 = 62 and 63: the 305 steps before them only END a chunk at 63)
SPLIT = (1, 1, 13, 1, 15, 16, 17, 47, 1, 62, 1, 1, 64, 65) + (13, 1, 1)
R = 64


def _edges(split):
    """(l4, l64) at which the chunks of consecutive launches from step 0 begin and (of their last step) end"""
    begin, end, s = set(), set(), 0
    for n in split:
        t = s
        while t < s + n:  # chunks end at the 16-step batch and at the launch
            u = min(s + n, (t | 15) + 1)
            begin.add(((t & 15) * 4, t & 63))
            end.add((((u - 1) & 15) * 4, (u - 1) & 63))
            t = u
        s += n
    return begin, end


def test_the_split_reaches_the_chunk_edges_it_is_meant_to():
    begin, end = _edges(SPLIT)
    for edge in (begin, end):
        assert {0, 4, 56, 60} <= {l4 for l4, _ in edge}
        assert {0, 62, 63} <= {l64 for _, l64 in edge}


def _pair(tab, cfg, shape, monkeypatch):
    """the rows handle and the same handle under SMOLMC_NO_SOLO_ROWS=1"""
    rows = _engine(tab, cfg)
    assert "solo=1" in rows.kernel_info() and f" rows={shape}" in rows.kernel_info(), rows.kernel_info()
    monkeypatch.setenv("SMOLMC_NO_SOLO_ROWS", "1")
    plain = _engine(tab, cfg)
    assert "rows=" not in plain.kernel_info().split(" env=")[0], plain.kernel_info()
    monkeypatch.delenv("SMOLMC_NO_SOLO_ROWS")
    return rows, plain


def _random_start(c, seed):
    rng = np.random.default_rng(seed)
    occ0 = (rng.random((R, c["sc"].num_sites)) < 0.5).astype(np.int32)
    return occ0, np.arange(1, R + 1, dtype=np.uint64) * np.uint64(104729)


def _near_pure_start(c, seed):
    """walker r: all sites of one species (alternating with r) except 1, 2 or 0 random sites of the other"""
    rng = np.random.default_rng(seed)
    n = c["sc"].num_sites
    occ0 = np.zeros((R, n), np.int32)
    for r in range(R):
        occ0[r] = r & 1
        occ0[r, rng.choice(n, (1, 2, 0)[r % 3], replace=False)] = 1 - (r & 1)
    return occ0, np.arange(R, dtype=np.uint64) * np.uint64(97) + np.uint64(5)


def _split_against_the_oracle(name, shape, occ0, seeds, temps, monkeypatch, what):
    from oracle import oracle as orc

    c, tab = _tables(name, False)
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP)
    rows, plain = _pair(tab, cfg, shape, monkeypatch)
    ora = orc.OracleMC(tab, cfg)
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


@pytest.mark.parametrize("name,shape", SHAPES)
def test_split_launches(name, shape, monkeypatch):
    _clean(monkeypatch)
    c, _ = _tables(name, False)
    occ0, seeds = _random_start(c, 23)
    a = _split_against_the_oracle(name, shape, occ0, seeds, np.linspace(500.0, 5000.0, R), monkeypatch, "split launches")
    assert 0 < a["n_accepted"].sum() < a["n_steps"].sum()


@pytest.mark.parametrize("scale", ["0", "1e9"], ids=["always-exact-0", "always-exact-1e9"])
@pytest.mark.parametrize("name,shape", SHAPES)
def test_split_launches_on_the_exact_path(name, shape, scale, monkeypatch):
    _clean(monkeypatch)
    monkeypatch.setenv("SMOLMC_FAST_EPS_SCALE", scale)
    c, _ = _tables(name, False)
    occ0, seeds = _random_start(c, 17)
    # from almost-always-reject to almost-always-accept
    a = _split_against_the_oracle(name, shape, occ0, seeds, np.geomspace(30.0, 30000.0, R), monkeypatch,
                                  f"split launches, eps scale {scale}")
    assert 0 < a["n_accepted"].sum() < a["n_steps"].sum()


@pytest.mark.parametrize("name,shape", SHAPES)
def test_split_launches_from_near_pure_and_pure_starts(name, shape, monkeypatch):
    _clean(monkeypatch)
    c, _ = _tables(name, False)
    occ0, seeds = _near_pure_start(c, 11)
    a = _split_against_the_oracle(name, shape, occ0, seeds, np.linspace(800.0, 6000.0, R), monkeypatch,
                                  "split launches, near-pure starts")
    pure = np.arange(R) % 3 == 2
    # every step of a pure walker is empty; the reference accepts an empty step (tests/test_gpu_rows_straight.py)
    assert np.array_equal(a["occupancy"][pure], occ0[pure]) and np.all(a["n_accepted"][pure] == sum(SPLIT))
    assert np.all(a["n_accepted"][np.arange(R) % 3 == 0] > 0)  # one minority site: moving it costs nothing


@pytest.mark.parametrize("thin", [1, 3, 16, 17, 100])
@pytest.mark.parametrize("name,shape", SHAPES)
def test_sampled_runs_cut_the_chunks(name, shape, thin, monkeypatch):
    from oracle import oracle as orc

    _clean(monkeypatch)
    c, tab = _tables(name, False)
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP)
    rows, plain = _pair(tab, cfg, shape, monkeypatch)
    ora = orc.OracleMC(tab, cfg)
    occ0, seeds = _random_start(c, 29)
    occ0[:6] = _near_pure_start(c, 30)[0][:6]  # (cold proposals on sample rows too)
    temps = np.linspace(500.0, 5000.0, R)
    for e in (rows, plain, ora):
        e.set_state(occ0, seeds, temps)
    ns = 200 // thin
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
