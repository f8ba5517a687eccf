"""The float32 accept pre-test of the lean kernels with the Metropolis threshold a hair from the exact energy change on
every tested step (tests/fast_band.py): at the default band every such decision must be the oracle's; with the band
scaled down (SMOLMC_FAST_EPS_SCALE = 1, 1/2, ... 2^-20) some scale must show a wrong one, or the construction never
reaches the float32 error.  The kernel family is asserted from ``kernel_info``; the wrong decisions per scale go into
the junit record and are printed."""

import functools

import numpy as np
import pytest

from tests import fast_band as fb

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle_rows(name, chunks=(32, 32, 32)):
    """The oracle's state after every chunk of construction B's launch."""
    return fb.oracle_rows(fb.CASES[name], fb.construction_b(name), chunks)


@functools.lru_cache(maxsize=None)
def _oracle_state(kind, name):
    case = fb.CASES[fb.CASES[name].twin or name]
    if kind == "B":
        return _oracle_rows(name)[-1]
    return fb.oracle_run(case, fb.construction_a(name))


@pytest.mark.parametrize("name", fb.RUNS["A"])
def test_one_step_at_every_phase_of_the_batches(name, monkeypatch):
    """Construction A at the default band: accepted, n_accepted, occupancy equal the oracle's on every walker, and the
    decision of every adversarial walker is the one its hair implies."""
    case, con = fb.CASES[name], fb.construction_a(name)
    fb.clean_env(monkeypatch, case)
    st, info = fb.launch(case, con)
    print(f"[fast band] {name} A: {info}; adversarial {int(con.adversarial.sum())} of {len(con.occ)}")
    assert len(fb.residues(con)) == 64 and con.adversarial.sum() * 2 >= len(con.occ)
    assert fb.wrong_decisions(con, st) == 0
    fb.assert_parity(st, _oracle_state("A", name))


@pytest.mark.parametrize("name", fb.RUNS["B"])
def test_one_step_inside_a_launch(name, monkeypatch):
    """Construction B: 96 steps from a quenched state, the tested step up to 63 steps after its threshold was computed;
    then the same handle through run_sampled(3, 32), so that sample boundaries cut the batches."""
    case, con = fb.CASES[name], fb.construction_b(name)
    fb.clean_env(monkeypatch, case)
    want = _oracle_state("B", name)
    assert len(fb.residues(con)) >= 48 and con.adversarial.sum() * 2 >= len(con.occ)

    def sampled(eng):
        fb.set_up(eng, con)
        smp = eng.run_sampled(3, 32)
        return smp, eng.get_state()

    st, info, (smp, st2) = fb.launch(case, con, after=sampled)
    print(f"[fast band] {name} B: {info}; adversarial {int(con.adversarial.sum())} of {len(con.occ)}")
    fb.assert_parity(st, want)
    fb.assert_parity(st2, want)
    for i, row in enumerate(_oracle_rows(name)):
        assert np.array_equal(smp["occupancy"][i], row["occupancy"])
        assert np.array_equal(smp["accepted"][i], row["accepted"])
        np.testing.assert_allclose(smp["enthalpy"][i], row["enthalpy"], rtol=fb.RTOL, atol=fb.ATOL)


@pytest.mark.parametrize("name", fb.RUNS["C"])
def test_replay_with_every_step_adversarial(name, monkeypatch):
    case, con = fb.CASES[name], fb.construction_c(name)
    fb.clean_env(monkeypatch, case)
    acc, H, info = fb.launch_replay(case, con)
    print(f"[fast band] {name} C: {info}; adversarial {int(con['adversarial'].sum())} of {con['adversarial'].size}")
    assert con["adversarial"].sum() * 2 >= con["adversarial"].size
    assert np.array_equal(acc, con["accepted"]), int(np.sum(acc != con["accepted"]))
    np.testing.assert_allclose(H, con["H"], rtol=fb.RTOL, atol=fb.ATOL)


def _judge_sweep(name, kind, counts, record_property):
    line = fb.sweep_line(name, kind, counts)
    print(line)
    record_property(f"fast_band_{name}_{kind}", line)
    assert counts[1.0][0] == 0, line  # the band as shipped decides every adversarial step as the float64 rule does
    assert fb.margin(counts) is not None, "no scale of the sweep shows a wrong decision: " + line


@pytest.mark.parametrize("name", fb.RUNS["A"])
def test_band_scale_sweep_one_step(name, monkeypatch, record_property):
    """Teeth: the same one-step construction with the band scaled by 1, 1/2, ... 2^-20, a fresh handle per scale."""
    case = fb.CASES[name]
    counts = fb.sweep_a(name, lambda scale: fb.clean_env(monkeypatch, case, scale))
    _judge_sweep(name, "A", counts, record_property)


@pytest.mark.parametrize("name", fb.RUNS["C"])
def test_band_scale_sweep_replay(name, monkeypatch, record_property):
    case = fb.CASES[name]
    counts = fb.sweep_c(name, lambda scale: fb.clean_env(monkeypatch, case, scale))
    _judge_sweep(name, "C", counts, record_property)


# ---- Wang-Landau: the float32 bin pre-test of mc_wl.h with the proposed enthalpy 1e-8 bin from an edge -------------------
# (no band-scale sweep here: the pre-test's tolerance in bins is WL_RESYNC_FRAC at every scale of the band, so a sweep
# has no wrong bin to find -- tests/fast_band.py says what these runs hold instead)
def _wl_env(monkeypatch):
    from tests.test_gpu_wl_windows import ENV

    for v in ENV + fb.cl.DISPATCH_SWITCHES:
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("b", fb.WL_BINS)
@pytest.mark.parametrize("k", fb.WL_KS)
def test_wang_landau_bin_edges_per_walker_windows(k, b, monkeypatch):
    """R = 1024 walkers with their own windows; the last step of the k-step launch proposes an enthalpy 1e-8 bin from an
    interior edge (half), the upper end (a quarter), the lower end (a quarter): histogram, occurrences, n_accepted and
    the occupancy equal the float64 floor-division reference entry for entry."""
    _wl_env(monkeypatch)
    con = fb.wl_construction(k, b)
    assert con["adversarial"].sum() * 2 >= len(con["chain"])
    st, wl, info = fb.wl_launch(con, per_walker=True)
    print(f"[fast band] wang-landau k={k} bin={b}: {info}; adversarial {int(con['adversarial'].sum())} of {len(con['chain'])}")
    assert info.startswith("lean ") and " wl=v3" in info and "wl_windows=1" in info, info
    fb.wl_assert(con, st, wl)


@pytest.mark.parametrize("i", range(len(fb.WL_WIDE)))
def test_wang_landau_bin_edges_handle_window(i, monkeypatch):
    """The instantiation without per-walker windows: 64 copies of one chain, the handle's window tuned to its step k."""
    _wl_env(monkeypatch)
    con = fb.wl_wide_construction(i)
    st, wl, info = fb.wl_launch(con, per_walker=False)
    assert info.startswith("lean ") and " wl=v3" in info and "wl_windows" not in info, info
    fb.wl_assert(con, st, wl)


@pytest.mark.parametrize("name", list(fb.WL_SWEEPS))
def test_wang_landau_band_scale_sweep(name, monkeypatch, record_property):
    """The band-scale sweep on both instantiations (k = 200, 0.011 eV bins), recorded and printed.  Asserted: no wrong row
    at scale 1.  NOT asserted, unlike the Metropolis sweeps: a wrong row at some smaller scale.  The pre-test works
    against tolb = tol0 + resync_after * e1b with resync_after = (WL_RESYNC_FRAC - tol0) / e1b (mc_wl.h), which is
    WL_RESYNC_FRAC = 0.005 bin whatever SMOLMC_FAST_EPS_SCALE is: the scale only moves how often the enthalpy is rebuilt.
    An enthalpy 1e-8 bin from an edge therefore takes the exact path at every scale, and the float32 error carried over
    200 accepted steps (about 1e-7 eV each) stays far below 0.005 bin = 5.5e-5 eV.  Measured on the MI355X: 0 wrong rows
    at all 21 scales in both instantiations (profiles/fast_band_margin.jsonl).  A sweep with teeth needs a build with a
    small WL_RESYNC_FRAC (NOTES.md)."""
    def set_env(scale):
        _wl_env(monkeypatch)
        monkeypatch.setenv("SMOLMC_FAST_EPS_SCALE", repr(float(scale)))

    counts = fb.sweep_wl(name, set_env)
    line = fb.sweep_line(name, "WL", counts)
    print(line)
    record_property(f"fast_band_{name}", line)
    assert counts[1.0][0] == 0, line
