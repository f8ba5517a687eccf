"""The adversarial constructions of tests/fast_band.py against the CPU oracle alone: the oracle's own decision at the
tested step follows the sign of the hair on every adversarial walker and flips with it, at least half the walkers
are adversarial, the tested steps cover the lanes of the threshold batch, and the exact dH agrees with the
from-scratch difference on 16 walkers per construction."""

import numpy as np
import pytest

from smol_amd import capi
from tests import fast_band as fb


def _follows_the_hair(case, con):
    acc, before = fb.oracle_decisions(case, con)
    adv = con.adversarial
    assert adv.sum() * 2 >= len(adv), (case.name, int(adv.sum()), len(adv))
    assert np.all(before[adv] == 0)  # (every earlier step of the launch was rejected)
    assert np.array_equal(acc[adv], con.sign[adv] > 0), int(np.sum(acc[adv] != (con.sign[adv] > 0)))
    assert (con.sign[adv] > 0).any() and (con.sign[adv] < 0).any()
    return acc


@pytest.mark.parametrize("name", [n for n in fb.RUNS["A"] if not fb.CASES[n].twin])
def test_construction_a_decides_by_the_hair(name):
    case = fb.CASES[name]
    con = fb.construction_a(name)
    assert len(con.checked) == 16
    assert len(fb.residues(con)) == 64
    assert np.all(fb.HAIR * con.A[con.adversarial] < 2.0 ** -14 * con.dH[con.adversarial])  # (the hair is a hair)
    acc = _follows_the_hair(case, con)
    flipped = con.flipped()
    acc2 = _follows_the_hair(case, flipped)
    assert np.array_equal(acc2[con.adversarial], ~acc[con.adversarial])
    if "big" in case.built:  # the walkers with the large chemical potentials are among the adversarial ones
        big = np.arange(len(con.occ)) % 8 == 3
        assert (con.adversarial & big).sum() * 2 >= big.sum()
    st = fb.oracle_run(case, con)  # the one-step launch as the device test runs it
    assert np.array_equal(st["accepted"], acc)
    assert fb.wrong_decisions(con, st) == 0


@pytest.mark.parametrize("name", fb.RUNS["B"])
def test_construction_b_decides_by_the_hair(name):
    case = fb.CASES[name]
    con = fb.construction_b(name)
    assert len(con.checked) == 16
    assert len(fb.residues(con)) >= 48
    acc = _follows_the_hair(case, con)
    acc2 = _follows_the_hair(case, con.flipped())
    assert np.array_equal(acc2[con.adversarial], ~acc[con.adversarial])


@pytest.mark.parametrize("name", fb.RUNS["C"])
def test_construction_c_replays_to_the_host_signs(name):
    from oracle import oracle as orc

    case = fb.CASES[name]
    con = fb.construction_c(name)
    assert con["checked"] == 16
    assert con["adversarial"].sum() * 2 >= con["adversarial"].size
    ora = orc.OracleMC(case.tab, capi.make_config(len(con["occ"]), capi.KERNEL_METROPOLIS, case.step))
    acc, H = fb.replay(case, ora, con)
    assert np.array_equal(acc, con["accepted"]), int(np.sum(acc != con["accepted"]))
    np.testing.assert_allclose(H, con["H"], rtol=fb.RTOL, atol=fb.ATOL)
    probe = con["probe"]  # the one-step probes of the sweep: the same decisions from the states the chain passed
    assert probe["adversarial"].sum() * 2 >= len(probe["occ"])
    accp, _ = fb.replay(case, ora, probe)
    assert np.array_equal(accp, probe["accepted"])
    # the signs flipped: the host's chain is again the oracle's, and the first adversarial step of every walker (same
    # state, same proposal) is decided the other way
    con2 = fb.construction_c(name, flip=True)
    acc2, _ = fb.replay(case, ora, con2)
    assert np.array_equal(acc2, con2["accepted"])
    rows = np.flatnonzero(con["adversarial"].any(axis=1))
    first = np.argmax(con["adversarial"], axis=1)[rows]
    assert np.array_equal(con["steps"][rows, first], con2["steps"][rows, first])
    assert np.all(con2["adversarial"][rows, first])
    assert np.all(acc2[rows, first] != acc[rows, first])


# ---- Wang-Landau: the reference bins of the window constructions against per-walker oracles ---------------------------
def _wl_oracle_agrees(con, rows):
    from oracle import oracle as orc

    vmin, vmax = np.broadcast_to(con["vmin"], len(con["chain"])), np.broadcast_to(con["vmax"], len(con["chain"]))
    exp = con["expected"]
    for r in rows:
        ora = orc.OracleMC(fb.wl_tab(), fb.wl_config(1, vmin[r], vmax[r], con["bin"]))
        assert ora.L == con["L"]
        ora.set_state(con["occ0"][r:r + 1], con["seeds"][r:r + 1], 0.0)
        ora.run(con["k"])
        st, wl = ora.get_state(), ora.get_wl()
        assert np.array_equal(wl["histogram"][0], exp["histogram"][r]), (r, con["kind"][r], con["sign"][r])
        assert np.array_equal(wl["occurrences"][0], exp["histogram"][r])
        assert int(st["n_accepted"][0]) == exp["n_accepted"][r] and np.array_equal(st["occupancy"][0], exp["occupancy"][r])
        assert np.all(wl["entropy"][0] <= con["k"] * fb.WL_MOD)  # (no entropy difference can reach log u)


def _wl_hair_decides(con):
    """On the adversarial walkers the hair's sign decides: the side of the window end, or of the bin edge."""
    adv, kind, sign, exp = con["adversarial"], con["kind"], con["sign"], con["expected"]
    assert np.array_equal(exp["accepted_last"][adv & (kind == 1)], sign[adv & (kind == 1)] < 0)
    assert np.array_equal(exp["accepted_last"][adv & (kind == 2)], sign[adv & (kind == 2)] > 0)
    rows = np.flatnonzero(adv & (kind == 0))
    Hk = fb.wl_pool()["H"][con["chain"][rows], con["k"]]
    x = (Hk - np.broadcast_to(con["vmin"], len(adv))[rows]) / con["bin"]
    frac = x - np.floor_divide(Hk - np.broadcast_to(con["vmin"], len(adv))[rows], con["bin"])
    assert np.all(np.where(sign[rows] > 0, frac < 1e-7, frac > 1.0 - 1e-7))
    assert np.all(exp["accepted_last"][rows])


@pytest.mark.parametrize("b", fb.WL_BINS)
@pytest.mark.parametrize("k", fb.WL_KS)
def test_wang_landau_window_construction(k, b):
    con = fb.wl_construction(k, b)
    assert con["L"] >= 40 and con["adversarial"].sum() * 2 >= len(con["chain"])
    for q in range(3):  # both signs of every kind are among the adversarial walkers
        for s in (1.0, -1.0):
            assert np.any(con["adversarial"] & (con["kind"] == q) & (con["sign"] == s)), (q, s)
    _wl_hair_decides(con)
    _wl_oracle_agrees(con, range(16))


def test_wang_landau_handle_wide_constructions():
    for i in range(len(fb.WL_WIDE)):
        con = fb.wl_wide_construction(i)
        assert con["L"] >= 40
        _wl_hair_decides(con)
        _wl_oracle_agrees(con, [0])


def test_numpy_philox_is_the_oracles():
    seeds = [0, 1, 12345678901234, 2 ** 32 + 5, 2 ** 63 + 2 ** 40 + 17, 2 ** 64 - 1]
    steps = [0, 99, 2 ** 32 - 1, 2 ** 32, 2 ** 33 + 5, 2 ** 64 - 1]
    got = fb.uniforms_of(np.array(seeds, dtype=np.uint64)[:, None], np.array(steps, dtype=np.uint64)[None, :])
    want = np.array([[fb.uniform_of(s, t) for t in steps] for s in seeds])
    assert np.array_equal(got, want)
