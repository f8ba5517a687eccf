"""Engine chains on cells chosen for the group count of their Ewald potential field, against the CPU oracle on the same
Philox streams (the pattern of tests/test_gpu_fuzz.py::test_ewald_field_sweep_shapes_match_oracle; cases and cells in
tests/ewald_size_cases.py).  The oracle keeps no field: it sums the dense Ewald rows at every proposal, so a field entry
skipped, updated twice or written past na shows as an enthalpy off the oracle's, then as a different accept decision, and the
final features disagree with eval_full of the final occupancies.

Which test reaches which sweep branch (na = changeable sites = 64 groups + tail):

    branch of smolmc_common.h / its call site                          reached by
    ------------------------------------------------------------------------------------------------------------------
    small masked path between 4 and 8 groups with a ragged tail        360-flip, 360-swap (5 + 40)
    3-flip sweep off 8 / 36 / 1728 entries                             360-table (5 + 40), 1792-table (28 + 0)
    4-flip sweep (no step of this flip table has four flips)           2048-*-hbm (the pending flush); every size: the probe
    dense rows, U = 14 below its first batch                           640-swap-rows (10 + 0)
    last size below the 27-batch: shifted nine-batch + tail            1716-flip (26 + 52)
    field_sweep_gx_pre27's tail call, the shifted 27-batch             1792-flip (28 + 0), 1890-flip (29 + 34, ragged tail)
    dense rows at another size (SMOLMC_NO_EWALD_GX), U = 9 / 14        1792-flip-rows, 1792-swap-rows
    dense rows of the general kernel, U = 6 / 4                        1792-flip-general, 1792-swap-general
    field in HBM below / from the pending list's threshold             1920-*-hbm (off), 2048-*-hbm (on; the 1- and 40-step
                                                                       launches end with a partly filled list)
    16-group register sweep (Wang-Landau, field in LDS, na == 1024)    1024-flip-wl, 1024-swap-wl; 1008-*-wl beside it
    chunk boundaries beyond 36 groups, every other group count         tests/test_gpu_ewald_sweeps.py (the sweep probe)

Chunk boundaries beyond 36 groups need cells of 5000 sites or more with an 800 MB Ewald matrix: they are left to the probe,
which runs every instantiation on every group count up to 82.  Tolerances are the parity suite's (tests/test_gpu_parity.py)."""

import numpy as np
import pytest

from tests import ewald_size_cases as ec

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-9  # tests/test_gpu_parity.py


@pytest.mark.parametrize("name", ec.CASE_IDS)
def test_chain_on_a_cell_chosen_for_its_group_count(name, monkeypatch):
    from oracle import oracle as orc
    from smol_amd.engine import Engine

    case = ec.CASES[ec.CASE_IDS.index(name)]
    cell = ec.CELLS[case.cell]
    for k in ec.DISPATCH_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    tab, cfg, occ, seeds, temp = ec.setup(case)
    assert ec.changeable_sites(ec.cell_tables(case.cell)[0]) == cell.na == 64 * cell.groups + cell.tail
    eng, ora = Engine(tab, cfg), orc.OracleMC(tab, cfg)
    info = eng.kernel_info()
    # the words that prove the path: family, where the field lives, compressed tables (gx=) or dense rows (no gx=)
    assert info.startswith(case.starts), info
    assert all(w in info for w in case.has) and not any(w in info for w in case.hasnot), info
    if "gx=" in case.has:
        assert "gx=%dx%dx%dx%d" % ((2 if cell.two else 1,) + cell.dims) in info, info
    eng.set_state(occ, seeds, temp)
    ora.set_state(occ, seeds, temp)
    for chunk in ec.CHUNKS:
        eng.run(chunk)
        ora.run(chunk)
        a, b = eng.get_state(), ora.get_state()
        assert np.array_equal(a["occupancy"], b["occupancy"])
        assert np.array_equal(a["n_accepted"], b["n_accepted"])
        assert np.array_equal(a["n_steps"], b["n_steps"])
        assert np.array_equal(a["accepted"], b["accepted"])
        np.testing.assert_allclose(a["enthalpy"], b["enthalpy"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(a["features"], b["features"], rtol=RTOL, atol=1e-8)
        if case.kernel == "wang-landau":
            x, y = eng.get_wl(), ora.get_wl()
            assert np.array_equal(x["histogram"], y["histogram"])
            assert np.array_equal(x["occurrences"], y["occurrences"])
            np.testing.assert_allclose(x["entropy"], y["entropy"], rtol=0, atol=0)
            np.testing.assert_allclose(x["mean_features"], y["mean_features"], rtol=RTOL, atol=1e-8)
    assert a["n_accepted"].min() > ec.MIN_ACCEPTED, a["n_accepted"]  # the sweeps ran
    # the field itself has not drifted: running Ewald term == from-scratch evaluation
    np.testing.assert_allclose(a["features"], eng.eval_full(a["occupancy"]), rtol=RTOL, atol=1e-8)
    eng.close()
