"""The cases of tests/ewald_size_cases.py on the CPU oracle alone: every cell still has the group count and tail its case
was chosen for (a change to smol_amd.synth cannot silently move a case off its edge), and every walker of every case
accepts more than 60 of its 201 steps -- the condition under which the device test's sweeps run at all, checked here
before any GPU time is spent."""

import numpy as np
import pytest

from tests import ewald_size_cases as ec


@pytest.mark.parametrize("name", list(ec.CELLS))
def test_cell_has_the_group_count_it_was_chosen_for(name):
    cell = ec.CELLS[name]
    sc = ec.cell_tables(name)[0]
    na = ec.changeable_sites(sc)
    assert (na, na >> 6, na & 63) == (cell.na, cell.groups, cell.tail)
    assert na == int(np.prod(cell.dims)) * (2 if cell.two else 1)


def test_cases_sit_on_the_edges_they_name():
    g = {c.name: ec.CELLS[c.cell] for c in ec.CASES}
    assert g["360-flip"].groups < 9 and 4 < g["360-flip"].groups < 8 and g["360-flip"].tail  # small path, two rounds, masked
    assert g["640-swap-rows"].groups < 14 and g["640-swap-rows"].tail == 0                   # dense U = 14 below its batch
    assert g["1716-flip"].groups == 26 and g["1716-flip"].tail                               # last size below the 27-batch
    assert g["1792-flip"].groups == 28 and g["1792-flip"].tail == 0                          # pre27 + shifted 27-batch
    assert g["1890-flip"].groups > 27 and g["1890-flip"].tail                                # ... and a ragged tail
    assert g["1920-flip-hbm"].na < 2048 <= g["2048-flip-hbm"].na == 2048                     # pending list off / on
    assert g["1024-flip-wl"].na == 1024 and g["1008-flip-wl"].na != 1024                     # the 16-group register sweep
    # (no affordable cell crosses a chunk boundary beyond 36 groups: those are the probe's, tests/test_gpu_ewald_sweeps.py)
    assert max(c.groups for c in g.values()) < 36


@pytest.mark.parametrize("name", ec.CASE_IDS)
def test_oracle_chain_accepts_enough_steps(name):
    from oracle import oracle as orc

    case = ec.CASES[ec.CASE_IDS.index(name)]
    tab, cfg, occ, seeds, temp = ec.setup(case)
    ora = orc.OracleMC(tab, cfg)
    ora.set_state(occ, seeds, temp)
    ora.run(ec.NSTEPS)
    st = ora.get_state()
    assert np.all(st["n_steps"] == ec.NSTEPS)
    assert st["n_accepted"].min() > ec.MIN_ACCEPTED, st["n_accepted"]
    if case.step == ec.TABLE:  # charge neutral throughout: Li+ / Mn3+ / Ti4+ against O2-
        P = ec.cell_tables(case.cell)[0].size
        assert np.all(np.array([1, 3, 4])[st["occupancy"][:, :P]].sum(axis=1) == 2 * P)
