"""The universal kernel at every switch of its LDS layout (tests/univ_layout.py: the rules restated, and the cases):
shadow copies of the feature cells 8 / 4 / 2 / 1 and none, dictionaries in LDS and dropped for each reason, occupancy in
LDS and in HBM, 4 / 2 / 1 waves per workgroup, workgroups above 64 KiB up to the largest a CU holds, the window where the
dictionaries give way to the occupancy, the three outcomes of the crowded shrink, and the dense instantiations.

Per case: kernel_info() names the layout the restated rules give for the same tables; the chain equals the CPU oracle's
(tests/test_gpu_universal.py: _same_chain -- occupancy, accept counts and flags bit for bit, enthalpy and features at
rtol 1e-10 / atol 1e-8) over launches of 1, 16 and 40 steps, every walker compared; the final features equal eval_full
of the final occupancy.  The feature-cell classes also run one sampled block and one Wang-Landau handle: both read the
features through the accepted-step cells.

The release library only: the bounds build traps the gathers of mc_lean.h and mc_dist.h and adds nothing to mc_univ.h
-- its 32 instantiations are the release library's byte for byte (tests/test_univ_layout_host.py asserts it) -- and the
layout is host code shared by both."""

import numpy as np
import pytest

from smol_amd import capi, codeobj, engine
from tests import dispatch_matrix as dm
from tests import univ_layout as ul
from tests.test_gpu_universal import _pair, _same_chain

pytestmark = pytest.mark.gpu
CHUNKS = (1, 16, 40)
STEPS = {"flip": capi.STEP_FLIP, "swap": capi.STEP_SWAP, "table": capi.STEP_TABLE_FLIP}


@pytest.fixture
def case(request, monkeypatch):
    c = ul.BY_NAME[request.param]
    for name in ("SMOLMC_FORCE_GENERAL", ul.FORCE, ul.HBM):
        monkeypatch.delenv(name, raising=False)
    for name in c.env:
        monkeypatch.setenv(name, "1")
    return c


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _expect_layout(c, eng, tab):
    """kernel_info() against the restated rules on the same tables; returns the layout."""
    args = ul.args_of(tab, c.R, occ_hbm_env=ul.HBM in c.env)
    assert args == c.args, "the case table's pinned arguments are not what the tables give"
    L, info = ul.layout(**args), eng.kernel_info()
    print(c.name, "->", info)
    assert info.startswith("universal occ=" + ("lds" if L.occ_lds else "hbm")), info
    assert ul.info_words(info) == L.words(_cus()), (info, L)
    symbol = dm.predict(info, dm.Facts(STEPS[c.step]))
    assert symbol == L.symbol(_cus()) and symbol in codeobj.kernel_digests(engine.LIB_PATH), (info, symbol)
    return L


@pytest.mark.parametrize("case", ul.CASE_IDS, indirect=True)
def test_chain_at_the_layout(case):
    c = case
    _, tab = ul.tables_of(c.name)
    occ, seeds, temps = ul.start_state(c.name)
    eng, ora = _pair(tab, capi.make_config(c.R, capi.KERNEL_METROPOLIS, STEPS[c.step]), occ, seeds, temps)
    try:
        L = _expect_layout(c, eng, tab)
        for key, want in c.want.items():
            assert {"lds": L.total}.get(key, getattr(L, key, None)) == want, (key, L)
        a = _same_chain(eng, ora, CHUNKS)
        np.testing.assert_allclose(a["features"], eng.eval_full(a["occupancy"]), rtol=1e-10, atol=1e-8)
        assert 0 < a["n_accepted"].sum() < a["n_steps"].sum()
        assert (a["occupancy"] != occ).any(axis=1).sum() > c.R // 2  # the accepted steps changed most walkers
    finally:
        eng.close()


EXTRA = [c.name for c in ul.CASES if c.extra]


@pytest.mark.parametrize("case", EXTRA, indirect=True)
def test_samples_read_the_accepted_step_cells(case):
    """Thinned samples taken inside one launch: their features are the walker's features plus the cells of the steps
    accepted so far in this launch."""
    c = case
    _, tab = ul.tables_of(c.name)
    occ, seeds, temps = ul.start_state(c.name)
    eng, ora = _pair(tab, capi.make_config(c.R, capi.KERNEL_METROPOLIS, STEPS[c.step]), occ, seeds, temps)
    try:
        _expect_layout(c, eng, tab)
        smp = eng.run_sampled(5, 9)
        moved = 0
        for i in range(5):
            ora.run(9)
            b = ora.get_state()
            assert np.array_equal(smp["occupancy"][i], b["occupancy"])
            assert np.array_equal(smp["accepted"][i], b["accepted"])
            np.testing.assert_allclose(smp["enthalpy"][i], b["enthalpy"], rtol=1e-10, atol=1e-8)
            np.testing.assert_allclose(smp["features"][i], b["features"], rtol=1e-10, atol=1e-8)
            moved += int((b["occupancy"] != occ).any())
        assert moved >= 4  # steps were accepted before most samples
    finally:
        eng.close()


@pytest.mark.parametrize("case", EXTRA, indirect=True)
def test_wang_landau_reads_the_accepted_step_cells(case):
    """The per-bin feature means of a Wang-Landau handle are updated after every step from features + cells."""
    from oracle import oracle as orc

    c = case
    _, tab = ul.tables_of(c.name)
    occ, seeds, _ = ul.start_state(c.name)
    ev = orc.OracleEvaluator(tab)
    h = np.array([ev.natural_parameters() @ ev.feature_vector(o) for o in occ])
    cfg = capi.make_config(c.R, capi.KERNEL_WANGLANDAU, STEPS[c.step], min_enthalpy=float(h.min()) - 20.37,
                           max_enthalpy=float(h.max()) + 20.11, bin_size=0.5, check_period=20)
    eng, ora = _pair(tab, cfg, occ, seeds, 0.0)
    try:
        _expect_layout(c, eng, tab)
        a = _same_chain(eng, ora, CHUNKS, wl=True)
        assert 0 < a["n_accepted"].sum()
    finally:
        eng.close()
