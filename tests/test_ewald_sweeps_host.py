"""Host side of the sweep probe (tests/ewald_sweeps.py, smol_amd/libsmolmc_probe.so): the library exports its entry, the
ladder of na holds every size switch of the sweeps, and the exact data set meets the bit budget that makes its comparison
a bit equality.  The device run is tests/test_gpu_ewald_sweeps.py."""

import numpy as np
import pytest

from tests import ewald_sweeps as es


def test_probe_library_exports_its_entry():
    """Built by build() after the engine libraries; one variant per entry of VARIANTS; refuses what it cannot run before any
    launch (pre27 below 27 groups and the 16-group sweep off na = 1024 would read E8 entries that are not there)."""
    lib = es.load_probe()
    assert lib.smolmc_probe_variant_count() == len(es.VARIANTS) == 17
    assert lib.smolmc_probe_guard() == es.GUARD
    buf = np.zeros(4, dtype=np.float64)
    p = buf.ctypes.data
    pre27, g16 = es.VARIANT_NAMES.index("gx_pre27"), es.VARIANT_NAMES.index("gx_groups<1,16>")
    assert lib.smolmc_probe_sweep(pre27, 0, 1, 1727, 1728, p, p, p, p, p, p, None, None, p, p) == -3
    assert lib.smolmc_probe_sweep(g16, 0, 1, 1024, 1088, p, p, p, p, p, p, None, None, p, p) == -3
    assert lib.smolmc_probe_sweep(len(es.VARIANTS), 0, 1, 1, 1, p, p, p, p, p, p, None, None, p, p) == -1
    assert lib.smolmc_probe_sweep(0, 0, 1, 1, 1, p, p, p, p, None, None, None, None, p, p) == -2
    assert lib.smolmc_probe_sweep(0, 1, 1, 1, 8192, p, p, p, p, p, p, None, None, p, p) == -4


def test_probe_is_not_part_of_the_engine():
    """The probe is its own library: the engine libraries are made of the Makefile's OBJS, which do not name it."""
    import os
    import re

    with open(os.path.join(es.ROOT, "smol_amd", "csrc", "Makefile")) as fh:
        mk = fh.read()
    objs = re.findall(r"^[A-Z_]*OBJS\s*=.*$", mk, flags=re.M)
    assert objs and not any("probe" in line for line in objs)
    assert "../libsmolmc_probe.so: probe_sweeps.hip" in mk


def test_ladder_holds_every_size_switch():
    """U - 1, U, U + 1, 2U - 1, 2U, NB U, NB U + 1 groups for the batch sizes U = 4, 9, 14, 27 with the chunk sizes NB the
    kernels use them with (4 only with U = 9: chunk boundary at 36 groups) -- each with tails of 0, 1 and 63 entries; every
    na up to 768; 82 groups = three batches of 27 and two chunks of 4 x 9 with groups behind them."""
    full = es.ladder(0)
    have = set(full.tolist())
    assert set(range(1, 769)) <= have
    assert set(es.BATCHES) == {4, 9, 14, 27} and es.BATCHES[9] == (1, 4)
    for g in es.edge_groups():
        assert g <= es.MAX_GROUPS
        for t in (0, 1, 63):
            assert g * 64 + t in have, (g, t)
    for g in range(1, es.MAX_GROUPS + 1):
        assert {g * 64, g * 64 + 1, g * 64 + 63} <= have, g
    assert es.MAX_GROUPS > 3 * 27 and es.MAX_GROUPS > 2 * 4 * 9
    assert full.max() == es.MAX_GROUPS * 64 + 63 and 900 < len(full) < 1100
    assert len(set(full.tolist())) == len(full)
    for v, name in enumerate(es.VARIANT_NAMES):
        nas = es.ladder(v)
        if name == "gx_pre27":  # (the kernels take it from 27 groups on: mc_lean.h epre_on)
            assert nas.min() == 27 * 64 and set(nas.tolist()) == {n for n in have if n >= 27 * 64}
        elif name.startswith("gx_groups"):  # (mc_lean_multi.h: ew_nact == 1024 only)
            assert nas.tolist() == [1024]
        else:
            assert np.array_equal(nas, full)
    # the LDS flavour of the largest slice fits the default 64 KiB with its guard and the slack behind it
    assert (int(full.max()) + es.GUARD + es.PAD) * 8 <= 64 * 1024


@pytest.mark.parametrize("variant", range(len(es.VARIANTS)), ids=es.VARIANT_NAMES)
def test_exact_data_set_meets_its_bit_budget(variant):
    """In int64 units of 2^-24: every partial sum below 2^30, the float64 reference equal to the integer result, no update
    (nor twice it) zero -- so the device comparison can be bit equality, and a skipped or doubled entry always shows."""
    c = es.make_case(variant, "exact")
    worst = es.check_exact_budget(c)
    assert worst < 2 ** 30
    assert np.all(c.delta != 0.0) and np.all(2.0 * c.delta != 0.0)
    # the reference itself detects each defect it is meant to
    i = len(c.j) // 3
    for wrong in (c.phi0[c.pos_phi[i]], c.expected[c.pos_phi[i]] + c.delta[i]):
        got = c.expected.copy()
        got[c.pos_phi[i]] = wrong
        assert es.first_mismatch(c, got) is not None
    got = c.expected.copy()
    got[c.pos_phi[-1] + 1] += 1.0  # first guard entry of the last slice
    assert "guard entry" in es.first_mismatch(c, got)
    assert es.first_mismatch(c, c.expected.copy()) is None
    # padding: E8 / rows behind every slice are valid and lead to 2^30
    if c.compressed:
        pad = np.ones(c.tab_len, dtype=bool)
        pad[c.pos_tab] = False
        assert pad.sum() == len(c.nas) * es.PAD
        cells = c.E8[pad].astype(np.int64) // 8
        assert all(np.all(c.gx[cells + b] == es.BIG) for b in c.b)
        assert int(c.E8.max()) + int(c.s8.max()) + 8 <= c.gx.nbytes
    else:
        pad = np.ones(c.tab_len, dtype=bool)
        pad[c.pos_tab] = False
        assert np.all(c.ga[pad] == es.BIG) and np.all(c.gb[pad] == es.BIG)


def test_real_data_set_bound_is_the_derived_one():
    c = es.make_case(3, "real")  # gx_multi<2,1>
    S = np.abs(c.phi0[c.pos_phi]) + sum(np.abs(c.dq[f] * c.G[f]) for f in range(c.NF))
    np.testing.assert_allclose(np.asarray(c.bound, dtype=np.float64), c.NF * 2.0 ** -52 * S, rtol=1e-12)
    assert es.first_mismatch(c, c.expected.copy()) is None
    got = c.expected.copy()
    got[c.pos_phi[5]] += 4.0 * float(c.bound[5])
    assert es.first_mismatch(c, got) is not None
