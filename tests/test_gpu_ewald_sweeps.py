"""The Ewald potential-field sweeps of smolmc_common.h, each instantiation the kernels call, at EVERY size switch: one probe
launch (smol_amd/csrc/probe_sweeps.hip, test-only) sweeps ~1000 slices of phi whose lengths na run through every value up to
768 and every group count up to 82 with tails of 0, 1 and 63 entries, on phi in global memory and on phi staged in LDS,
against the plain NumPy reference of tests/ewald_sweeps.py.

    data set   comparison
    exact      bit equality (dyadic inputs: float64 is exact in any order); no update is zero, so an entry skipped or
               updated twice always differs
    real       |err| <= NF 2^-52 (|phi| + sum_f |dq_f G|), derived in tests/ewald_sweeps.py, reference in long double

Branches reached here and by no engine test of affordable size: every chunk boundary beyond 36 groups (two chunks of
4 x 9 = 72 groups, three batches of 27 = 81), every shifted last batch at every overlap, the small masked path at each
ragged length, field_sweep_gx_pre27's tail call at every group count from 27 on, the four-flip batches of four of the pending
flush, and the dense-row batches of 9 / 14 / 6 / 4 at every size.  A failure names the variant, na, the first wrong entry
and its group."""

import functools

import pytest

from tests import ewald_sweeps as es

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=2)
def _case(variant, kind):
    """Built once for the two memory flavours of a (variant, data set) pair; the inputs are never written."""
    case = es.make_case(variant, kind)
    if kind == "exact":
        es.check_exact_budget(case)
    return case


@pytest.mark.parametrize("where", ["global", "lds"])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("variant", range(len(es.VARIANTS)), ids=es.VARIANT_NAMES)
def test_sweep_variant_on_the_ladder(variant, kind, where):
    case = _case(variant, kind)
    got = es.run_on_device(case, where == "lds")
    msg = es.first_mismatch(case, got, f"phi in {'LDS' if where == 'lds' else 'global memory'}, ")
    assert msg is None, msg
