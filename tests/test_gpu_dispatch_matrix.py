"""The reduced dispatch matrix on the device: one case per cell (tests/dispatch_matrix.py: CASES), on the release
library and on the bounds library (device-side traps at the gathers of mc_lean.h, mc_wl.h and mc_dist.h).

Per case: (a) the kernel predicted from kernel_info() and the case's own facts is the cell the case was written for;
(b) the native stream, (c) the Wang-Landau estimators -- per-walker windows and chemical potentials against one
one-walker oracle per walker -- and (d) the replay of the oracle's own trajectory equal the CPU oracle: occupancies and
counters bit for bit, enthalpies and features at the suite's RTOL 1e-10 / ATOL 1e-9 (features atol 1e-8), the final
features equal to eval_full of the final occupancy; (e) the variant's own term is live (dispatch_matrix.liveness).
The oracle's side of a case is computed once and shared by both libraries (dispatch_matrix.reference)."""

import os

import pytest

from smol_amd import codeobj, engine
from tests import dispatch_matrix as dm

pytestmark = pytest.mark.gpu

LIBS = ["release", "bounds"]


@pytest.fixture(params=LIBS)
def lib(request, monkeypatch):
    path = engine.LIB_PATH if request.param == "release" else os.path.join(
        os.path.dirname(engine.LIB_PATH), "libsmolmc_hip_bounds.so")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: build() makes both libraries")
    monkeypatch.setattr(engine, "_LIB", None)
    monkeypatch.setattr(engine, "LIB_PATH", path)
    yield path
    engine._LIB = None


@pytest.mark.parametrize("case", dm.CASES, ids=[c.id for c in dm.CASES])
def test_cell_runs_its_kernel_and_follows_the_oracle(case, lib):
    info, symbol = dm.run_case(case, engine.Engine)
    assert symbol in codeobj.kernel_digests(lib), (info, symbol)
    assert dm.show(dm.coords(symbol)) == dm.TARGETS[case.id], (info, symbol)
