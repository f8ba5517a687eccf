"""CPU-side checks of the distance-objective boundary (smolmc_create_distance) and the SQS generator's host
logic: ctypes mirror, exported symbols, diameter groups, the exact-match diameter and argument validation."""

import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle as orc
from smol_amd import capi, engine, synth
from smol_amd import sqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fcc():
    return synth.build_cluster_model(synth.fcc_prim(), {2: 7.0, 3: 5.0})


def test_distance_struct_layout_matches_header():
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "smolmc.h"
    int main(){printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(smolmc_distance),
      offsetof(smolmc_distance, target), offsetof(smolmc_distance, match_weight),
      offsetof(smolmc_distance, n_groups), offsetof(smolmc_distance, group_diameter),
      offsetof(smolmc_distance, feature_group), offsetof(smolmc_distance, kB), SMOLMC_DIST_MAX_FEATURES);return 0;}
    """
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        vals = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    D = capi.smolmc_distance
    assert vals == [ctypes.sizeof(D), D.target.offset, D.match_weight.offset, D.n_groups.offset,
                    D.group_diameter.offset, D.feature_group.offset, D.kB.offset, capi.DIST_MAX_FEATURES]


def test_distance_symbols_exported():
    for name in ("smolmc_create_distance", "smolmc_get_best", "smolmc_reset_best"):
        assert name in engine.SYMBOLS
    if os.path.exists(engine.LIB_PATH):
        lib = ctypes.CDLL(engine.LIB_PATH)
        for name in ("smolmc_create_distance", "smolmc_get_best", "smolmc_reset_best"):
            assert hasattr(lib, name)


def test_diameter_groups_fcc(fcc):
    """Groups ascending; the NN pair at a / sqrt(2) shares its group with the NN triangle (same diameter)."""
    a = 4.09
    groups = sqs.orbits_by_diameter(fcc)
    diams = list(groups)
    assert diams == sorted(diams) and diams[0] == 0.0
    assert diams[1] == pytest.approx(a / np.sqrt(2), abs=1e-6)
    assert sorted(len(o.base) for o in groups[diams[1]]) == [2, 3]
    gd, fg = sqs.diameter_groups(fcc, capi.FEATURES_CORRELATIONS)
    assert fg[0] == -1 and np.all(fg[1:] >= 0) and len(fg) == fcc.num_corr_functions
    gdi, fgi = sqs.diameter_groups(fcc, capi.FEATURES_INTERACTIONS)
    assert np.array_equal(gd, gdi) and len(fgi) == fcc.num_orbits


def test_exact_match_max_diameter_cases(fcc):
    gd, fg = sqs.diameter_groups(fcc, capi.FEATURES_CORRELATIONS)
    d = np.zeros(len(fg))
    assert sqs.exact_match_max_diameter(d, gd, fg, 1e-5) == pytest.approx(gd[-1])
    d[1] = 1.0  # point term unmatched: nothing is matched
    assert sqs.exact_match_max_diameter(d, gd, fg, 1e-5) == 0.0
    d[:] = 0.0
    d[np.flatnonzero(fg == 2)[0]] = 1e-5  # at the tolerance: matched (<=)
    assert sqs.exact_match_max_diameter(d, gd, fg, 1e-5) == pytest.approx(gd[-1])
    d[np.flatnonzero(fg == 2)[0]] = 2e-5  # third group unmatched: L = diameter of the second
    assert sqs.exact_match_max_diameter(d, gd, fg, 1e-5) == pytest.approx(gd[1])


def test_distance_vector_from_oracle(fcc):
    """The L10 structure against its own correlations: every feature matched, L = the largest diameter."""
    sc, tab = sqs.distance_tables(fcc, np.diag([4, 4, 4]), capi.FEATURES_CORRELATIONS)
    oe = orc.OracleEvaluator(tab)
    z = sc.lattice_points[sc.site_t][:, 2]
    l10 = (z % 2).astype(np.int32)
    f = oe.correlations(l10)
    spec = sqs.distance_spec(fcc, capi.FEATURES_CORRELATIONS, f)
    d = np.abs(oe.correlations(l10) - spec.target)
    assert sqs.exact_match_max_diameter(d, spec.group_diameter, spec.feature_group, 1e-5) == pytest.approx(
        spec.group_diameter[-1])


def test_distance_spec_errors(fcc):
    """distance.py:75-87 (test_processor.py:402-420)."""
    with pytest.raises(ValueError, match="match weight"):
        sqs.distance_spec(fcc, capi.FEATURES_CORRELATIONS, match_weight=-1.0)
    with pytest.raises(ValueError, match="target_weights"):
        sqs.distance_spec(fcc, capi.FEATURES_CORRELATIONS, target_weights=np.ones(3))
    spec = sqs.distance_spec(fcc, capi.FEATURES_CORRELATIONS)
    assert np.array_equal(spec.target, np.zeros(fcc.num_corr_functions))
    assert np.array_equal(spec.weights, np.ones(fcc.num_corr_functions - 1))
    assert spec.struct.n_features == fcc.num_corr_functions and spec.struct.kB == 1.0


def test_generator_argument_validation(fcc):
    m = np.diag([4, 4, 4])
    with pytest.raises(ValueError, match="feature_type"):
        sqs.StochasticSQSGenerator(fcc, 64, feature_type="energy", supercell_matrices=[m])
    with pytest.raises(ValueError, match="supercell_matrices"):
        sqs.StochasticSQSGenerator(fcc, 64)
    with pytest.raises(ValueError, match="size"):
        sqs.StochasticSQSGenerator(fcc, 32, supercell_matrices=[m])
    with pytest.raises(ValueError, match="step_type"):
        sqs.StochasticSQSGenerator(fcc, 64, supercell_matrices=[m], step_type="table")
    gen = sqs.StochasticSQSGenerator(fcc, 64, supercell_matrices=[m], nwalkers=2)
    with pytest.raises(RuntimeError, match="generate"):
        gen.get_best_sqs()
    occ = sqs.random_ordered_occupancy(gen._cells[0][0], np.random.default_rng(0))
    assert np.array_equal(np.bincount(occ), [32, 32])
