"""CPU checks of the distance objective against the reference's own compiled distance evaluators
(tests/golden/distance_v1.npz, made by tests/golden/make_distance_golden.py), the distance processors'
host logic (smol's test_processor.py:373-420) and orbit diameters of models loaded through smol_amd.mson."""

import os

import numpy as np
import pytest

from oracle import oracle as orc
from smol_amd import capi, moca, mson, synth
from smol_amd import sqs

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "distance_v1.npz"))

CASES = {
    "binary444": (lambda: synth.fcc_prim(), {2: 7.0, 3: 5.0}, np.diag([4, 4, 4])),
    "binary222": (lambda: synth.fcc_prim(), {2: 7.0, 3: 5.0}, np.diag([2, 2, 2])),
    "ternary333": (lambda: synth.fcc_prim(nspecies=3), {2: 6.0, 3: 4.5, 4: 4.2}, np.diag([3, 3, 3])),
    "rocksalt333": (lambda: synth.rocksalt_prim(anion_charges=(-2.0, -1.0)), {2: 4.5, 3: 3.2}, np.diag([3, 3, 3])),
}


def golden_case(name, mode):
    prim, cut, mat = CASES[name]
    model = synth.build_cluster_model(prim(), cut)
    sc, tab = sqs.distance_tables(model, mat, mode)
    return model, sc, tab


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("mode", [capi.FEATURES_CORRELATIONS, capi.FEATURES_INTERACTIONS])
def test_reference_distance_rows(name, mode):
    """corr_/interaction_distances_from_occupancies of the reference = |oracle features - target|, entry 0 = 0;
    the exact-match diameters of the fixture = sqs.exact_match_max_diameter."""
    model, sc, tab = golden_case(name, mode)
    oe = orc.OracleEvaluator(tab)
    key = "corr" if mode == capi.FEATURES_CORRELATIONS else "int"
    t = G[f"{name}/target_{key}"]
    rows, L = G[f"{name}/dist_{key}"], G[f"{name}/L_{key}"]
    gd, fg = sqs.diameter_groups(model, mode)
    tol = float(G[f"{name}/match_tol"])
    for i, (oi, of) in enumerate(zip(G[f"{name}/occ_i"], G[f"{name}/occ_f"])):
        for j, o in enumerate((oi, of)):
            f = oe.correlations(o) if mode == capi.FEATURES_CORRELATIONS else oe.interactions(o)
            want = np.abs(f - t)
            want[0] = 0.0
            np.testing.assert_allclose(rows[i, j], want, rtol=0, atol=1e-12)
            assert sqs.exact_match_max_diameter(rows[i, j], gd, fg, tol) == pytest.approx(L[i, j], abs=1e-12)
    assert L.max() > 0  # the ordered row matches its own target: the L branch is exercised


@pytest.fixture(scope="module")
def fcc_sc():
    model = synth.build_cluster_model(synth.fcc_prim(), {2: 7.0, 3: 5.0})
    return model, synth.build_supercell(model, np.diag([3, 3, 3]))


@pytest.mark.parametrize("cls", [moca.CorrelationDistanceProcessor, moca.ClusterInteractionDistanceProcessor])
def test_exact_match_max_diameter_reference_cases(cls, fcc_sc):
    """test_processor.py:373-399."""
    model, sc = fcc_sc
    rng = np.random.default_rng(0)
    proc = cls(sc)
    groups = sqs.orbits_by_diameter(model)
    d = np.zeros(len(proc.coefs))
    assert proc.exact_match_max_diameter(d) == max(groups)
    diameter = rng.choice(list(groups)[2:])
    orbit = groups[diameter][rng.integers(len(groups[diameter]))]
    index = (rng.choice(range(orbit.bit_id, orbit.bit_id + len(orbit.bit_combos)))
             if cls is moca.CorrelationDistanceProcessor else orbit.id)
    d[index] = 2 * proc.match_tol
    assert 0 < proc.exact_match_max_diameter(d) < diameter
    d[1] = 2 * proc.match_tol
    assert proc.exact_match_max_diameter(d) == 0.0


def test_bad_distance_processor(fcc_sc):
    """test_processor.py:402-420 (the external term: a model loaded with its EwaldTerm)."""
    model, sc = fcc_sc
    ce = mson.load_mson(os.path.join(HERE, "golden", "lno_ce_ewald.mson.json.gz"))
    with pytest.raises(ValueError):
        moca.CorrelationDistanceProcessor(ce.subspace, 3 * np.eye(3, dtype=int))
    with pytest.raises(ValueError):
        moca.CorrelationDistanceProcessor(model, 3 * np.eye(3, dtype=int), match_weight=-1)
    with pytest.raises(ValueError):
        moca.CorrelationDistanceProcessor(model, 3 * np.eye(3, dtype=int),
                                          target_weights=np.ones(model.num_corr_functions - 4))
    with pytest.raises(ValueError, match="chemical potentials"):
        moca.Ensemble(moca.CorrelationDistanceProcessor(sc), chemical_potentials={"A": 0.0, "B": 0.0})


def test_processor_defaults(fcc_sc):
    model, sc = fcc_sc
    p = moca.CorrelationDistanceProcessor(sc, match_weight=2.0, match_tol=1e-6)
    assert np.array_equal(p.target_vector, np.zeros(model.num_corr_functions))
    assert np.array_equal(p.coefs, np.concatenate([[-2.0], np.ones(model.num_corr_functions - 1)]))
    assert p.match_tol == 1e-6
    q = moca.ClusterInteractionDistanceProcessor(model, np.diag([3, 3, 3]))
    assert len(q.coefs) == model.num_orbits and q.size == 27
    assert np.array_equal(moca.Ensemble(p).natural_parameters, p.coefs)


def test_mson_orbit_diameters_and_generator():
    """MsonOrbit.diameter = largest pairwise Cartesian distance of the base cluster; groups ascending; the SQS
    generator accepts a model loaded through mson."""
    ce = mson.load_mson(os.path.join(HERE, "golden", "lno_ce.mson.json.gz"))
    sub = ce.subspace
    for orb in sub.orbits:
        cart = orb.frac_coords @ sub.lattice
        want = max((np.linalg.norm(a - b) for a in cart for b in cart), default=0.0)
        assert orb.diameter == pytest.approx(want, abs=1e-12)
    groups = sqs.orbits_by_diameter(sub)
    assert list(groups) == sorted(groups) and list(groups)[0] == 0.0
    pairs = [o for o in sub.orbits if o.num_sites == 2]
    assert all(o.diameter > 0 for o in pairs) and all(o.diameter == 0 for o in sub.orbits if o.num_sites == 1)
    gen = sqs.StochasticSQSGenerator(ce, 8, supercell_matrices=[np.diag([2, 2, 2])], nwalkers=4)
    assert gen.spec.struct.n_features == sub.num_corr_functions
    sc = gen._cells[0][0]
    occ = sqs.random_ordered_occupancy(sc, np.random.default_rng(0))
    assert len(occ) == sc.num_sites and sqs._translations(sc).shape == (sc.size, sc.num_sites)


def test_mson_fcc_nn_pair_diameter():
    """An fcc prim through the mson path: the NN pair sits at a / sqrt(2)."""
    a = 4.09
    lat = 0.5 * a * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=float)
    orb = mson.MsonOrbit({"sites": [[0, 0, 0], [1, 0, 0]], "bits": [[0], [0]], "structure_symops": [],
                          "site_bases": [{"func_array": [[1, 1], [1, -1]]}] * 2, "_bit_combos": [[[0, 0]]]},
                         2, 2, lat)
    assert orb.diameter == pytest.approx(a / np.sqrt(2), abs=1e-12)
