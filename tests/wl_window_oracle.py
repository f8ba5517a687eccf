"""A walker with its own Wang-Landau window against an unmodified one-walker CPU oracle that was given the identical
(min, max, bin): the helpers shared by tests/test_gpu_wl_windows.py and the dispatch matrix (tests/dispatch_matrix.py)."""

import numpy as np

from smol_amd import capi


def top(vmin, L, bin_size):
    """vmin + L bins, an ulp lower where rounding would make the engine's ceil rule count L + 1."""
    vmax = vmin + L * bin_size
    while int(np.ceil((vmax - vmin) / bin_size)) > L:
        vmax = np.nextafter(vmax, -np.inf)
    assert int(np.ceil((vmax - vmin) / bin_size)) == L
    return vmax


def enthalpies(tab, occ):
    from oracle import oracle as orc

    ev = orc.OracleEvaluator(tab)
    nat = ev.natural_parameters()
    return np.array([ev.feature_vector(o) @ nat for o in occ])


def one_walker_oracle(tab, occ, seed, vmin, vmax, **kw):
    """An unmodified one-walker oracle with the window [vmin, vmax)."""
    from oracle import oracle as orc

    o = orc.OracleMC(tab, capi.make_config(1, capi.KERNEL_WANGLANDAU, min_enthalpy=float(vmin), max_enthalpy=float(vmax), **kw))
    o.set_state(np.asarray(occ).reshape(1, -1), np.array([seed], dtype=np.uint64), 0.0)
    return o


def same(eng_state, eng_wl, walker, estimator, ora):
    """Walker `walker` of the engine, which updates estimator `estimator`, against a one-walker oracle, as in
    test_wang_landau_bin_pretest_is_decision_neutral."""
    b, y = ora.get_state(), ora.get_wl()
    assert np.array_equal(eng_state["occupancy"][walker], b["occupancy"][0])
    assert eng_state["n_accepted"][walker] == b["n_accepted"][0] and eng_state["n_steps"][walker] == b["n_steps"][0]
    np.testing.assert_allclose(eng_state["enthalpy"][walker], b["enthalpy"][0], rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(eng_state["features"][walker], b["features"][0], rtol=1e-10, atol=1e-8)
    np.testing.assert_allclose(eng_wl["entropy"][estimator], y["entropy"][0], rtol=0, atol=0)
    assert np.array_equal(eng_wl["histogram"][estimator], y["histogram"][0])
    assert np.array_equal(eng_wl["occurrences"][estimator], y["occurrences"][0])
    np.testing.assert_allclose(eng_wl["mean_features"][estimator], y["mean_features"][0], rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(eng_wl["mod_factor"][estimator], y["mod_factor"][0])
