"""Distance-objective handles (smolmc_create_distance) and the SQS generator on the GPU, on the release
library and on the bounds library (device-side traps at the new kernel's gathers).

References: the CPU oracle's full correlation / interaction vectors (the reference's
corr_distances_from_occupancies / interaction_distances_from_occupancies recompute them in full,
evaluator.pyx:319-437) turned into the distance vector of distance.py:133-182, and a numpy restatement of
the Metropolis chain that takes its proposals from OracleMC.propose and its uniform from the Philox stream."""

import os

import numpy as np
import pytest

from oracle import oracle as orc
from smol_amd import capi, engine, synth
from smol_amd import sqs as sqs_mod

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
    yield request.param
    engine._LIB = None


_MODELS = {}


def model_case(name):
    if name not in _MODELS:
        if name == "binary444":
            m = synth.build_cluster_model(synth.fcc_prim(), {2: 7.0, 3: 5.0})
            mat = np.diag([4, 4, 4])
        elif name == "binary222":  # aliased: clusters hold a site twice
            m = synth.build_cluster_model(synth.fcc_prim(), {2: 7.0, 3: 5.0})
            mat = np.diag([2, 2, 2])
        elif name == "rocksalt333":  # two active sublattices (cations, anions)
            m = synth.build_cluster_model(synth.rocksalt_prim(anion_charges=(-2.0, -1.0)), {2: 4.5, 3: 3.2})
            mat = np.diag([3, 3, 3])
        elif name == "ternary333":
            m = synth.build_cluster_model(synth.fcc_prim(nspecies=3), {2: 6.0, 3: 4.5, 4: 4.2})
            mat = np.diag([3, 3, 3])
        else:
            raise KeyError(name)
        _MODELS[name] = (m, mat)
    return _MODELS[name]


def setup(name, mode, step, R, target=None, match_weight=1.0, kB=1.0, weights=None):
    m, mat = model_case(name)
    sc, tab = sqs_mod.distance_tables(m, mat, mode)
    spec = sqs_mod.distance_spec(m, mode, target, weights, match_weight, 1e-5, kB)
    cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, step)
    return m, sc, tab, spec, cfg


def ref_distance(oe, occ, spec, mode):
    """distance.py:133-154 from a full recomputation."""
    f = oe.correlations(occ) if mode == capi.FEATURES_CORRELATIONS else oe.interactions(occ)
    d = np.abs(f - spec.target)
    w = spec.struct.match_weight
    d[0] = sqs_mod.exact_match_max_diameter(d, spec.group_diameter, spec.feature_group, spec.struct.match_tol) if w else 0.0
    H = float(np.concatenate([[-w], spec.weights]) @ d)
    return d, H


def ordered_target(oe, sc, mode, kind="L10"):
    """Features of an ordered structure that fits the cell: L1_0 layers along z (binary)."""
    z = sc.lattice_points[sc.site_t][:, 2]
    occ = (z % 2).astype(np.int32)
    f = oe.correlations(occ) if mode == capi.FEATURES_CORRELATIONS else oe.interactions(occ)
    return occ, f


def random_occ(sc, R, seed):
    rng = np.random.default_rng(seed)
    return np.stack([sqs_mod.random_ordered_occupancy(sc, rng) for _ in range(R)])


@pytest.mark.parametrize("name", ["binary444", "binary222", "ternary333", "rocksalt333"])
@pytest.mark.parametrize("mode", [capi.FEATURES_CORRELATIONS, capi.FEATURES_INTERACTIONS])
def test_eval_full_and_delta(lib, name, mode):
    m, sc, tab, spec0, cfg = setup(name, mode, capi.STEP_SWAP, 4)
    oe = orc.OracleEvaluator(tab)
    if name.startswith("binary"):  # a target that some rows match exactly: the L term is non-zero there
        l10, tgt = ordered_target(oe, sc, mode)
    else:
        l10, tgt = None, np.zeros(spec0.struct.n_features)
    spec = sqs_mod.distance_spec(m, mode, tgt, None, 1.0, 1e-5, 1.0)
    eng = engine.Engine(tab, cfg, distance=spec)
    assert eng.kernel_info().startswith("dist")
    occ = random_occ(sc, 6, 1)
    if l10 is not None:
        occ[0] = l10
    got = eng.eval_full(occ)
    for i in range(len(occ)):
        d, _ = ref_distance(oe, occ[i], spec, mode)
        np.testing.assert_allclose(got[i], d, rtol=0, atol=1e-12)
    if l10 is not None:
        assert got[0][0] > 0  # the L term of the matched structure
    # single and double flips (sequential semantics) against full recomputation
    rng = np.random.default_rng(2)
    nsp = np.array([m.prim.nspecies[b] for b in sc.site_b])
    active = np.flatnonzero(nsp > 1)
    recs, want = [], []
    base = occ[0]
    for k in range(12):
        s1, s2 = rng.choice(active, 2, replace=False)
        c1, c2 = (base[s1] + 1) % nsp[s1], (base[s2] + 1) % nsp[s2]
        rec = [s1, c1] if k % 2 == 0 else [s1, c1, s2, c2]
        recs.append(rec + [-1] * (capi.STEP_ROW - len(rec)))
        o2 = base.copy()
        o2[s1] = c1
        if k % 2:
            o2[s2] = c2
        want.append(ref_distance(oe, o2, spec, mode)[0] - ref_distance(oe, base, spec, mode)[0])
    dd = eng.eval_delta(base, np.array(recs, dtype=np.int32))
    np.testing.assert_allclose(dd, np.array(want), rtol=0, atol=1e-12)
    eng.close()


def restate_chain(tab, cfg1, spec, mode, occ0, seed, T, nsteps):
    """The numpy restatement: proposals from OracleMC.propose, uniform u53(W(step, 0)[2:4]), full distance per step."""
    oe = orc.OracleEvaluator(tab)
    om = orc.OracleMC(tab, cfg1)
    occ = occ0.copy()
    om.set_state(occ[None], np.array([seed], np.uint64), T)
    d, H = ref_distance(oe, occ, spec, mode)
    beta = 1.0 / (spec.struct.kB * T)
    nacc = 0
    key = [seed & 0xFFFFFFFF, seed >> 32]
    for step in range(nsteps):
        nf, fl = om.propose(0, step)
        w0 = orc.philox([step & 0xFFFFFFFF, step >> 32, 0, 0], key)
        u = (((w0[2] >> 5) << 26) | (w0[3] >> 6)) * (1.0 / 9007199254740992.0)
        new = occ.copy()
        for f in range(nf):
            new[fl[2 * f]] = fl[2 * f + 1]
        d2, H2 = ref_distance(oe, new, spec, mode)
        expo = -beta * (H2 - H)
        acc = expo >= 0 or expo > np.log(u)
        if acc:
            occ, d, H = new, d2, H2
            nacc += 1
            om.set_state(occ[None], np.array([seed], np.uint64), T)
    return occ, d, H, nacc


@pytest.mark.parametrize("name,mode,step", [
    ("binary444", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP),
    ("binary444", capi.FEATURES_CORRELATIONS, capi.STEP_FLIP),
    ("binary222", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP),
    ("binary444", capi.FEATURES_INTERACTIONS, capi.STEP_SWAP),
    ("ternary333", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP),
    ("rocksalt333", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP),
    ("rocksalt333", capi.FEATURES_CORRELATIONS, capi.STEP_FLIP),
])
def test_native_stream_matches_restatement(lib, name, mode, step):
    # 64 walkers x 2000 steps, two launches (the restatement recomputes the full distance on the CPU at every
    # step, ~0.1 ms each: this is what keeps the run short of the 4000 steps a GPU-only check could take)
    R, n, T = 64, 2000, 0.05
    m, sc, tab, _, cfg = setup(name, mode, step, R)
    oe = orc.OracleEvaluator(tab)
    tgt = ordered_target(oe, sc, mode)[1] if name.startswith("binary") else None
    spec = sqs_mod.distance_spec(m, mode, tgt, None, 1.0, 1e-5, 1.0)
    eng = engine.Engine(tab, cfg, distance=spec)
    assert eng.kernel_info().startswith("dist")
    occ0 = random_occ(sc, R, 7)
    seeds = np.arange(R, dtype=np.uint64) * np.uint64(7919) + np.uint64(3)
    eng.set_state(occ0, seeds, T)
    eng.run(n // 3)
    eng.run(n - n // 3)  # two launches: the features are taken afresh from the occupancy in between
    st = eng.get_state()
    cfg1 = capi.make_config(1, capi.KERNEL_METROPOLIS, step)
    for r in range(R):
        occ, d, H, nacc = restate_chain(tab, cfg1, spec, mode, occ0[r], int(seeds[r]), T, n)
        assert np.array_equal(st["occupancy"][r], occ), r
        assert int(st["n_accepted"][r]) == nacc
        np.testing.assert_allclose(st["enthalpy"][r], H, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(st["features"][r], d, rtol=1e-10, atol=1e-10)
    assert np.all(st["n_steps"] == n)
    eng.close()


def test_replay_matches_restatement(lib):
    R, n, T = 8, 600, 0.1
    m, sc, tab, _, cfg = setup("binary444", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP, R)
    oe = orc.OracleEvaluator(tab)
    spec = sqs_mod.distance_spec(m, capi.FEATURES_CORRELATIONS, ordered_target(oe, sc, 0)[1], None, 1.0, 1e-5, 1.0)
    occ0 = random_occ(sc, R, 11)
    rng = np.random.default_rng(5)
    steps = np.full((R, n, capi.STEP_ROW), -1, dtype=np.int32)
    us = rng.random((R, n))
    acc_ref, H_ref, occ_ref = np.zeros((R, n), bool), np.zeros((R, n)), occ0.copy()
    for r in range(R):
        occ = occ0[r].copy()
        d, H = ref_distance(oe, occ, spec, 0)
        for i in range(n):  # a reference-order swap trajectory
            while True:
                s1, s2 = rng.integers(0, sc.num_sites, 2)
                if occ[s1] != occ[s2]:
                    break
            steps[r, i, :4] = [s1, occ[s2], s2, occ[s1]]
            new = occ.copy()
            new[s1], new[s2] = occ[s2], occ[s1]
            d2, H2 = ref_distance(oe, new, spec, 0)
            expo = -(H2 - H) / T
            a = expo >= 0 or expo > np.log(us[r, i])
            if a:
                occ, d, H = new, d2, H2
            acc_ref[r, i], H_ref[r, i] = a, H
        occ_ref[r] = occ
    eng = engine.Engine(tab, cfg, distance=spec)
    eng.set_state(occ0, None, T)
    acc, H = eng.replay(steps, us)
    assert np.array_equal(acc, acc_ref)
    np.testing.assert_allclose(H, H_ref, rtol=1e-10, atol=1e-10)
    assert np.array_equal(eng.get_state()["occupancy"], occ_ref)
    eng.close()


def test_best_records_and_samples(lib):
    R, T = 32, 0.5
    m, sc, tab, spec, cfg = setup("binary444", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP, R)
    oe = orc.OracleEvaluator(tab)
    eng = engine.Engine(tab, cfg, distance=spec)
    occ0 = random_occ(sc, R, 3)
    eng.set_state(occ0, np.arange(R, dtype=np.uint64) + np.uint64(1), T)
    b0 = eng.get_best()
    np.testing.assert_allclose(b0["score"], eng.get_state()["enthalpy"], rtol=0, atol=0)
    assert np.array_equal(b0["occupancy"], occ0)
    smp = eng.run_sampled(20, 50, occupancy=True)
    Hs = np.asarray(smp["enthalpy"])
    st = eng.get_state()
    # the last sample row is the state at the end of the block
    np.testing.assert_array_equal(Hs[-1], st["enthalpy"])
    np.testing.assert_array_equal(np.asarray(smp["features"])[-1], st["features"])
    np.testing.assert_array_equal(np.asarray(smp["occupancy"])[-1], st["occupancy"])
    for j in (0, 7):  # rows are distance vectors of their occupancies
        rows = np.asarray(smp["occupancy"])[j]
        for r in range(0, R, 8):
            d, H = ref_distance(oe, rows[r], spec, 0)
            np.testing.assert_allclose(np.asarray(smp["features"])[j][r], d, rtol=0, atol=1e-10)
            np.testing.assert_allclose(Hs[j][r], H, rtol=1e-10, atol=1e-10)
    best = eng.get_best()
    assert np.all(best["score"] <= Hs.min(axis=0) + 1e-12)
    assert np.all(best["score"] <= b0["score"])
    for r in range(R):
        d, H = ref_distance(oe, best["occupancy"][r], spec, 0)
        np.testing.assert_allclose(best["score"][r], H, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(best["features"][r], d, rtol=0, atol=1e-10)
        assert np.bincount(best["occupancy"][r], minlength=2).tolist() == np.bincount(occ0[r], minlength=2).tolist()
    assert np.all(best["step"] <= 1000)
    eng.reset_best()
    b1 = eng.get_best()
    # (the launch takes the features afresh from the occupancy: the running enthalpy to rounding)
    np.testing.assert_allclose(b1["score"], st["enthalpy"], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(b1["occupancy"], st["occupancy"])
    assert np.all(b1["step"] == 1000)
    eng.close()


def test_create_refusals(lib):
    m, sc, tab, spec, cfg = setup("binary222", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP, 2)
    with pytest.raises(Exception, match="Wang-Landau"):
        engine.Engine(tab, capi.make_config(2, capi.KERNEL_WANGLANDAU, capi.STEP_SWAP, min_enthalpy=-10,
                                            max_enthalpy=10, bin_size=1), distance=spec)
    bad = capi.DistanceSpec(spec.target, spec.weights, -1.0, 1e-5, spec.group_diameter, spec.feature_group, 1.0)
    with pytest.raises(Exception, match="match weight"):
        engine.Engine(tab, cfg, distance=bad)
    eng = engine.Engine(tab, cfg)
    with pytest.raises(Exception, match="not a distance handle"):
        eng.get_best()
    eng.close()


def test_known_answer_l10():
    """The L1_0 target in the 64-site binary cell: the default ladder finds a structure matching every feature,
    score -(largest diameter), whose correlations are L1_0's."""
    m, mat = model_case("binary444")
    sc, tab = sqs_mod.distance_tables(m, mat, capi.FEATURES_CORRELATIONS)
    oe = orc.OracleEvaluator(tab)
    _, tgt = ordered_target(oe, sc, capi.FEATURES_CORRELATIONS)
    gen = sqs_mod.StochasticSQSGenerator(m, 64, target_vector=tgt, match_weight=1.0, supercell_matrices=[mat],
                                         nwalkers=256, seeds=1)
    gen.generate(2000)
    best = gen.get_best_sqs(1)[0]
    gd, _ = sqs_mod.diameter_groups(m, capi.FEATURES_CORRELATIONS)
    assert np.all(best.feature_distance[1:] <= 1e-5)
    np.testing.assert_allclose(best.score, -gd[-1], rtol=0, atol=1e-9)
    np.testing.assert_allclose(oe.correlations(best.occupancy), tgt, rtol=0, atol=1e-9)
    np.testing.assert_allclose(gen.compute_score(best.occupancy, mat), best.score, atol=1e-9)


def test_default_target_beats_random():
    m, mat = model_case("binary444")
    gen = sqs_mod.StochasticSQSGenerator(m, 64, supercell_matrices=[mat], nwalkers=64, seeds=2)
    sc = gen._cells[0][0]
    init = random_occ(sc, 64, 9)
    init_scores = [gen.compute_score(o, mat) for o in init]
    gen.generate(500, initial_occupancies=[init])
    res = gen.get_best_sqs(5)
    assert len(res) == 5 and res[0].score <= res[-1].score
    assert res[0].score < np.mean(init_scores)
    assert np.array_equal(np.bincount(res[0].occupancy, minlength=2), [32, 32])


GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distance_v1.npz"))


@pytest.mark.parametrize("name", ["binary444", "binary222", "ternary333", "rocksalt333"])
@pytest.mark.parametrize("mode", [capi.FEATURES_CORRELATIONS, capi.FEATURES_INTERACTIONS])
@pytest.mark.parametrize("w", [0.0, 1.0])
def test_eval_against_reference_fixture(lib, name, mode, w):
    """eval_full / eval_delta of a distance handle against the reference's compiled
    corr_/interaction_distances_from_occupancies (tests/golden/distance_v1.npz), entry 0 = L (w = 1) or 0."""
    key = "corr" if mode == capi.FEATURES_CORRELATIONS else "int"
    m, sc, tab, _, cfg = setup(name, mode, capi.STEP_SWAP, 2)
    spec = sqs_mod.distance_spec(m, mode, GOLDEN[f"{name}/target_{key}"], None, w, float(GOLDEN[f"{name}/match_tol"]), 1.0)
    eng = engine.Engine(tab, cfg, distance=spec)
    rows, L = GOLDEN[f"{name}/dist_{key}"].copy(), GOLDEN[f"{name}/L_{key}"]
    rows[:, :, 0] = L if w else 0.0
    oi, of = GOLDEN[f"{name}/occ_i"], GOLDEN[f"{name}/occ_f"]
    np.testing.assert_allclose(eng.eval_full(oi), rows[:, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(eng.eval_full(of), rows[:, 1], rtol=0, atol=1e-12)
    for i in range(len(oi)):
        flips = [[int(s), int(of[i][s])] for s in np.flatnonzero(of[i] != oi[i])]
        rec = np.full((1, capi.STEP_ROW), -1, np.int32)
        rec[0, :2 * len(flips)] = np.ravel(flips)
        np.testing.assert_allclose(eng.eval_delta(oi[i], rec)[0], rows[i, 1] - rows[i, 0], rtol=0, atol=1e-12)
    eng.close()


def test_replay_reference_trajectory(lib):
    """The fixture's reference-order Metropolis swap chain (kB = 1): accept flags bit-exact, enthalpies 1e-10."""
    m, sc, tab, _, _ = setup("binary444", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP, 1)
    occ0, steps = GOLDEN["traj/occ0"], GOLDEN["traj/steps"]
    R, n = steps.shape[:2]
    spec = sqs_mod.distance_spec(m, capi.FEATURES_CORRELATIONS, GOLDEN["binary444/target_corr"], None, 1.0, 1e-5, 1.0)
    eng = engine.Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP), distance=spec)
    eng.set_state(occ0, None, float(GOLDEN["traj/T"]))
    rec = np.full((R, n, capi.STEP_ROW), -1, np.int32)
    rec[:, :, :4] = steps
    acc, H = eng.replay(rec, GOLDEN["traj/uniforms"])
    assert np.array_equal(acc, GOLDEN["traj/accepted"].astype(bool))
    np.testing.assert_allclose(H, GOLDEN["traj/enthalpy"], rtol=1e-10, atol=1e-10)
    occ = occ0.copy()
    for r in range(R):
        for i in range(n):
            if acc[r, i]:
                s1, c1, s2, c2 = steps[r, i]
                occ[r, s1], occ[r, s2] = c1, c2
    assert np.array_equal(eng.get_state()["occupancy"], occ)
    eng.close()


def test_sampler_on_distance_ensemble(lib):
    """moca: an Ensemble on a CorrelationDistanceProcessor runs the distance kernel through Sampler; the kernel's
    kB reaches the handle; Wang-Landau and biases are refused."""
    from smol_amd import moca

    m, mat = model_case("binary444")
    sc = synth.build_supercell(m, mat)
    ens = moca.Ensemble(moca.CorrelationDistanceProcessor(sc))
    R, T = 16, 0.2
    sampler = moca.Sampler.from_ensemble(ens, T, nwalkers=R, step_type="swap")
    for k in sampler.mckernels:
        k.kB = 1.0
        k.temperature = T
    occ = random_occ(sc, R, 4)
    sampler.run(500, occ, thin_by=100)
    eng = sampler._get_engine()
    assert eng.kernel_info().startswith("dist")
    st = eng.get_state()
    for r in range(0, R, 5):
        np.testing.assert_allclose(st["enthalpy"][r], ens.processor.compute_property(st["occupancy"][r]),
                                   rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(st["features"][r], ens.compute_feature_vector(st["occupancy"][r]),
                                   rtol=0, atol=1e-10)
    assert eng.distance.struct.kB == 1.0
    with pytest.raises(ValueError):
        moca.Sampler.from_ensemble(ens, kernel_type="Wang-Landau", min_enthalpy=-10, max_enthalpy=10, bin_size=1,
                                   nwalkers=2, step_type="swap")._get_engine()
    with pytest.raises(ValueError):
        moca.Sampler.from_ensemble(ens, T, nwalkers=2, step_type="swap", bias_type="fugacity")._get_engine()
