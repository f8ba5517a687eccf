"""Population annealing on the host: the integer definition of the resampling move (parallel.PopulationAnnealing),
the scheme on the CPU oracle against exact enumeration, and the argument checks of Sampler.anneal_population.  The
device side is tests/test_gpu_pop_anneal.py."""

import itertools
from fractions import Fraction

import numpy as np
import pytest

from smol_amd import parallel
from tests import pop_anneal_case as pc
from tests import wl_windows_case as wc

PA = parallel.PopulationAnnealing


def word_of_offset(off, Q):
    """A 64-bit word whose offset (word * Q) >> 64 is ``off`` (0 <= off < Q)."""
    word = -((-off << 64) // Q)  # ceil(off 2^64 / Q)
    assert 0 <= word < 2 ** 64 and (word * Q) >> 64 == off
    return word


def check_map(q, word):
    q = np.asarray(q, dtype=np.uint64)
    n = len(q)
    cnt = PA.children(q, word)
    parent = PA.parent_map(q, word)
    assert cnt.sum() == n
    assert np.all(cnt[q == 0] == 0)
    alive = cnt > 0
    assert np.array_equal(parent[alive], np.flatnonzero(alive))  # survivors keep their slot
    assert np.array_equal(parent[parent], parent)                 # a source is never a destination
    assert np.array_equal(np.bincount(parent, minlength=n), cnt)
    filled = parent[~alive]
    assert np.all(np.diff(filled) >= 0)                           # dead slots are filled in ascending order of donors
    assert np.array_equal(filled, np.repeat(np.arange(n), np.maximum(cnt - 1, 0)))
    return cnt, parent


# ---- exactness of the map -------------------------------------------------------------------------------------------
def small_weight_vectors():
    rng = np.random.default_rng(3)
    out = [[1], [3, 1], [1, 0, 2], [0, 0, 5], [7, 7, 7, 7], [1, 2, 3, 4, 5], [13, 0, 1, 0, 9, 2], [1, 1, 1, 1, 1, 35]]
    for n in range(2, 7):
        for _ in range(6):
            q = rng.integers(0, 9, size=n)
            if q.sum() == 0:
                q[rng.integers(n)] = 1
            out.append([int(x) for x in q])
    assert all(len(q) <= 6 and 0 < sum(q) <= 40 for q in out)
    return out


@pytest.mark.parametrize("q", small_weight_vectors(), ids=lambda q: "-".join(map(str, q)))
def test_every_offset_unbiased(q):
    """Over all offsets 0 .. Q - 1 the mean number of children of j is n q_j / Q exactly, and every map is well formed."""
    n, Q = len(q), sum(q)
    total = np.zeros(n, dtype=np.int64)
    for off in range(Q):
        cnt, _ = check_map(q, word_of_offset(off, Q))
        total += cnt
    for j in range(n):
        assert Fraction(int(total[j]), Q) == Fraction(n * q[j], Q)


def test_children_against_the_rule_spelled_out():
    """``children`` (a sorted search over integer thresholds) against the rule as written: child m descends from the
    smallest j with n C_j > m Q + off, in Python integers of any size."""
    rng = np.random.default_rng(11)
    for n in (1, 2, 5, 64, 131):
        q = [int(x) for x in rng.integers(0, 2 ** 40 + 1, size=n)]
        q[rng.integers(n)] = 2 ** 40
        for word in (0, 2 ** 64 - 1, int(rng.integers(0, 2 ** 63)) * 2 + 1):
            Q, C = sum(q), list(itertools.accumulate(q))
            off = (word * Q) >> 64
            cnt = [0] * n
            for m in range(n):
                cnt[next(j for j in range(n) if n * C[j] > m * Q + off)] += 1
            assert np.array_equal(PA.children(q, word), cnt)
            check_map(q, word)


# ---- degenerate inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", [0, 1, 2 ** 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15])
def test_equal_weights_are_the_identity(word):
    H = np.random.default_rng(1).normal(size=37)
    q, Q, href = PA.weights(H, 2.5, 2.5)  # db = 0
    assert np.all(q == 2 ** 40) and Q == 37 * 2 ** 40 and href == H.max()
    assert np.array_equal(PA.parent_map(q, word), np.arange(37))


@pytest.mark.parametrize("word", [0, 2 ** 64 - 1, 12345678901234567])
def test_single_walker_and_single_weight(word):
    q, Q, href = PA.weights([0.3], 1.0, 7.0)
    assert q[0] == 2 ** 40 and Q == 2 ** 40 and href == 0.3
    assert np.array_equal(PA.parent_map(q, word), [0])
    assert np.array_equal(PA.parent_map([0, 0, 9, 0, 0], word), [2] * 5)
    assert np.array_equal(PA.parent_map([0, 0, 0, 0, 2 ** 40], word), [4] * 5)


def test_weights_follow_the_sign_of_db():
    H = np.array([0.5, -0.25, 1.0, -0.25])
    q, Q, href = PA.weights(H, 1.0, 3.0)  # cooling: the lowest enthalpy has weight 1
    assert href == -0.25 and q[1] == q[3] == 2 ** 40 and np.all(q <= 2 ** 40) and Q == int(q.astype(object).sum())
    assert q[0] == int(np.floor(np.exp(-(2.0 * 0.75)) * 2.0 ** 40))
    q, Q, href = PA.weights(H, 3.0, 1.0)  # heating: the highest
    assert href == 1.0 and q[2] == 2 ** 40 and q[1] == int(np.floor(np.exp(-(-2.0 * -1.25)) * 2.0 ** 40))
    q, _, _ = PA.weights([0.0, 1.0], 0.0, 50.0)  # a weight below 2^-40 truncates to zero: no copy
    assert q[1] == 0 and np.array_equal(PA.parent_map(q, 2 ** 64 - 1), [0, 0])


def test_offset_words_and_bookkeeping():
    pa = PA([900.0, 600.0, 400.0], populations=3, seed=9)
    w = pa.offset_words(4)
    u = parallel._philox_uniforms(9, 4, 3)
    assert w.dtype == np.uint64 and np.array_equal(w, (u * 2.0 ** 53).astype(np.uint64) << np.uint64(11))
    assert np.array_equal(w, pa.offset_words(4)) and not np.array_equal(w, pa.offset_words(5))
    H = np.random.default_rng(2).normal(scale=0.05, size=12)
    res = pa.step(H, 0)
    n = 4
    for p in range(3):
        sl = slice(4 * p, 4 * p + 4)
        q, Q, href = PA.weights(H[sl], pa.betas[0], pa.betas[1])
        assert np.array_equal(res["q"][sl], q) and int(res["qsum"][p]) == Q and res["href"][p] == href
        assert np.array_equal(res["parent"][sl], 4 * p + PA.parent_map(q, pa.offset_words(0)[p]))
        assert res["log_q"][p] == np.log(Q / (n * 2.0 ** 40)) - (pa.betas[1] - pa.betas[0]) * href
    res2 = pa.step(H[res["parent"]], 1)
    assert pa.calls == 2 and pa.log_q.shape == (2, 3) and pa.n_families.shape == (2, 3) and pa.rho_t.shape == (2, 3)
    assert np.array_equal(pa.family, res["parent"][res2["parent"]])
    np.testing.assert_array_equal(pa.log_partition_ratio(), res["log_q"] + res2["log_q"])
    assert pa.free_energy().shape == (2, 3)
    np.testing.assert_allclose(pa.free_energy()[1], -pa.log_partition_ratio() / pa.betas[2])
    for p in range(3):
        _, sizes = np.unique(pa.family[4 * p:4 * p + 4], return_counts=True)
        assert pa.n_families[1, p] == len(sizes) and pa.rho_t[1, p] == (sizes ** 2).sum() / 4
    wts = pa.population_weights()
    np.testing.assert_allclose(wts, np.exp(pa.log_partition_ratio()) / np.exp(pa.log_partition_ratio()).sum())
    np.testing.assert_allclose(pa.combine([1.0, 2.0, 4.0]), wts @ [1.0, 2.0, 4.0])
    np.testing.assert_allclose(pa.combined_log_partition_ratio(), np.log(np.mean(np.exp(pa.log_partition_ratio()))))
    with pytest.raises(ValueError, match="populations do not divide"):
        pa.step(np.zeros(10), 0, record=False)
    with pytest.raises(ValueError, match="positive"):
        PA([300.0, 0.0])


# ---- the scheme on the CPU oracle against exact enumeration ---------------------------------------------------------
def test_exact_values_of_the_case():
    lnz, emean = pc.exact()
    assert abs(lnz - pc.LNZ_EXACT) < 1e-5 and abs(emean - pc.EMEAN_EXACT) < 1e-6
    E = wc.case()["E"]
    assert len(E) == 12870 and abs(E.min() + 0.162) < 1e-3 and abs(E.max() - 6.373) < 1e-3


@pytest.mark.parametrize("seed", pc.SEEDS)
def test_oracle_population_annealing_against_enumeration(seed):
    dl, de, history = pc.oracle_errors(seed)
    print(f"seed {seed}: sum ln Q - exact", np.round(dl, 4), " final mean enthalpy - exact", np.round(de, 5))
    assert len(history) == len(pc.TEMPERATURES) - 1
    n = pc.WALKERS
    for parent in history:  # (on the NumPy definition alone: the resampling does something, and not too much)
        for p in range(pc.POPULATIONS):
            local = parent[p * n:(p + 1) * n] - p * n
            assert local.min() >= 0 and local.max() < n
            cnt = np.bincount(local, minlength=n)
            assert (cnt == 0).sum() >= 1, "a step killed no walker"
            assert (cnt > 0).sum() >= n // 2, "a step left fewer than half the walkers as distinct survivors"
    assert np.all(np.abs(dl) <= pc.LNZ_BOUND), dl
    assert np.all(np.abs(de) <= pc.EMEAN_BOUND), de


# ---- Sampler.anneal_population: argument checks and schema (no engine) ----------------------------------------------
def test_sampler_anneal_population_arguments():
    from smol_amd import moca

    c = wc.case()
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    s = moca.Sampler.from_ensemble(ens, temperature=3000.0, step_type="swap", nwalkers=6, seeds=list(range(6)))
    occ = pc.start_occupancies(5, 6)
    with pytest.raises(ValueError, match="End temperature is greater"):
        s.anneal_population([300.0, 3000.0], 10, occ)
    with pytest.raises(ValueError, match="populations do not divide"):
        s.anneal_population([3000.0, 300.0], 10, occ, populations=4)
    with pytest.raises(ValueError, match="at least one temperature"):
        s.anneal_population([], 10, occ)
    with pytest.raises(RuntimeError, match="initial occupancies"):
        s.anneal_population([3000.0, 300.0], 10, None, populations=2)
    wl = moca.Sampler.from_ensemble(ens, c["lo"], c["hi"], c["bin"], kernel_type="Wang-Landau")
    with pytest.raises(AttributeError, match="thermal kernel"):
        wl.anneal_population([3000.0, 300.0], 10, occ[:1])
    # the metadata block round-trips through to_npz / from_npz
    meta = dict(temperatures=[3000.0, 300.0], populations=2, seed=4, log_partition_ratio=[[0.0, 0.0], [4.1, 4.2]],
                n_families=[[3, 3], [2, 1]], rho_t=[[1.0, 1.0], [1.5, 3.0]])
    s.samples.metadata["population_annealing"] = meta
    import os
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "samples.npz")
        s.samples.to_npz(path)
        assert moca.SampleContainer.from_npz(path, ens).metadata["population_annealing"] == meta
