"""All five per-sample families (smol_amd/families.py) in one sampler: the order of their traces in a block, a statistics
record that reads all five segments of the column sources at once, a minima record beside it."""

import numpy as np
import pytest

from smol_amd import connectivity as cn
from smol_amd import moca
from smol_amd import statistics as st
from smol_amd.connectivity import Connectivity
from smol_amd.minima import Minima
from smol_amd.patterns import Patterns
from smol_amd.statistics import Statistics, StatisticsRecord
from smol_amd.structure import StructureFactor, commensurate_points
from tests.cases import load_case
from tests.test_environments_host import case_spec
from tests.test_gpu_observables import ENV, _rand_occ
from tests.test_gpu_statistics import _same_record

pytestmark = pytest.mark.gpu
CASE = "rocksalt333_two_sublattices"
NW, NS, THIN = 6, 12, 9
TRACES = ("species_counts", "pair_counts", "structure_amplitudes", "structure_intensities", "connectivity", "pattern_counts",
          "environment_counts")


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _same(got, want, dtype):
    assert got.dtype == dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want)  # (the float64 intensities too: exact equality)


def five_specs():
    """(the case, from_ensemble keyword -> spec): the specs the sampler tests of the five families use on this case."""
    c = load_case(CASE)
    sc, obs, env = case_spec(CASE)
    sf = StructureFactor.from_supercell(sc, commensurate_points(sc),
                                        intensities=[(q, a, a) for q in (0, 13, 26) for a in range(obs.n_kinds)])
    conn = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=3.0), dict(members=[1, 2], cutoff=4.3)])
    pat = Patterns.from_supercell(sc, obs, orbits=[o.id for o in sc.model.orbits if o.size >= 3][:3])
    return c, dict(observables=obs, structure_factor=sf, connectivity=conn, patterns=pat, environments=env)


def five_sampler(c, specs, nw=NW, **kw):
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    return moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                      **specs, **kw), ens


def scenario():
    """(the case, the five specs, start occupancies, a statistics spec with one column of each of the seven tags)."""
    c, specs = five_specs()
    occ = _rand_occ(c["sc"], np.random.default_rng(12), NW)
    pool = _rand_occ(c["sc"], np.random.default_rng(1), 40)
    moving = [int(np.flatnonzero(specs[k].evaluate(pool).std(axis=0) > 0)[1]) for k in ("patterns", "environments")]
    # (intensity 7 is at a wave vector other than zero: swaps move it; a kind count they cannot move)
    cols = [st.ENTHALPY, st.feature(1), st.kind(specs["observables"], 1), st.intensity(7), st.connectivity(0, cn.WRAP_AXES),
            st.pattern(moving[0]), st.environment(moving[1])]
    stat = Statistics.per_walker(cols, n_levels=3, hist=(st.environment(moving[1]), 64, 0.0, 1.0))
    return c, specs, occ, stat


def _offered(stat, H, f, traces):
    """The definition's record of rows with enthalpy (ns, NW), features and the derived traces by name."""
    return StatisticsRecord(stat, NW).offer(H, f, traces["species_counts"], intensities=traces["structure_intensities"],
                                            connectivity=traces["connectivity"], patterns=traces["pattern_counts"],
                                            environments=traces["environment_counts"])


def test_one_sampler_traces_all_five_families(clean_env, tmp_path):
    c, specs, occ, stat = scenario()
    sampler, ens = five_sampler(c, specs, statistics=stat, minima=Minima.per_walker())
    sampler.run(NS * THIN, occ, thin_by=THIN)
    s = sampler.samples
    assert s.num_samples == NS and tuple(s.traced_values[-7:]) == TRACES
    occs = s.get_occupancies(flat=False)
    traces = {name: s.get_trace_value(name, flat=False) for name in TRACES}
    # every trace is its spec's definition on the recorded occupancies
    counts, pairs = specs["observables"].evaluate(occs)
    amp, inten = specs["structure_factor"].evaluate(occs)
    want = dict(species_counts=counts, pair_counts=pairs, structure_amplitudes=amp, structure_intensities=inten,
                connectivity=specs["connectivity"].evaluate(occs)[0], pattern_counts=specs["patterns"].evaluate(occs),
                environment_counts=specs["environments"].evaluate(occs))
    dtypes = dict(zip(TRACES, (np.int32, np.int32, np.int64, np.float64, np.int64, np.int32, np.int32)))
    for name in TRACES:
        assert traces[name].shape[:2] == (NS, NW)
        _same(traces[name], want[name], dtypes[name])
    assert s.get_pattern_counts(flat=False).any() and s.get_environment_counts(flat=False).any() and traces["connectivity"].any()
    # the statistics record read all five segments; the minima record saw every sample
    H, f = s.get_trace_value("enthalpy", flat=False)[:, :, 0], s.get_trace_value("features", flat=False)
    rec = _offered(stat, H, f, traces)
    _same_record(sampler.statistics, rec, "one pass")
    # (the enthalpy, the intensity and the two cells did not stand still; the graphs of this case rarely change)
    assert all((rec.s1[:, j] != 0).any() for j in (0, 3, 5, 6))
    low = sampler.minima
    np.testing.assert_array_equal(low.value, H.min(axis=0) + 0.0)
    np.testing.assert_array_equal(low.occupancy, occs[H.argmin(axis=0), np.arange(NW)])
    # the same pass in three ring blocks: block k + 1 is queued before block k is fetched
    split, _ = five_sampler(c, specs, statistics=stat, minima=Minima.per_walker())
    blocks = list(split._sample_blocks(NS * THIN, occ, THIN, max_block=5))
    assert [len(b["enthalpy"]) for b in blocks] == [5, 5, 2]
    for b in blocks:
        assert tuple(b)[-7:] == TRACES
    got = {name: np.concatenate([b[name] for b in blocks]) for name in blocks[0]}
    for name in TRACES:  # (the chains do not depend on where the blocks end)
        np.testing.assert_array_equal(got[name], traces[name], err_msg=name)
    # the enthalpy is a running sum that a launch boundary may round differently (seen: the last bit): the two records of
    # this pass are compared on the rows of its own blocks
    Hs = got["enthalpy"][:, :, 0]
    _same_record(split.statistics, _offered(stat, Hs, got["features"], got), "three blocks")
    np.testing.assert_array_equal(split.minima.value, Hs.min(axis=0) + 0.0)
    # keep_occupancy=False: the occupancies stay on the device, the derived traces are the same
    dry, _ = five_sampler(c, specs, statistics=stat, minima=Minima.per_walker())
    dry.run(NS * THIN, occ, thin_by=THIN, keep_occupancy=False)
    with pytest.raises(ValueError, match="keep_occupancy=False"):
        dry.samples.get_occupancies()
    for name in TRACES + ("enthalpy", "features", "accepted"):
        assert np.array_equal(dry.samples.get_trace_value(name, flat=False), s.get_trace_value(name, flat=False)), name
    _same_record(dry.statistics, rec, "dry")
    # the npz round trip carries the traces and the metadata
    s.to_npz(tmp_path / "five.npz")
    back = moca.SampleContainer.from_npz(tmp_path / "five.npz", ens)
    for name in TRACES:
        _same(back.get_trace_value(name, flat=False), traces[name], dtypes[name])
    for key in ("observables", "connectivity", "patterns", "environments"):
        assert back.metadata[key] == s.metadata[key], key
    assert back.metadata["connectivity"] == specs["connectivity"].to_metadata()
    assert back.metadata["patterns"] == specs["patterns"].describe()
    assert back.metadata["environments"] == specs["environments"].describe()
