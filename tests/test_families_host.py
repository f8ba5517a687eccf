"""The table of the per-sample families (smol_amd/families.py) against what it drives: the C ABI's flags and symbols, the
column sources of a statistics record, the schema a sampler builds before an engine exists, the meta/* arrays of an .npz."""

import numpy as np

from smol_amd import capi, engine, moca
from smol_amd import statistics as st
from smol_amd.families import BY_NAME, FAMILIES, trace_shape
from smol_amd.statistics import Statistics
from tests.test_gpu_families import TRACES, five_sampler, five_specs  # (no engine: the helpers build specs and a sampler)


def test_the_table_names_the_flags_symbols_and_methods_of_the_c_abi():
    assert [fam.name for fam in FAMILIES] == ["observables", "structure", "connectivity", "patterns", "environments"]
    assert tuple(name for fam in FAMILIES for name, _, _ in fam.traces) == TRACES
    flags = dict(engine.SAMPLE_FLAGS)
    assert len(flags) == len(engine.SAMPLE_FLAGS) == 5 + len(FAMILIES)
    assert sum(flags.values()) == (1 << len(flags)) - 1  # (every bit once)
    for fam in FAMILIES:
        assert BY_NAME[fam.name] is fam
        assert fam.flag == getattr(capi, "SAMPLE_" + fam.name.upper()) == flags[fam.run_keyword]
        for symbol in (f"smolmc_set_{fam.stem}", f"smolmc_{fam.stem}_shape", f"smolmc_eval_{fam.stem}", f"smolmc_get_sample_{fam.stem}"):
            assert symbol in engine.SYMBOLS, symbol
        # the shape reader fills one int per size name; eval and get_sample take one pointer per trace
        _, args = engine.SYMBOLS[f"smolmc_{fam.stem}_shape"]
        assert len(args) == 1 + len(fam.sizes)
        assert len(engine.SYMBOLS[f"smolmc_get_sample_{fam.stem}"][1]) == 1 + len(fam.traces)
        assert len(engine.SYMBOLS[f"smolmc_eval_{fam.stem}"][1]) in (3 + len(fam.traces), 4 + len(fam.traces))
        for method in (fam.set, fam.eval, f"{fam.stem}_shape", f"sample_{fam.stem}"):
            assert callable(getattr(engine.Engine, method)), method
        assert callable(getattr(fam.spec, fam.describe))
        assert fam.rests_on is None or FAMILIES.index(BY_NAME[fam.rests_on]) < FAMILIES.index(fam)
        for _, _, dims in fam.traces:
            assert all(isinstance(d, int) or d in fam.sizes for d in dims)
    for keyword in flags:  # the keyword signatures stay explicit: every keyword of the table is one of theirs
        for fn in (engine.Engine.run_sampled, engine.Engine.run_sampled_async):
            assert keyword in fn.__code__.co_varnames[:fn.__code__.co_argcount], keyword


def test_segments_tile_the_column_sources_and_agree_with_sources():
    rng = np.random.default_rng(5)
    tags = ["enthalpy", "feature", "kind", "energy", "intensity", "connectivity", "pattern", "environment"]
    assert [fam.stat[0] for fam in FAMILIES] == ["kind", "intensity", "connectivity", "pattern", "environment"]
    cases = [(0, 0, 0, 0, 0, 0), (3, 0, 0, 0, 0, 0), (1, 2, 0, 1, 0, 4)] + [tuple(int(x) for x in rng.integers(0, 6, 6)) for _ in range(40)]
    for F, K, I, G, PC, EC in cases:
        segs = st.segments(F, K, I, G, PC, EC)
        assert [s[0] for s in segs] == tags
        assert [s[2] for s in segs] == [1, F, K, 1, I, 24 * G, PC, EC]
        at = 0
        for _, first, width in segs:  # (no gap, no overlap)
            assert first == at and width >= 0
            at += width
        assert at == 2 + F + K + I + 24 * G + PC + EC
        # one column of every tag that has a source, at the first and at the last source of its segment
        for last in (False, True):
            cols, want = [], []
            for tag, first, width in segs:
                if width == 0:
                    continue
                i = width - 1 if last else 0
                cols.append({"enthalpy": st.ENTHALPY, "energy": st.ENERGY, "feature": st.feature(i), "kind": ("kind", i),
                             "intensity": st.intensity(i), "connectivity": st.connectivity(i // 24, i % 24),
                             "pattern": st.pattern(i), "environment": st.environment(i)}[tag])
                want.append(first + i)
            got = Statistics.per_walker(cols).sources(F, K, I, G, PC, EC)
            assert got.dtype == np.int32 and got.tolist() == want, (F, K, I, G, PC, EC)


def test_a_sampler_builds_the_schema_of_all_five_families_without_an_engine():
    c, specs = five_specs()
    sampler, _ = five_sampler(c, specs)
    assert sampler._engine is None
    schema, nw = sampler.samples._schema, 6
    assert tuple(schema)[-7:] == TRACES
    K, S, sf = specs["observables"].n_kinds, specs["observables"].n_shells, specs["structure_factor"]
    assert (K, sf.n_kinds, sf.n_points, sf.n_intensities) == (5, 5, 27, 15) and S >= 1
    want = dict(species_counts=(np.int32, (K,)), pair_counts=(np.int32, (S, K, K)),  # (written out: not through the table)
                structure_amplitudes=(np.int64, (27, K, 2)), structure_intensities=(np.float64, (15,)),
                connectivity=(np.int64, (2, 24)), pattern_counts=(np.int32, (specs["patterns"].n_cells,)),
                environment_counts=(np.int32, (specs["environments"].n_cells,)))
    for fam in FAMILIES:
        spec = specs[fam.keyword]
        assert isinstance(spec, fam.spec) and sampler._traced[fam.name] is spec
        assert sampler.samples.metadata[fam.keyword] == getattr(spec, fam.describe)()
        for name, dtype, dims in fam.traces:
            assert schema[name] == (np.dtype(dtype), (nw,) + trace_shape(dims, spec)), name
            assert schema[name] == (np.dtype(want[name][0]), (nw,) + want[name][1]), name
    assert sampler._engine is None


def test_npz_round_trip_of_the_metadata_of_an_empty_container(tmp_path):
    c, specs = five_specs()
    sampler, ens = five_sampler(c, specs)
    path = str(tmp_path / "empty.npz")
    sampler.samples.to_npz(path)
    back = moca.SampleContainer.from_npz(path, ens)
    assert back.num_samples == 0
    for fam in FAMILIES:
        if fam.saved:
            assert back.metadata[fam.keyword] == sampler.samples.metadata[fam.keyword], fam.name
        else:
            assert fam.name == "structure" and fam.keyword not in back.metadata
        for name, dtype, _ in fam.traces:
            assert back._schema[name] == sampler.samples._schema[name], name
    assert [fam.name for fam in FAMILIES if fam.saved] == ["observables", "connectivity", "patterns", "environments"]
