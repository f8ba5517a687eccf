"""One block of the sample ring with every combination of its consumers (smolmc_run_sampled with the observables,
structure, connectivity, minima and statistics flags, occupancy on and off): what is downloaded, what the columns hold and
what the records keep do not depend on which other consumers ran in the same block.  Every comparison is exact: integers and
doubles come from the same kernels on both sides."""

import ctypes as C
import itertools

import numpy as np
import pytest

from smol_amd import capi
from smol_amd import connectivity as cn
from smol_amd import statistics as st
from smol_amd.connectivity import Connectivity
from smol_amd.minima import Minima, MinimaRecord
from smol_amd.statistics import Statistics, StatisticsRecord
from smol_amd.structure import StructureFactor, commensurate_points
from tests.cases import load_case
from tests.test_gpu_minima import _same_record as _same_minima
from tests.test_gpu_observables import ENV, _handle, _rand_occ
from tests.test_gpu_statistics import _same_record as _same_statistics
from tests.test_gpu_statistics import _semigrand

pytestmark = pytest.mark.gpu
CONSUMERS = ("observables", "structure", "connectivity", "minima", "statistics")
NS, THIN = 2, 5
DERIVED = {"observables": ("species_counts", "pair_counts"), "structure": ("structure_amplitudes", "structure_intensities"),
           "connectivity": ("connectivity",)}
COMMON = ("enthalpy", "features", "accepted")


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _up(x):
    return (x + 255) & ~255


def _consumers(eng, obs, sc, cutoff):
    """Structure factors with two intensities, one graph, a minima record keyed by composition and a statistics record
    with one column of each source, on a handle whose observables are set: (structure spec, connectivity spec)."""
    sf = StructureFactor.from_supercell(sc, commensurate_points(sc)[:3], observables=obs, intensities=[(1, 0, 0), (2, 0, 1)])
    eng.set_structure_factor(sf)
    conn = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=cutoff)], observables=obs)
    eng.set_connectivity(conn)
    eng.set_minima(Minima.by_composition(obs, [1], extents=[sc.num_sites + 1]))
    eng.set_statistics(Statistics.per_walker([st.ENTHALPY, st.feature(0), st.kind(obs, 1), st.intensity(0),
                                              st.connectivity(0, cn.LARGEST)], n_levels=3))
    return sf, conn


def _block_bytes(eng, obs, flags):
    """Bytes the download of a block of NS samples moves: the 256-byte aligned columns whose flag is set."""
    rows = NS * eng.R
    K, S = obs.n_kinds, obs.n_shells
    Q, Ks, I = eng.structure_shape()
    G, _ = eng.connectivity_shape()
    size = _up(rows * 8) + _up(rows * eng.F * 8) + _up(rows)
    if flags.get("bias"):
        size += _up(rows * 8)
    if flags.get("wl"):
        size += _up(rows * 8) + 3 * _up(rows * eng.L * 8) + _up(rows * eng.L * eng.F * 8)
    if flags["occupancy"]:
        size += _up(rows * ((eng.N + 15) // 16 * 16))
    if flags["observables"]:
        size += _up(rows * K * 4) + _up(rows * S * K * K * 4)
    if flags["structure"]:
        size += _up(rows * Q * Ks * 16) + _up(rows * I * 8)
    if flags["connectivity"]:
        size += _up(rows * G * capi.CONN_STATS * 8)
    return size


def _derived_of(eng, occ):
    """The derived columns of occupancy rows (ns, R, N) by the eval_* calls, keyed as ``fetch_samples`` keys them."""
    ns, R, N = occ.shape
    flat = occ.reshape(-1, N)
    counts, pairs = eng.observables(flat)
    amp, inten = eng.structure_factor(flat)
    stats = eng.connectivity(flat)
    out = dict(species_counts=counts, pair_counts=pairs, structure_amplitudes=amp, structure_intensities=inten, connectivity=stats)
    return {k: v.reshape((ns, R) + v.shape[1:]) for k, v in out.items()}


def _offer_state(eng, min_rec, stat_rec):
    """One offer of the walkers' current states to the NumPy records, the derived columns by the eval_* calls."""
    s = eng.get_state()
    d = _derived_of(eng, s["occupancy"][None])
    min_rec.offer(s["enthalpy"], s["features"], s["occupancy"], d["species_counts"], s["n_steps"][None])
    stat_rec.offer(s["enthalpy"], s["features"], d["species_counts"], intensities=d["structure_intensities"],
                   connectivity=d["connectivity"])


def _offer_block(eng, min_rec, stat_rec, block, occ, derived):
    """The rows of a fetched block offered to the NumPy records; the step of a row from the walkers' counters now."""
    back = (NS - 1 - np.arange(NS)) * THIN
    steps = eng.get_state()["n_steps"][None, :] - back[:, None].astype(np.uint64)
    min_rec.offer(block["enthalpy"], block["features"], occ, derived["species_counts"], steps)
    stat_rec.offer(block["enthalpy"], block["features"], derived["species_counts"], intensities=derived["structure_intensities"],
                   connectivity=derived["connectivity"])


def _one_block(eng, obs, start, size_fn, flags, kw):
    """From the same state and seeds: one offer of the current states by update_*, then one block with ``flags``.  Returns
    (block, minima and statistics after the update, minima and statistics after the block)."""
    eng.reset_minima()
    eng.reset_statistics()
    start()
    eng.update_minima()
    eng.update_statistics()
    before = (eng.minima(), eng.statistics())
    eng.run_sampled_async(NS, THIN, **flags, **kw)
    assert size_fn(eng._h) == _block_bytes(eng, obs, {**flags, **kw}), flags
    block = eng.fetch_samples()
    return block, before, (eng.minima(), eng.statistics())


def _size_fn(eng):
    fn = eng._lib.smolmc_debug_block_bytes
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p]
    return fn


def test_every_subset_of_consumers_on_a_lean_handle(clean_env):
    R = 3
    eng, obs, sc = _semigrand("fcc3_indicator_skew", R)
    assert "lean" in eng.kernel_info() and sc.num_sites == 60, eng.kernel_info()
    _consumers(eng, obs, sc, 4.09 / np.sqrt(2.0) + 0.01)
    occ0 = _rand_occ(sc, np.random.default_rng(5), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(11)
    start = lambda: eng.set_state(occ0, seeds, 3000.0)  # noqa: E731
    size_fn = _size_fn(eng)
    minima_spec, stat_spec = eng.minima_spec, eng.statistics_spec
    new_records = lambda: (MinimaRecord(minima_spec, R, eng.F, eng.N, obs.n_kinds), StatisticsRecord(stat_spec, R))  # noqa: E731

    # the subset {minima, statistics} alone: what the records hold after the update and after the block
    none = dict.fromkeys(CONSUMERS, False)
    ref, ref_before, ref_after = _one_block(eng, obs, start, size_fn, dict(none, occupancy=True, minima=True, statistics=True), {})
    want_min, want_stat = new_records()
    start()
    _offer_state(eng, want_min, want_stat)
    _same_minima(ref_before[0], want_min, "update_minima")
    _same_statistics(ref_before[1], want_stat, "update_statistics")
    assert (ref_before[1].n == 1).all() and (ref_after[1].n == 1 + NS).all()
    assert len({ref["occupancy"][i].tobytes() for i in range(NS)}) == NS  # (the chain moves)
    ref_derived = _derived_of(eng, ref["occupancy"])
    # ... and the block's rows offered to the definition give the records after it
    eng.run(NS * THIN)  # (the counters where the block left them: the steps of the rows)
    _offer_block(eng, want_min, want_stat, ref, ref["occupancy"], ref_derived)
    _same_minima(ref_after[0], want_min, "minima alone")
    _same_statistics(ref_after[1], want_stat, "statistics alone")

    for subset in itertools.product((False, True), repeat=len(CONSUMERS)):
        with_occ = {}
        for occupancy in (True, False):
            flags = dict(zip(CONSUMERS, subset), occupancy=occupancy)
            what = str(flags)
            block, before, after = _one_block(eng, obs, start, size_fn, flags, {})
            for key in COMMON:
                np.testing.assert_array_equal(block[key], ref[key], err_msg=f"{what} {key}")
            if occupancy:
                np.testing.assert_array_equal(block["occupancy"], ref["occupancy"], err_msg=what)
                with_occ = block
            else:
                assert block["occupancy"] is None
            for name, keys in DERIVED.items():
                for key in keys:
                    assert (key in block) == flags[name], (what, key)
                    if flags[name]:
                        want = ref_derived[key] if occupancy else with_occ[key]
                        assert block[key].dtype == want.dtype and block[key].shape == want.shape, (what, key)
                        np.testing.assert_array_equal(block[key], want, err_msg=f"{what} {key}")
            _same_minima(before[0], ref_before[0], what + " update_minima")
            _same_statistics(before[1], ref_before[1], what + " update_statistics")
            _same_minima(after[0], ref_after[0] if flags["minima"] else ref_before[0], what + " minima")
            _same_statistics(after[1], ref_after[1] if flags["statistics"] else ref_before[1], what + " statistics")
    eng.close()


@pytest.mark.parametrize("which", ["lazy", "wang-landau"])
def test_none_and_all_consumers_on_the_other_recording_paths(which, clean_env):
    """Lazy cluster features (rows of scalar features, evaluated after the launch) and Wang-Landau (one snapshot per
    sample): a block without consumers, then from the same state one with all five whose occupancy rows stay on the device."""
    R = 3
    eng, obs, occ0, kw = _handle(which, R, clean_env)
    name = "rocksalt333_two_sublattices" if which == "lazy" else "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    _consumers(eng, obs, sc, 3.0)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(31)
    start = lambda: eng.set_state(occ0, seeds, 0.0 if which == "wang-landau" else 3000.0)  # noqa: E731
    size_fn = _size_fn(eng)
    want_min, want_stat = MinimaRecord(eng.minima_spec, R, eng.F, eng.N, obs.n_kinds), StatisticsRecord(eng.statistics_spec, R)

    plain, before0, after0 = _one_block(eng, obs, start, size_fn, dict(dict.fromkeys(CONSUMERS, False), occupancy=True), kw)
    start()
    _offer_state(eng, want_min, want_stat)
    _same_minima(before0[0], want_min, "update_minima")
    _same_statistics(before0[1], want_stat, "update_statistics")
    _same_minima(after0[0], before0[0], "no flag, no offer")
    _same_statistics(after0[1], before0[1], "no flag, no offer")
    derived = _derived_of(eng, plain["occupancy"])

    full, before1, after1 = _one_block(eng, obs, start, size_fn, dict(dict.fromkeys(CONSUMERS, True), occupancy=False), kw)
    assert full["occupancy"] is None and set(full) == set(plain) | set(derived)
    for key in plain:
        if key != "occupancy":
            np.testing.assert_array_equal(full[key], plain[key], err_msg=key)
    for key, want in derived.items():
        assert full[key].dtype == want.dtype and full[key].shape == want.shape, key
        np.testing.assert_array_equal(full[key], want, err_msg=key)
    _same_minima(before1[0], before0[0], "update_minima again")
    _same_statistics(before1[1], before0[1], "update_statistics again")
    _offer_block(eng, want_min, want_stat, full, plain["occupancy"], derived)
    _same_minima(after1[0], want_min, "minima")
    _same_statistics(after1[1], want_stat, "statistics")
    eng.close()
