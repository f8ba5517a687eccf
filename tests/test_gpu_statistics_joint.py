"""The joint field of a statistics record on the device (csrc/statistics.hip: mode 4 of statistics_kernel;
smolmc_set_statistics_joint, smolmc_statistics_joint_shape, smolmc_get_statistics_joint): joint and joint_out equal
``statistics.StatisticsRecord.offer``, the NumPy definition, fed with what the same blocks delivered -- exact integer
equality everywhere, no tolerance -- in the three key modes, on the release library and on the bounds library.  The
record's other arrays and a site field are compared along with it."""

import numpy as np
import pytest

from smol_amd import connectivity as cn
from smol_amd import statistics as st
from smol_amd.connectivity import Connectivity
from smol_amd.patterns import Patterns
from smol_amd.statistics import Statistics, StatisticsRecord
from tests.test_gpu_observables import _rand_occ
from tests.test_gpu_statistics import _semigrand
from tests.test_gpu_statistics_sites import SCATTERED, THIN, _codes, _run_blocks, lib  # noqa: F401  (lib: the fixture)
from tests.test_gpu_statistics_sites import _same as _same_with_sites

pytestmark = pytest.mark.gpu
SIZES = (1, 3, 20)
NN = 4.09 / np.sqrt(2.0)  # nearest-neighbour distance of the fcc cases (a = 4.09)


def _same(got, want, what=""):
    """Every array of the record, the site field and the joint field, and both identities."""
    _same_with_sites(got, want, what)
    for f in st._JOINT_ARRAYS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, g.shape, w.dtype, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {f}")
    np.testing.assert_array_equal(got.joint.sum(axis=(1, 2)) + got.joint_out, got.n, err_msg=f"{what} joint identity")


def _offer(rec, blocks, keys=None):
    for i, b in enumerate(blocks):
        rec.offer(b["enthalpy"], b["features"], b.get("species_counts"), None if keys is None else keys[i],
                  patterns=b.get("pattern_counts"), connectivity=b.get("connectivity"), occupancy=b["occupancy"])
    return rec


def _axis(values, n, pad=0.01):
    """(n, min, bin) of n cells that hold every one of ``values``."""
    lo, hi = float(np.min(values)), float(np.max(values))
    w = max(hi - lo, 1.0)
    return n, lo - pad * w, (1.0 + 2.0 * pad) * w / n


def _grid_handle(R):
    """A semigrand handle whose walkers hold different chemical potentials, so that their counts differ: (engine,
    observables, supercell, restart()), restart() putting every walker back to one start."""
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    rows = np.zeros(eng._mu_shape())
    rows[:, 0, 1] = np.linspace(-0.3, 0.3, R)
    temps = np.linspace(2500.0, 4000.0, R)
    occ0 = _rand_occ(sc, np.random.default_rng(5), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(11)

    def restart():
        eng.set_walker_mu(rows)  # (the walkers' points are named afresh: point p is walker p)
        eng.set_state(occ0, seeds, temps)

    return eng, obs, sc, restart


# ---- 1: by walker and by state point -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 70, 300])
def test_by_walker_and_by_state_point_equal_the_definition(R, lib):  # noqa: F811
    """Axes: the weighted-sum energy x a kind count.  64 x 64 cells that hold every row, then 5 x 3 cells whose count axis
    ends at the median of the walkers' largest counts: the definition's own record has joint_out > 0 on some keys and
    == 0 on others."""
    eng, obs, sc, restart = _grid_handle(R)
    nat = eng.natural_parameters
    cols = [st.ENERGY, st.kind(obs, 1), st.ENTHALPY]
    restart()
    dry = eng.run_sampled(sum(SIZES), THIN, observables=True)
    x = Statistics.per_walker(cols, weights=nat[:-1]).column_values(dry["enthalpy"], dry["features"], dry["species_counts"])
    E, N = x[..., 0], x[..., 1]
    top = np.sort(N.max(axis=0))[R // 2]  # the median of the walkers' largest counts
    fields = {"64 x 64": ((st.ENERGY,) + _axis(E, 64), (st.kind(obs, 1), 64, -0.5, (sc.num_sites + 1) / 64.0)),
              "5 x 3": ((st.ENERGY,) + _axis(E, 5), (st.kind(obs, 1), 3, float(N.min()) - 0.5, (top - float(N.min()) + 1.0) / 3.0))}
    for make in (Statistics.per_walker, Statistics.by_state_point):
        for what, joint in fields.items():
            spec = make(cols, weights=nat[:-1], n_levels=3, joint=joint)
            eng.set_statistics(spec)
            assert eng.statistics_joint_shape() == spec.c_joint()
            _same(eng.statistics(), StatisticsRecord(spec, R), "empty")
            restart()
            blocks = _run_blocks(eng, SIZES, observables=True)
            want = _offer(StatisticsRecord(spec, R), blocks)
            got = eng.statistics()
            _same(got, want, f"{make.__name__} {what}")
            assert (got.n == sum(SIZES)).all()
            if what == "64 x 64":
                assert not want.joint_out.any() and (want.joint.sum(axis=(1, 2)) == sum(SIZES)).all()
                assert (want.joint.sum(axis=0) > 0).sum() > 3
            else:
                assert (want.joint_out > 0).any() and (want.joint_out == 0).any(), want.joint_out
    eng.close()


def test_by_state_point_follows_the_exchanges(lib):  # noqa: F811
    R = 6
    eng, obs, sc, restart = _grid_handle(R)
    nat = eng.natural_parameters
    cols = [st.ENERGY, st.kind(obs, 1)]
    joint = ((st.ENERGY, 16, -40.0, 5.0), (st.kind(obs, 1), 32, -0.5, 8.0))
    even, odd = np.array([[0, 1], [2, 3], [4, 5]]), np.array([[1, 2], [3, 4]])
    fields = {}
    for what, make in (("point", Statistics.by_state_point), ("walker", Statistics.per_walker)):
        spec = make(cols, weights=nat[:-1], n_levels=2, joint=joint)
        restart()
        eng.set_statistics(spec)
        keys = []

        def exchange(i):
            if i > 0:  # every pair accepted: even pairs, then odd pairs, ...
                pairs = even if i % 2 else odd
                eng.exchange_grid(pairs, np.full(len(pairs), -np.inf))
            keys.append(eng.state_points()[0].copy())

        blocks = _run_blocks(eng, (3, 4, 2, 6, 5), thin=7, before_block=exchange, observables=True)
        assert not np.array_equal(keys[-1], np.arange(R)) and all(sorted(k) == list(range(R)) for k in keys)
        got = eng.statistics()
        _same(got, _offer(StatisticsRecord(spec, R), blocks, keys if what == "point" else None), what)
        fields[what] = got.joint
    # rows follow the state point, not the walker: the same rows in all, in other keys
    assert not np.array_equal(fields["point"], fields["walker"])
    np.testing.assert_array_equal(fields["point"].sum(axis=0), fields["walker"].sum(axis=0))
    eng.close()


# ---- 2: by bin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [70, 300])
def test_by_bin_equals_the_definition(R, lib):  # noqa: F811
    eng, obs, sc, restart = _grid_handle(R)
    Ns = sc.num_sites
    restart()
    dry = eng.run_sampled(sum(SIZES), THIN, observables=True)
    H, f1 = dry["enthalpy"], dry["features"][..., 1]  # (feature 0 is the empty cluster: one value)
    lo, hi = float(H.min()), float(H.max())
    w = hi - lo
    count, other = st.kind(obs, 1), st.kind(obs, 0)
    specs = {
        # keyed by composition: neighbouring rows in different keys; the axes are two other columns
        "composition": Statistics.by_composition(obs, 1, Ns, columns=[count, st.ENTHALPY, st.feature(1)],
                                                 joint=((st.ENTHALPY,) + _axis(H, 12), (st.feature(1),) + _axis(f1, 7))),
        # the middle half of the enthalpies in 4 bins: rows under and over the keys, and rows outside the 3 x 4 cells.  The
        # feature takes few values, each with its rounding noise, and its axis begins at their median: rows lie below min by
        # less than an ulp of the bin width, where the remainder of the exact floor division rounds to the width itself
        "four": Statistics.by_bin(st.ENTHALPY, 4, lo + 0.25 * w, w / 8, columns=[st.ENTHALPY, st.feature(1), count],
                                  joint=((st.feature(1), 3, float(np.median(f1)), float(f1.max() - np.median(f1)) / 2.0),
                                         (count, 4, -0.5, (Ns + 1) / 4.0))),
        # a single cell and a single key: every row of every wave goes to ONE counter
        "one cell": Statistics.by_bin(st.ENTHALPY, 1, lo - 1.0, w + 2.0, columns=[st.ENTHALPY, count, other],
                                      joint=((count, 1, -0.5, Ns + 1.0), (other, 1, -0.5, Ns + 1.0))),
        # a single cell under 4 keys: long runs of rows that share a counter, rows outside the keys between them
        "one cell, four keys": Statistics.by_bin(st.ENTHALPY, 4, lo + 0.25 * w, w / 8, columns=[st.ENTHALPY, count],
                                                 joint=((count, 1, -0.5, Ns + 1.0), (st.ENTHALPY, 1, lo - 1.0, w + 2.0))),
    }
    rows = sum(SIZES) * R
    for what, spec in specs.items():
        eng.set_statistics(spec)
        restart()
        blocks = _run_blocks(eng, SIZES, observables=True)
        got = eng.statistics()
        _same(got, _offer(StatisticsRecord(spec), blocks), what)
        assert got.n.sum() + got.key_under + got.key_over == rows
        if what == "composition":
            assert (got.n > 0).sum() > 8 and got.key_under == got.key_over == 0 and not got.joint_out.any()
        if what == "four":
            assert got.key_under > 0 and got.key_over > 0 and got.n.min() > 0 and got.joint_out.sum() > 0 and got.joint.sum() > 0
        if what.startswith("one cell"):
            assert got.joint.shape[1:] == (1, 1) and not got.joint_out.any()
            np.testing.assert_array_equal(got.joint[:, 0, 0], got.n)
        if what == "one cell":
            assert got.n[0] == rows
    eng.close()


# ---- 3: column sources and the ways to offer ---------------------------------------------------------------------------------
def test_pattern_and_connectivity_columns_go_through_the_shared_reader(lib):  # noqa: F811
    R = 70
    eng, obs, sc, restart = _grid_handle(R)
    pat = Patterns.from_tuples(obs, [np.arange(240, dtype=np.int32).reshape(80, 3)])  # (the model has pairs only: 80 triples of sites)
    con = Connectivity.from_supercell(sc, [dict(members=[1], cutoff=NN + 0.01)], observables=obs)
    eng.set_patterns(pat)
    eng.set_connectivity(con)
    restart()
    dry = eng.run_sampled(sum(SIZES), THIN, patterns=True, connectivity=True)
    cell = int(np.argmax(dry["pattern_counts"].reshape(-1, pat.n_cells).std(axis=0)))  # a cell that moves
    a, b = st.pattern(cell), st.connectivity(0, cn.LARGEST)
    joint = ((a,) + _axis(dry["pattern_counts"][..., cell], 9), (b,) + _axis(dry["connectivity"][..., 0, cn.LARGEST], 6))
    for spec in (Statistics.per_walker([st.ENTHALPY, a, b], n_levels=2, joint=joint),
                 Statistics.by_bin(st.ENTHALPY, 5, float(np.median(dry["enthalpy"])) - 10.0, 4.0, columns=[st.ENTHALPY, b, a], joint=joint)):
        eng.set_statistics(spec)
        restart()
        blocks = _run_blocks(eng, SIZES, patterns=True, connectivity=True)
        got = eng.statistics()
        _same(got, _offer(StatisticsRecord(spec, R), blocks), "pattern x connectivity")
        assert not got.joint_out.any() and (got.joint.sum(axis=0) > 0).sum() > 3
        # the same field with the two columns left on the device
        eng.set_statistics(spec)
        restart()
        for i, ns in enumerate(SIZES):
            eng.run_sampled_async(ns, THIN, occupancy=False, statistics=True)
            if i > 0:
                assert "pattern_counts" not in eng.fetch_samples()
        eng.fetch_samples()
        _same(eng.statistics(), got, "columns stay on the device")
    eng.close()


def test_site_field_update_reset_detach_and_attach(lib):  # noqa: F811
    R = 70
    eng, obs, sc, restart = _grid_handle(R)
    S, Ns = _codes(sc), sc.num_sites
    nat = eng.natural_parameters
    cols = [st.ENERGY, st.kind(obs, 1), st.ENTHALPY]
    joint = ((st.ENERGY, 16, -40.0, 5.0), (st.kind(obs, 1), 32, -0.5, 8.0))
    restart()
    lo = float(np.sort(eng.run_sampled(4, THIN)["enthalpy"].ravel())[2 * R])  # (a value that a row holds: the runs below repeat it)
    for spec in (Statistics.by_state_point(cols, weights=nat[:-1], n_levels=2, joint=joint, sites=SCATTERED, site_codes=S),
                 Statistics.by_bin(st.ENTHALPY, 6, lo - 6.0, 2.0, columns=cols, weights=nat[:-1], joint=joint, sites=None, site_codes=S - 1)):
        # a site field and a joint field together, both right
        eng.set_statistics(spec)
        assert eng.statistics_joint_shape() == spec.c_joint() and eng.statistics_sites_shape()[1] == spec.site_codes
        restart()
        blocks = _run_blocks(eng, SIZES, observables=True)
        want = _offer(StatisticsRecord(spec, R), blocks)
        got = eng.statistics()
        _same(got, want, "both fields")
        assert got.site_counts.any() and got.joint.any()
        # update_statistics offers the current states to both
        for n in (40, 1):
            eng.run(n)
            eng.update_statistics()
            s = eng.get_state()
            want.offer(s["enthalpy"], s["features"], obs.evaluate(s["occupancy"])[0], occupancy=s["occupancy"])
            _same(eng.statistics(), want, "update")
        # reset: the empty record with both fields empty and in force
        eng.reset_statistics()
        assert eng.statistics_joint_shape() == spec.c_joint()
        _same(eng.statistics(), StatisticsRecord(spec, R, Ns), "reset")
        # update_statistics alone, no sampled block
        eng.update_statistics()
        s = eng.get_state()
        alone = StatisticsRecord(spec, R).offer(s["enthalpy"], s["features"], obs.evaluate(s["occupancy"])[0], occupancy=s["occupancy"])
        _same(eng.statistics(), alone, "update alone")
        assert alone.joint.sum() + alone.joint_out.sum() + alone.key_under + alone.key_over == R
        # detach: the record and the site field stay, the joint field is gone
        before = eng.statistics()
        eng.set_statistics_joint(0, 0, 0.0, 0.0)
        assert eng.statistics_joint_shape() == (0, 0, 0.0, 0.0) * 2
        plain_kw = dict(weights=nat[:-1], sites=spec.sites, site_codes=spec.site_codes)
        eng.statistics_spec = (Statistics.by_bin(st.ENTHALPY, 6, spec.key_min, spec.key_bin, columns=cols, **plain_kw) if spec.binned
                               else Statistics.by_state_point(cols, n_levels=2, **plain_kw))
        detached = eng.statistics()
        assert detached.joint.shape == (detached.n_keys, 0, 0)
        for f in st._ARRAYS + st._SITE_ARRAYS:
            np.testing.assert_array_equal(getattr(detached, f), getattr(before, f), err_msg=f)
        eng.update_statistics()  # (a record without a joint field goes on as it did)
        # attach again, other cells: the field is zero, the moments and the site field go on
        before = eng.statistics()
        again = ((st.kind(obs, 1), 8, -0.5, 40.0), (st.kind(obs, 1), 4, -0.5, 80.0))  # (one column on both axes)
        respec = (Statistics.by_bin(st.ENTHALPY, 6, spec.key_min, spec.key_bin, columns=cols, joint=again, **plain_kw) if spec.binned
                  else Statistics.by_state_point(cols, n_levels=2, joint=again, **plain_kw))
        eng.set_statistics_joint(*respec.c_joint())
        eng.statistics_spec = respec
        assert eng.statistics_joint_shape() == (1, 8, -0.5, 40.0, 1, 4, -0.5, 80.0)
        after = eng.statistics()
        assert after.joint.shape[1:] == (8, 4) and not after.joint.any() and not after.joint_out.any()
        for f in st._ARRAYS + st._SITE_ARRAYS:
            np.testing.assert_array_equal(getattr(after, f), getattr(before, f), err_msg=f)
        eng.update_statistics()
        filled = eng.statistics()
        offered = filled.n - before.n
        np.testing.assert_array_equal(filled.joint.sum(axis=(1, 2)) + filled.joint_out, offered)
        qa, qb = np.nonzero(filled.joint.sum(axis=0))
        assert offered.sum() > 0 and (qb == qa // 2).all()
        # a new spec drops the field
        eng.set_statistics(Statistics.per_walker([st.ENTHALPY]))
        assert eng.statistics_joint_shape() == (0, 0, 0.0, 0.0) * 2 and eng.statistics_sites_shape() == (0, 0)
        eng.run_sampled(2, THIN, statistics=True)
        rec = eng.statistics()
        assert rec.joint.shape == (R, 0, 0) and (rec.n == 2).all()
    eng.close()


def test_refusals_leave_record_and_fields_alone(lib):  # noqa: F811
    from smol_amd.engine import EngineError

    R = 6
    eng, obs, sc, restart = _grid_handle(R)
    S = _codes(sc)
    err = (EngineError, ValueError)  # (the engine's wrapper raises ValueError for a message about a range)
    ok = (0, 4, -40.0, 20.0, 1, 8, -0.5, 33.0)
    with pytest.raises(err, match="statistics joint: no statistics record set"):
        eng.set_statistics_joint(*ok)
    assert eng.statistics_joint_shape() == (0, 0, 0.0, 0.0) * 2
    cols = [st.ENTHALPY, st.kind(obs, 1)]
    spec = Statistics.per_walker(cols, n_levels=2, joint=((cols[0],) + ok[1:4], (cols[1],) + ok[5:]), sites=SCATTERED, site_codes=S)
    assert spec.c_joint() == ok
    eng.set_statistics(spec)
    restart()
    blocks = [eng.run_sampled(4, THIN, statistics=True, observables=True)]
    before = eng.statistics()
    _same(before, _offer(StatisticsRecord(spec, R), blocks), "before")
    assert before.joint.sum() + before.joint_out.sum() == 4 * R

    def refused(match, *args):
        with pytest.raises(err, match=match):
            eng.set_statistics_joint(*args)
        assert eng.statistics_joint_shape() == ok and eng.statistics_sites_shape() == (5, S)
        _same(eng.statistics(), before, match)

    refused("n_a must be 0..65536, got 65537", 0, 65537, 0.0, 1.0, 1, 4, 0.0, 1.0)
    refused("n_a must be 0..65536, got -1", 0, -1, 0.0, 1.0, 1, 4, 0.0, 1.0)
    refused("n_b must be 1..65536, got 0", 0, 4, 0.0, 1.0, 1, 0, 0.0, 1.0)
    refused("n_b must be 1..65536, got 65537", 0, 4, 0.0, 1.0, 1, 65537, 0.0, 1.0)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused("bin_a must be a positive finite number and min_a finite", 0, 4, 0.0, bad, 1, 4, 0.0, 1.0)
        refused("bin_b must be a positive finite number and min_b finite", 0, 4, 0.0, 1.0, 1, 4, 0.0, bad)
    refused("bin_a must be a positive finite number and min_a finite", 0, 4, np.nan, 1.0, 1, 4, 0.0, 1.0)
    refused("bin_b must be a positive finite number and min_b finite", 0, 4, 0.0, 1.0, 1, 4, -np.inf, 1.0)
    refused("column_a = 2 is no index into the 2 columns", 2, 4, 0.0, 1.0, 1, 4, 0.0, 1.0)
    refused("column_b = -1 is no index into the 2 columns", 0, 4, 0.0, 1.0, -1, 4, 0.0, 1.0)
    # record plus both fields over 1 GiB: 6 keys x 65536 x 512 cells x 8 bytes = 1.5 GiB
    refused("6 keys x 65536 x 512 cells are larger than 1 GiB", 0, 65536, 0.0, 1.0, 1, 512, 0.0, 1.0)
    # a block recorded with the statistics flag still waits in the ring: neither attaching nor detaching
    eng.run_sampled_async(2, THIN, statistics=True, observables=True)
    for args in (ok, (0, 0, 0.0, 0.0)):
        with pytest.raises(err, match="smolmc_set_statistics_joint while a block recorded with SMOLMC_SAMPLE_STATISTICS waits in the ring"):
            eng.set_statistics_joint(*args)
    assert eng.statistics_joint_shape() == ok
    blocks.append(eng.fetch_samples())
    _same(eng.statistics(), _offer(StatisticsRecord(spec, R), blocks), "after the waiting block")
    # through Engine.set_statistics the record of the new spec is in force when the field is refused: the wrapper removes it
    big = Statistics.per_walker(cols, joint=((cols[0], 65536, 0.0, 1.0), (cols[1], 512, 0.0, 1.0)))
    with pytest.raises(err, match="larger than 1 GiB"):
        eng.set_statistics(big)
    assert eng.statistics_shape() == (0, 0, 0, 0) and eng.statistics_joint_shape() == (0, 0, 0.0, 0.0) * 2
    # the site field counts a joint field in force: 65536 keys x 64 x 16 cells x 8 bytes = 512 MiB, and 65536 keys x 256
    # sites x 4 codes x 8 bytes = 512 MiB
    eng.set_statistics(Statistics.by_bin(st.ENTHALPY, 65536, 0.0, 1.0, joint=((st.ENTHALPY, 64, 0.0, 1.0), (st.ENTHALPY, 16, 0.0, 1.0))))
    with pytest.raises(err, match="65536 keys x 256 sites x 4 codes are larger than 1 GiB"):
        eng.set_statistics_sites(None, 0, 4)
    assert eng.statistics_joint_shape()[1::4] == (64, 16) and eng.statistics_sites_shape() == (0, 0)
    eng.set_statistics_joint(0, 0, 0.0, 0.0)
    eng.set_statistics_sites(None, 0, 4)  # (without the joint field it fits)
    assert eng.statistics_sites_shape() == (256, 4)
    eng.close()


# ---- 4: the sampler: which state point a key of the record holds after run_exchange -------------------------------------------
def test_sampler_grid_state_points_name_the_keys_of_the_record(lib):  # noqa: F811
    """``Sampler.grid_state_points`` against the grid itself, and the record's keys against the ``state_point`` trace: key q of
    the record holds the rows of grid point ``_grid_base[q]``, on the first call (the identity) and on a call that begins
    from exchanged walkers."""
    from smol_amd import moca, synth
    from smol_amd.observables import Observables

    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 3.5})
    sc = synth.build_supercell(model, [3, 3, 3])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=5, scale=0.05))
    names = ens.species
    ens.chemical_potentials = {names[0]: 0.05, names[1]: -0.2, names[2]: 0.05}
    temps = [3000.0, 3600.0, 4500.0]
    shifts = np.linspace(-0.15, 0.15, 4)
    mus = [{names[0]: 0.05, names[1]: -0.2 + d, names[2]: 0.05} for d in shifts]
    nw = 12
    obs = Observables.from_supercell(sc)
    cols = [st.ENERGY, st.kind(obs, 1)]
    spec = Statistics.by_state_point(cols, weights=np.asarray(ens.natural_parameters)[:-1],
                                     joint=((st.ENERGY, 24, -30.0, 2.5), (st.kind(obs, 1), sc.size + 1, -0.5, 1.0)))
    sampler = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(11, 11 + nw)), observables=obs,
                                         statistics=spec)
    rng = np.random.default_rng(2)
    occ = np.zeros((nw, ens.num_sites), dtype=np.int32)
    occ[:, : sc.size] = rng.integers(0, 3, size=(nw, sc.size))

    def check(first_sample, what):
        gx, base = sampler._grid, sampler._grid_base
        betas, fields = sampler.grid_state_points()
        np.testing.assert_allclose(betas, 1.0 / (st.KB * gx.point_temperatures[base]), rtol=1e-15, err_msg=what)
        np.testing.assert_allclose(fields, np.tile(shifts, 3)[base] - 0.2 - 0.05, rtol=0, atol=1e-15, err_msg=what)
        np.testing.assert_allclose(fields, gx.point_rows[base][:, 0, 1] - gx.point_rows[base][:, 0, 0], rtol=0, atol=1e-15)
        c = sampler.samples
        point = c.get_trace_value("state_point", flat=False)[first_sample:, :, 0]
        key_of = np.empty(nw, dtype=np.int64)
        key_of[base] = np.arange(nw)  # grid point -> the engine's state point, the record's key
        want = StatisticsRecord(spec, nw).offer(
            c.get_trace_value("enthalpy", flat=False)[first_sample:, :, 0], c.get_feature_vectors(flat=False)[first_sample:],
            c.get_trace_value("species_counts", flat=False)[first_sample:], key_of_row=key_of[point])
        got = sampler.statistics
        np.testing.assert_array_equal(got.n, want.n, err_msg=what)
        np.testing.assert_array_equal(got.joint, want.joint, err_msg=what)
        np.testing.assert_array_equal(got.joint_out, want.joint_out, err_msg=what)
        assert got.joint.sum() > 0
        return base

    gx = sampler.run_exchange(8, 200, occ, thin_by=100, grid=dict(temperatures=temps, chemical_potentials=mus, seed=4))
    assert np.array_equal(check(0, "first call"), np.arange(nw))
    ln_g, f = sampler.grid_ln_g(tol=1e-8)
    assert ln_g.shape == (24, sc.size + 1) and np.isfinite(f).all() and np.isfinite(ln_g).any()
    # a second call begins from exchanged walkers and numbers the engine's state points afresh: the keys would mix
    assert not np.array_equal(gx.point_of, np.arange(nw))
    sampler.run_exchange(2, 200, thin_by=100)
    with pytest.raises(ValueError, match="reset_statistics\\(\\) before the second call"):
        sampler.grid_state_points()
    # emptied first, the record of the next call holds one state point per key again, under that call's numbering
    sampler.reset_statistics()
    before = sampler.samples.num_samples
    sampler.run_exchange(4, 200, thin_by=100)
    base = check(before, "after a reset")
    assert not np.array_equal(base, np.arange(nw)) and sorted(base) == list(range(nw))
