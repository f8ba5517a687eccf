"""The site field of a statistics record on the device (csrc/statistics.hip: mode 3 of statistics_kernel;
smolmc_set_statistics_sites, smolmc_statistics_sites_shape, smolmc_get_statistics_sites): site_counts and site_over equal
``statistics.StatisticsRecord.offer(..., occupancy=)``, the NumPy definition, fed with the occupancies the same block
delivered -- exact integer equality everywhere, no tolerance -- in the three key modes, on the release library and on the
bounds library.  The record's other arrays are compared along with the field."""

import os

import numpy as np
import pytest

from smol_amd import capi, engine, moca
from smol_amd import statistics as st
from smol_amd.statistics import Statistics, StatisticsRecord
from tests.cases import load_case
from tests.test_gpu_observables import ENV, _handle, _rand_occ
from tests.test_gpu_statistics import _semigrand

pytestmark = pytest.mark.gpu
THIN = 5
SCATTERED = [201, 3, 77, 255, 0]  # five sites of the 256, not ascending


@pytest.fixture(params=["release", "bounds"])
def lib(request, monkeypatch):
    path = engine.LIB_PATH if request.param == "release" else os.path.join(
        os.path.dirname(engine.LIB_PATH), "libsmolmc_hip_bounds.so")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: build() makes both libraries")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(engine, "_LIB", None)
    monkeypatch.setattr(engine, "LIB_PATH", path)
    yield monkeypatch
    engine._LIB = None


def _same(got, want, what=""):
    for f in st._ARRAYS + st._SITE_ARRAYS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, g.shape, w.dtype, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {f}")
    assert (got.key_under, got.key_over) == (want.key_under, want.key_over), what
    M = got.site_counts.shape[1]
    np.testing.assert_array_equal(got.site_counts.sum(axis=(1, 2)) + got.site_over, M * got.n, err_msg=f"{what} identity")


def _run_blocks(eng, sizes, thin=THIN, before_block=None, **kw):
    """Two blocks queued before the first fetch (the ring has two slots), then one queued per fetch: the fetched blocks in
    order.  Every block delivers its occupancies next to the offer."""
    out = []
    for i, ns in enumerate(sizes):
        if before_block is not None:
            before_block(i)
        eng.run_sampled_async(ns, thin, occupancy=True, statistics=True, **kw)
        if i > 0:
            out.append(eng.fetch_samples())
    out.append(eng.fetch_samples())
    return out


def _offer(rec, blocks, keys=None):
    for i, b in enumerate(blocks):
        rec.offer(b["enthalpy"], b["features"], b.get("species_counts"), None if keys is None else keys[i], occupancy=b["occupancy"])
    return rec


def _codes(sc):
    return int(max(sc.model.prim.nspecies))


# ---- 1: by walker ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 70, 300])
def test_by_walker_equals_the_definition(R, lib):
    """256 sites: all of them and five scattered ones, S the model's code count and one smaller (site_over fills).  At
    R = 3 one block has 300 samples: a thread's byte counters are flushed on the way."""
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    S = _codes(sc)
    occ0 = _rand_occ(sc, np.random.default_rng(5), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(11)
    sizes = (1, 3, 300) if R == 3 else (1, 3, 20)
    for sites in (None, SCATTERED):
        for codes in (S, S - 1):
            spec = Statistics.per_walker([st.ENTHALPY, st.feature(0)], n_levels=3, sites=sites, site_codes=codes)
            eng.set_statistics(spec)
            assert eng.statistics_sites_shape() == (sc.num_sites if sites is None else 5, codes)
            _same(eng.statistics(), StatisticsRecord(spec, R, sc.num_sites), "empty")
            eng.set_state(occ0, seeds, 3000.0)
            blocks = _run_blocks(eng, sizes)
            got = eng.statistics()
            _same(got, _offer(StatisticsRecord(spec, R), blocks), f"sites={sites} S={codes}")
            assert (got.n == sum(sizes)).all() and got.site_counts.any()
            assert (got.site_over.sum() > 0) == (codes < S)
    eng.close()


@pytest.mark.parametrize("name", ["fcc_prim222_aliased", "rocksalt333_two_sublattices"])
def test_rows_with_padding(name, lib):
    """8 and 54 sites: the ring's rows are padded to a multiple of 16 bytes, and the padding is no site."""
    R = 70
    eng, obs, sc = _semigrand(name, R)
    assert sc.num_sites % 16 != 0
    S = _codes(sc)
    eng.set_state(_rand_occ(sc, np.random.default_rng(4), R), np.arange(R, dtype=np.uint64) + np.uint64(2), 3000.0)
    for sites, codes in ((None, S), (None, S - 1), ([sc.num_sites - 1, 0, 2], S)):
        spec = Statistics.per_walker([st.ENTHALPY], sites=sites, site_codes=codes)
        eng.set_statistics(spec)
        blocks = _run_blocks(eng, (2, 9, 4))
        got = eng.statistics()
        _same(got, _offer(StatisticsRecord(spec, R), blocks), f"{name} sites={sites} S={codes}")
        assert got.site_counts.shape == (R, sc.num_sites if sites is None else 3, codes)
    eng.close()


def test_relabelled_handle_answers_in_the_callers_numbering(lib):
    """Restricted sites: smolmc_create renumbers the sites, the field's columns are the caller's."""
    from smol_amd.engine import Engine
    from tests.test_gpu_capi_relabel import _model

    sc, ens, tab, occ, frozen = _model(capi.STEP_SWAP)
    R, N = occ.shape
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    assert "relabelled=1" in eng.kernel_info(), eng.kernel_info()
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(9)
    scattered = [int(frozen[0]), N - 1, 5, int(frozen[-1]), 0]  # (frozen cations, an anion, not ascending)
    for sites, codes in ((None, 3), (scattered, 3), (scattered, 2)):
        spec = Statistics.per_walker([st.ENTHALPY], sites=sites, site_codes=codes)
        eng.set_statistics(spec)
        eng.set_state(occ, seeds, 4000.0)
        blocks = _run_blocks(eng, (2, 7, 3), thin=40)
        got = eng.statistics()
        _same(got, _offer(StatisticsRecord(spec, R), blocks), f"relabelled sites={sites} S={codes}")
        p = got.site_occupancy()
        if sites is None:  # a frozen site never changes, a free cation does
            assert set(np.unique(p[:, frozen])) <= {0.0, 1.0} and not set(np.unique(p[:, :sc.size])) <= {0.0, 1.0}
    # update_statistics reads the walkers' own rows through the same list
    eng.reset_statistics()
    eng.run(50)
    eng.update_statistics()
    s = eng.get_state()
    _same(eng.statistics(), StatisticsRecord(spec, R).offer(s["enthalpy"], s["features"], occupancy=s["occupancy"]), "update")
    eng.close()


# ---- 2: by state point -------------------------------------------------------------------------------------------------------
def test_by_state_point_follows_the_exchanges(lib):
    R = 6
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    rows = np.zeros(eng._mu_shape())
    rows[:, 0, 1] = np.linspace(-0.2, 0.2, R)
    temps = np.linspace(2500.0, 4000.0, R)
    occ0 = _rand_occ(sc, np.random.default_rng(9), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(21)
    even, odd = np.array([[0, 1], [2, 3], [4, 5]]), np.array([[1, 2], [3, 4]])
    fields = {}
    for what, make in (("point", Statistics.by_state_point), ("walker", Statistics.per_walker)):
        spec = make([st.ENTHALPY, st.feature(0)], n_levels=2, sites=None, site_codes=_codes(sc))
        eng.set_walker_mu(rows)  # (the walkers' points are named afresh: point p is walker p)
        eng.set_state(occ0, seeds, temps)
        eng.set_statistics(spec)
        keys = []

        def exchange(i):
            if i > 0:  # every pair accepted: even pairs, then odd pairs, ...
                pairs = even if i % 2 else odd
                eng.exchange_grid(pairs, np.full(len(pairs), -np.inf))
            keys.append(eng.state_points()[0].copy())

        blocks = _run_blocks(eng, (3, 4, 2, 6, 5), thin=7, before_block=exchange)
        assert not np.array_equal(keys[-1], np.arange(R)) and all(sorted(k) == list(range(R)) for k in keys)
        got = eng.statistics()
        _same(got, _offer(StatisticsRecord(spec, R), blocks, keys if what == "point" else None), what)
        fields[what] = got.site_counts
    assert not np.array_equal(fields["point"], fields["walker"])
    np.testing.assert_array_equal(fields["point"].sum(axis=0), fields["walker"].sum(axis=0))
    eng.close()


# ---- 3: by bin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [70, 300])
def test_by_bin_equals_the_definition(R, lib):
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    S = _codes(sc)
    occ0 = _rand_occ(sc, np.random.default_rng(5), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(11)
    sizes = (1, 3, 20)
    eng.set_state(occ0, seeds, 3000.0)
    H = eng.run_sampled(sum(sizes), THIN)["enthalpy"]
    lo, hi = float(H.min()), float(H.max())
    w, mid = hi - lo, float(np.median(H))
    specs = {
        # every row of every block in one key
        "one": Statistics.by_bin(st.ENTHALPY, 1, lo - 1.0, w + 2.0, sites=None, site_codes=S),
        # the middle half in 7 bins: long runs of rows per key, rows under and over
        "seven": Statistics.by_bin(st.ENTHALPY, 7, lo + 0.25 * w, w / 14, columns=[st.feature(0), st.ENTHALPY], sites=None, site_codes=S),
        # 257 bins over everything: neighbouring rows in different keys
        "spread": Statistics.by_bin(st.ENTHALPY, 257, lo - w / 256, w / 255, sites=None, site_codes=S - 1),
        # a window around the median so narrow that most rows fall under or over
        "narrow": Statistics.by_bin(st.ENTHALPY, 7, mid - 3.5 * w / 200, w / 200, sites=SCATTERED, site_codes=S),
        "narrow all": Statistics.by_bin(st.ENTHALPY, 7, mid - 3.5 * w / 200, w / 200, sites=None, site_codes=S),
    }
    for what, spec in specs.items():
        eng.set_statistics(spec)
        eng.set_state(occ0, seeds, 3000.0)
        blocks = _run_blocks(eng, sizes)
        got = eng.statistics()
        _same(got, _offer(StatisticsRecord(spec), blocks), what)
        rows = sum(sizes) * R
        assert got.n.sum() + got.key_under + got.key_over == rows
        if what == "one":
            assert got.n[0] == rows and got.site_counts.sum() == rows * sc.num_sites
        if what == "seven":
            assert got.key_under > 0 and got.key_over > 0 and got.n.min() > 0
        if what == "spread":
            assert (got.n > 0).sum() > 64 and got.site_over.sum() > 0
        if what.startswith("narrow"):
            assert 0 < got.n.sum() < rows // 4 and got.key_under > rows // 8 and got.key_over > rows // 8
    eng.close()


def test_wang_landau_levels_and_windows(lib):
    R = 6
    eng, obs, occ, kw = _handle("wang-landau", R, lib)
    cfg = eng.config
    spec = Statistics.on_wl_levels(cfg.wl_min_enthalpy, cfg.wl_bin_size, eng.L, columns=[st.ENTHALPY, st.feature(0)],
                                   sites=SCATTERED + [100, 101], site_codes=2)
    assert spec.n_keys == eng.L
    eng.set_statistics(spec)
    blocks = _run_blocks(eng, (2, 5, 9), thin=11, **kw)
    got = eng.statistics()
    _same(got, _offer(StatisticsRecord(spec), blocks), "levels")
    assert got.key_under == got.key_over == 0 and got.n.sum() == 16 * R and got.site_counts.sum() == 16 * R * 7
    # per-walker windows (the config's window for every walker: a valid set)
    vmin, vmax, _ = eng.wl_windows()
    eng.set_wl_windows(vmin, vmax)
    eng.set_statistics(spec)
    blocks = _run_blocks(eng, (3, 4), thin=11)  # (no Wang-Landau trace while windows are set)
    got = eng.statistics()
    _same(got, _offer(StatisticsRecord(spec), blocks), "windows")
    assert got.n.sum() == 7 * R
    # the readers on the device's record: the canonical field is a distribution over the codes on every site
    ln_g = np.where(got.n > 0, 1.0, np.nan)
    p = got.canonical_sites(ln_g, [800.0, 3000.0])
    assert p.shape == (2, 7, 2)
    np.testing.assert_allclose(p.sum(axis=2), 1.0, rtol=1e-12)
    eng.close()


# ---- 4: the ways to offer ----------------------------------------------------------------------------------------------------
def test_queued_blocks_update_reset_and_a_new_spec(lib):
    R = 70
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    S = _codes(sc)
    occ0 = _rand_occ(sc, np.random.default_rng(8), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(3)
    eng.set_state(occ0, seeds, 3000.0)
    H = eng.run_sampled(15, THIN)["enthalpy"]
    lo, hi = float(H.min()), float(H.max())
    for spec in (Statistics.per_walker([st.ENTHALPY], n_levels=2, sites=None, site_codes=S),
                 Statistics.by_bin(st.ENTHALPY, 7, lo + 0.25 * (hi - lo), (hi - lo) / 14, sites=None, site_codes=S)):
        # three blocks, each fetched before the next is queued ...
        eng.set_statistics(spec)
        eng.set_state(occ0, seeds, 3000.0)
        one_by_one = [eng.run_sampled(ns, THIN, statistics=True) for ns in (2, 9, 4)]
        want = _offer(StatisticsRecord(spec, R), one_by_one)
        _same(eng.statistics(), want, "one by one")
        # ... and queued ahead of the fetches, as far as the ring's two slots let a caller: the same field
        eng.set_statistics(spec)
        eng.set_state(occ0, seeds, 3000.0)
        queued = _run_blocks(eng, (2, 9, 4))
        for a, b in zip(one_by_one, queued):
            assert np.array_equal(a["occupancy"], b["occupancy"])
        _same(eng.statistics(), want, "queued")
        # the same record with the rows left on the device: nothing but the statistics asked for
        eng.set_statistics(spec)
        eng.set_state(occ0, seeds, 3000.0)
        for i, ns in enumerate((2, 9, 4)):
            eng.run_sampled_async(ns, THIN, occupancy=False, statistics=True)
            if i > 0:
                assert eng.fetch_samples()["occupancy"] is None
        assert eng.fetch_samples()["occupancy"] is None
        _same(eng.statistics(), want, "rows stay on the device")
        # update_statistics after run: one offer of the walkers' current states
        for n in (40, 1):
            eng.run(n)
            eng.update_statistics()
            s = eng.get_state()
            want.offer(s["enthalpy"], s["features"], occupancy=s["occupancy"])
            _same(eng.statistics(), want, "update")
        # reset: the empty record and the empty field, which fill again
        eng.reset_statistics()
        assert eng.statistics_sites_shape() == (sc.num_sites, S)
        _same(eng.statistics(), StatisticsRecord(spec, R, sc.num_sites), "reset")
        eng.update_statistics()
        s = eng.get_state()
        _same(eng.statistics(), StatisticsRecord(spec, R).offer(s["enthalpy"], s["features"], occupancy=s["occupancy"]), "after reset")
        # attaching a field again zeroes the field and leaves the record's other arrays
        before = eng.statistics()
        eng.set_statistics_sites(np.array(SCATTERED, dtype=np.int32), 5, S)
        assert eng.statistics_sites_shape() == (5, S)
        eng.statistics_spec = Statistics.per_walker([st.ENTHALPY], n_levels=2, sites=SCATTERED, site_codes=S) if not spec.binned else \
            Statistics.by_bin(st.ENTHALPY, 7, spec.key_min, spec.key_bin, sites=SCATTERED, site_codes=S)
        after = eng.statistics()
        assert not after.site_counts.any() and not after.site_over.any()
        for f in st._ARRAYS:
            np.testing.assert_array_equal(getattr(after, f), getattr(before, f), err_msg=f)
        # n_codes = 0 detaches it
        eng.set_statistics_sites(None, 0, 0)
        assert eng.statistics_sites_shape() == (0, 0)
        # a new spec drops the field: a new spec starts an empty record
        eng.set_statistics(spec)
        assert eng.statistics_sites_shape() == (sc.num_sites, S)
        plain = Statistics.per_walker([st.ENTHALPY])
        eng.set_statistics(plain)
        assert eng.statistics_sites_shape() == (0, 0)
        eng.run_sampled(2, THIN, statistics=True)
        rec = eng.statistics()
        assert rec.site_counts.shape == (R, 0, 0) and (rec.n == 2).all()
    eng.close()


def test_refusals_leave_record_and_field_alone(lib):
    from smol_amd.engine import EngineError

    R = 6
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    N, S = sc.num_sites, _codes(sc)
    err = (EngineError, ValueError)  # (the engine's wrapper raises ValueError for a message about a range)
    with pytest.raises(err, match="statistics sites: no statistics record set"):
        eng.set_statistics_sites(None, 0, S)
    assert eng.statistics_sites_shape() == (0, 0)
    spec = Statistics.per_walker([st.ENTHALPY], n_levels=2, sites=SCATTERED, site_codes=S)
    eng.set_statistics(spec)
    eng.set_state(_rand_occ(sc, np.random.default_rng(8), R), np.arange(R, dtype=np.uint64), 3000.0)
    eng.run_sampled(4, THIN, statistics=True)
    before = eng.statistics()
    assert before.site_counts.sum() == 4 * R * 5

    def refused(match, sites, n_codes):
        a = None if sites is None else np.asarray(sites, dtype=np.int32)
        with pytest.raises(err, match=match):
            eng.set_statistics_sites(a, 0 if a is None else len(a), n_codes)
        assert eng.statistics_sites_shape() == (5, S)
        _same(eng.statistics(), before, match)

    refused(f"entry 2 is site {N}, outside 0..{N - 1}", [0, 1, N], S)
    refused(f"entry 0 is site -1, outside 0..{N - 1}", [-1, 1], S)
    refused("site 7 is listed twice \\(entries 1 and 3\\)", [0, 7, 2, 7], S)
    refused("n_codes must be 0..16, got 17", None, 17)
    refused("n_codes must be 0..16, got -1", [0, 1], -1)
    # a block recorded with the statistics flag still waits in the ring
    eng.run_sampled_async(2, THIN, statistics=True)
    with pytest.raises(err, match="smolmc_set_statistics_sites while a block recorded with SMOLMC_SAMPLE_STATISTICS waits in the ring"):
        eng.set_statistics_sites(None, 0, S)
    assert eng.statistics_sites_shape() == (5, S)
    b = eng.fetch_samples()
    before.offer(b["enthalpy"], b["features"], occupancy=b["occupancy"])
    _same(eng.statistics(), before, "after the waiting block")
    # through Engine.set_statistics the record of the new spec is in force when the field is refused: the wrapper removes it
    with pytest.raises(err, match="listed twice"):
        eng.set_statistics(Statistics.per_walker([st.ENTHALPY], sites=[1, 1], site_codes=S))
    assert eng.statistics_shape() == (0, 0, 0, 0) and eng.statistics_sites_shape() == (0, 0)
    # record plus field over 1 GiB: 65536 keys x 256 sites x 16 codes x 8 bytes
    big = Statistics.by_bin(st.ENTHALPY, 65536, 0.0, 1.0)
    eng.set_statistics(big)
    with pytest.raises(err, match="65536 keys x 256 sites x 16 codes are larger than 1 GiB"):
        eng.set_statistics_sites(None, 0, 16)
    assert eng.statistics_sites_shape() == (0, 0) and eng.statistics_shape() == (65536, 1, 0, 0)
    eng.close()


# ---- 5: the chain is untouched -----------------------------------------------------------------------------------------------
def test_chains_do_not_change(lib):
    for which in ("lean", "lazy", "wang-landau"):
        got = []
        for with_field in (False, True):
            eng, obs, occ, kw = _handle(which, 5, lib)
            field = dict(sites=None, site_codes=2) if with_field else {}
            eng.set_statistics(Statistics.by_bin(st.ENTHALPY, 50, -500.0, 20.0, columns=[st.ENTHALPY, st.feature(0)], **field))
            eng.run(13)
            eng.run_sampled_async(4, 9, statistics=True, **kw)
            blocks = [eng.fetch_samples(), eng.run_sampled(2, 5, statistics=True, **kw)]
            got.append((blocks, eng.get_state(), eng.statistics()))
            eng.close()
        (plain, st0, rec0), (kept, st1, rec1) = got
        for p, c in zip(plain, kept):
            assert set(p) == set(c)
            for key in p:
                assert np.array_equal(p[key], c[key]), (which, key)
        for key in st0:
            assert np.array_equal(st0[key], st1[key]), (which, key)
        for f in st._ARRAYS:
            np.testing.assert_array_equal(getattr(rec0, f), getattr(rec1, f), err_msg=f"{which} {f}")
        _same(rec1, _offer(StatisticsRecord(rec1.spec), kept), which)


# ---- 6: the sampler ----------------------------------------------------------------------------------------------------------
def test_sampler_without_occupancies_keeps_the_same_field(lib):
    c = load_case("rocksalt333_two_sublattices")
    sc = c["sc"]
    nw, T = 6, 3000.0
    ens = moca.Ensemble.from_cluster_expansion(sc, c["coefs"])
    ens.chemical_potentials = {sp: 0.1 * (i - 1) for i, sp in enumerate(ens.species)}
    spec = Statistics.per_walker([st.ENTHALPY], n_levels=3, sites=None, site_codes=_codes(sc))
    occ = _rand_occ(sc, np.random.default_rng(12), nw)
    recs = {}
    for keep in (True, False):
        s = moca.Sampler.from_ensemble(ens, temperature=T, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                       statistics=spec)
        s.run(40 * 9, occ, thin_by=9, keep_occupancy=keep)
        s.run(25 * 9, thin_by=9, keep_occupancy=keep)  # (a second run: the record goes on)
        recs[keep] = s.statistics
        if keep:
            H = s.samples.get_trace_value("enthalpy", flat=False)[:, :, 0]
            want = StatisticsRecord(spec, nw).offer(H, s.samples.get_feature_vectors(flat=False),
                                                    occupancy=s.samples.get_occupancies(flat=False))
            _same(recs[keep], want, "sampler")
        else:
            with pytest.raises(ValueError, match="keep_occupancy=False"):
                s.samples.get_occupancies()
    _same(recs[False], recs[True], "keep_occupancy=False")
    p = recs[False].site_occupancy()
    assert p.shape == (nw, sc.num_sites, _codes(sc)) and (recs[False].n == 65).all()
    assert np.isfinite(recs[False].frozen_order()).all()
    s.reset_statistics()
    assert not s.statistics.site_counts.any()
