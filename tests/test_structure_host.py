"""Structure factors on the host (smol_amd/structure.py): the geometry of ``from_supercell`` against exp(-2 pi i k.r), the
fixed-point definition against the floating sum with its derived bound, exact known answers, Parseval, the inverse transform
against the observables' pair counts, validation, the ctypes mirror and the statistics columns fed by intensities."""

import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from smol_amd import capi, statistics as st
from smol_amd.observables import Observables
from smol_amd.structure import StructureFactor, _adjugate, commensurate_points, lattice_points_of
from tests.cases import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = 36
EPS = np.finfo(np.float64).eps
GEOMETRY = ["fcc3_indicator_skew", "fcc_conv444_pairs", "fcc_prim222_aliased", "rocksalt333_two_sublattices"]


def _rand_occ(sc, rng, n):
    nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    return (rng.random((n, sc.num_sites)) * nsp).astype(np.int32)


def _exact_phases(sc, g):
    """exp(-2 pi i k.r_j) (Q, N) with k = S^-1 g and r_j = n_j + tau_b: k.r_j is reduced modulo 1 as a rational number
    (the basis offsets of these cells are binary fractions), so the reference carries the error of one cos / sin only."""
    adj, det = _adjugate(sc.scmatrix)
    n = lattice_points_of(sc)
    P = len(n)
    tau = [[Fraction(float(x)) for x in row] for row in sc.model.prim.frac_coords]
    out = np.empty((len(g), sc.num_sites), dtype=np.complex128)
    for q, gq in enumerate(g):
        ag = [int(x) for x in adj @ gq]                       # det x k
        for j in range(sc.num_sites):
            r = [int(n[j % P][a]) + tau[int(sc.site_b[j])][a] for a in range(3)]
            t = sum(Fraction(ag[a], det) * r[a] for a in range(3)) % 1
            out[q, j] = np.exp(-2j * np.pi * float(t))
    return out


@pytest.fixture(scope="module")
def all_points():
    """name -> (sc, StructureFactor at every class representative, exact phases)"""
    out = {}
    for name in GEOMETRY:
        sc = load_case(name)["sc"]
        g = commensurate_points(sc)
        out[name] = (sc, StructureFactor.from_supercell(sc, g, bits=BITS), _exact_phases(sc, g))
    return out


# ---- 1. the phase formula ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOMETRY)
def test_phase_classes_and_tables_give_the_exact_phase(name, all_points):
    sc, sf, exact = all_points[name]
    D = abs(_adjugate(sc.scmatrix)[1])
    assert sf.n_points == D == sc.size and sf.phase.dtype == np.uint16 and sf.table.dtype == np.int64
    assert np.array_equal(sf.points[0], [0, 0, 0])
    q = np.arange(D)[:, None]
    got = sf.table[q, sf.phase, 0] * 2.0 ** -BITS + 1j * sf.table[q, sf.phase, 1] * 2.0 ** -BITS
    dev = np.abs(got - exact).max()
    bound = 2.0 ** -(BITS + 1) * np.sqrt(2) + 8 * EPS
    print(name, "M", sf.n_phases, "largest deviation", dev, "bound", bound)
    assert dev <= bound
    # the representatives are distinct classes: no two g differ by a combination of the columns of S
    adjT, detT = _adjugate(np.asarray(sc.scmatrix).T)
    keys = {tuple(int(x) for x in (np.sign(detT) * (gq @ adjT)) % D) for gq in sf.points}
    assert len(keys) == D


def test_fractional_points_are_checked_to_be_commensurate():
    sc = load_case("fcc_prim222_aliased")["sc"]
    a = StructureFactor.from_supercell(sc, np.array([[0.5, 0.0, 0.5]]))
    b = StructureFactor.from_supercell(sc, np.array([[1, 0, 1]]))
    np.testing.assert_array_equal(a.phase, b.phase)
    np.testing.assert_array_equal(a.table, b.table)
    with pytest.raises(ValueError, match="not commensurate"):
        StructureFactor.from_supercell(sc, np.array([[0.25, 0.0, 0.0]]))


def test_mson_style_supercell_gives_the_same_phases():
    """An ``mson`` supercell keeps pymatgen's fractional lattice points and no ``site_t``: same phases as the synth one."""
    import types

    sc = load_case("fcc3_indicator_skew")["sc"]
    g = commensurate_points(sc)[:7]
    inv = np.linalg.inv(sc.scmatrix.astype(np.float64))
    like = types.SimpleNamespace(scmatrix=sc.scmatrix, lattice_points=sc.lattice_points @ inv, site_b=sc.site_b, model=sc.model,
                                 num_sites=sc.num_sites, size=sc.size)
    a, b = StructureFactor.from_supercell(sc, g), StructureFactor.from_supercell(like, g)
    np.testing.assert_array_equal(a.phase, b.phase)
    np.testing.assert_array_equal(a.table, b.table)
    np.testing.assert_array_equal(a.kind_base, b.kind_base)


# ---- 2. fixed point against floating point ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOMETRY)
def test_fixed_point_agrees_with_the_float_sum_to_the_derived_bound(name, all_points):
    sc, sf, exact = all_points[name]
    rng = np.random.default_rng(5)
    occ = _rand_occ(sc, rng, 4)
    amp, inten = sf.evaluate(occ)
    assert amp.dtype == np.int64 and amp.shape == (4, sf.n_points, sf.n_kinds, 2) and inten.shape == (4, 0)
    A = sf.amplitudes(amp)
    kinds = sf.kinds_of(occ)
    worst = 0.0
    for k in range(sf.n_kinds):
        sel = kinds == k                                          # (4, N)
        ref = (sel[:, None, :] * exact[None]).sum(axis=-1)         # (4, Q)
        n_kind = sel.sum(axis=-1)[:, None]
        bound = n_kind * 2.0 ** -(BITS + 1) * np.sqrt(2) + 4 * n_kind * EPS
        dev = np.abs(A[:, :, k] - ref)
        worst = max(worst, float(dev.max()))
        assert np.all(dev <= bound), (k, float(dev.max()), float(bound.min()))
    print(name, "largest |A_fixed - A_float|", worst)


# ---- 3. an exact known answer -------------------------------------------------------------------------------------------------
def test_species_equal_to_a_two_class_phase_gives_exact_amplitudes():
    sc = load_case("fcc_prim666_triplets")["sc"]
    g = commensurate_points(sc)
    sf = StructureFactor.from_supercell(sc, g, bits=BITS)
    # a point with two phase classes of angles 0 and pi: g = (3, 0, 0) on the 6 x 6 x 6 cell
    q = int(np.flatnonzero((g == [3, 0, 0]).all(axis=1))[0])
    used = np.unique(sf.phase[q])
    assert len(used) == 2
    np.testing.assert_array_equal(sf.table[q, used], [[1 << BITS, 0], [-(1 << BITS), 0]])
    occ = (sf.phase[q] == used[1]).astype(np.int32)              # species = phase class
    n0, n1 = int((occ == 0).sum()), int((occ == 1).sum())
    amp, _ = sf.evaluate(occ)
    np.testing.assert_array_equal(amp[q, 0], [n0 << BITS, 0])
    np.testing.assert_array_equal(amp[q, 1], [-(n1 << BITS), 0])
    # Gamma counts the kinds
    np.testing.assert_array_equal(amp[0], [[n0 << BITS, 0], [n1 << BITS, 0]])


# ---- 4. Parseval ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc3_indicator_skew", "fcc_prim222_aliased"])
def test_parseval_over_all_class_representatives(name, all_points):
    sc, sf, _ = all_points[name]
    assert sc.model.prim.nb == 1
    occ = _rand_occ(sc, np.random.default_rng(9), 3)
    amp, _ = sf.evaluate(occ)
    A = sf.amplitudes(amp)                                         # (3, Q, K)
    D = sf.n_points
    n_kind = np.stack([(sf.kinds_of(occ) == k).sum(axis=-1) for k in range(sf.n_kinds)], axis=-1)  # (3, K)
    total = (np.abs(A) ** 2).sum(axis=1)
    # |A| <= n and |A_fixed - A_exact| <= e = n 2^-(bits+1) sqrt 2: every |A|^2 is off by at most 2 n e + e^2, D of them
    e = n_kind * 2.0 ** -(BITS + 1) * np.sqrt(2) + 4 * n_kind * EPS
    bound = D * (2 * n_kind * e + e * e) + 8 * D * n_kind ** 2 * EPS
    assert np.all(np.abs(total - D * n_kind) <= bound), np.abs(total - D * n_kind).max()


# ---- 5. the inverse transform against the observables' pair counts -------------------------------------------------------------
def test_inverse_transform_equals_the_symmetrised_pair_counts():
    sc = load_case("fcc_prim666_triplets")["sc"]
    obs = Observables.from_supercell(sc)
    assert obs.n_shells == 4
    sf = StructureFactor.from_supercell(sc, commensurate_points(sc), observables=obs, bits=BITS)
    occ = (np.random.default_rng(3).random((2, sc.num_sites)) < 0.4).astype(np.int32)
    _, pairs = obs.evaluate(occ)
    amp, _ = sf.evaluate(occ)
    n = lattice_points_of(sc)[np.asarray(sc.site_t)]
    adj, det = _adjugate(sc.scmatrix)
    D = abs(det)
    directed = []
    for sh, rows in enumerate(obs.shells):
        d = n[rows[:, 1]] - n[rows[:, 0]]
        # the classes of the shell's displacements modulo the supercell and their negatives: one representative each
        key = (np.sign(det) * (d @ adj)) % D
        both, first = np.unique(np.concatenate([key, (-key) % D]), axis=0, return_index=True)
        reps = np.concatenate([d, -d])[first]
        directed.append(len(both))
        got = sf.pair_counts_from_amplitudes(amp, reps).sum(axis=-3)         # (2, K, K)
        want = pairs[:, sh].astype(np.int64) + np.swapaxes(pairs[:, sh], -1, -2)
        assert np.abs(got - np.rint(got)).max() < 1e-6
        np.testing.assert_array_equal(np.rint(got).astype(np.int64), want)
    assert directed == [12, 6, 24, 12]


# ---- 6. validation, the ctypes mirror, the ABI version ----------------------------------------------------------------------------
def test_validation_errors():
    kb = np.zeros(6, dtype=np.int32)
    ph = np.zeros((2, 6), dtype=np.int64)
    tb = np.ones((2, 3, 2), dtype=np.int64)
    StructureFactor(kb, 2, ph, tb, [(1, 0, 1)])
    with pytest.raises(ValueError, match="1-D integer"):
        StructureFactor(kb.astype(float), 2, ph, tb)
    with pytest.raises(ValueError, match="n_kinds must be"):
        StructureFactor(kb, 255, ph, tb)
    with pytest.raises(ValueError, match="kind out of range"):
        StructureFactor(kb + 2, 2, ph, tb)
    with pytest.raises(ValueError, match="kind out of range"):
        StructureFactor(kb, 2, ph, tb, site_ncodes=np.full(6, 3))
    bad = ph.copy()
    bad[1, 4] = 3
    with pytest.raises(ValueError, match="phase holds 3, n_phases is 3: phase out of range"):
        StructureFactor(kb, 2, bad, tb)
    with pytest.raises(ValueError, match=r"phase must be a \(n_points, 6\)"):
        StructureFactor(kb, 2, ph[:, :5], tb)
    with pytest.raises(ValueError, match="table must be"):
        StructureFactor(kb, 2, ph, tb[:1])
    with pytest.raises(ValueError, match="n_points must be"):
        StructureFactor(kb, 2, np.zeros((capi.MAX_STRUCT_POINTS + 1, 6), np.int64), np.ones((capi.MAX_STRUCT_POINTS + 1, 1, 2), np.int64))
    with pytest.raises(ValueError, match="larger than MAX_CELLS"):
        StructureFactor(kb, 2, ph, np.ones((2, capi.MAX_STRUCT_CELLS // 2 + 1, 2), np.int64))
    with pytest.raises(ValueError, match="point out of range"):
        StructureFactor(kb, 2, ph, tb, [(2, 0, 0)])
    with pytest.raises(ValueError, match="kind out of range"):
        StructureFactor(kb, 2, ph, tb, [(0, 0, 2)])
    with pytest.raises(ValueError, match="intensity_scale must be finite"):
        StructureFactor(kb, 2, ph, tb, [(0, 0, 1)], intensity_scale=np.inf)
    with pytest.raises(ValueError, match="reaches 2\\^62"):
        StructureFactor(kb, 2, ph, tb * (1 << 60))
    StructureFactor(kb, 2, ph, tb * ((1 << 62) // 6))   # 6 x floor(2^62 / 6) < 2^62
    sf = StructureFactor(kb, 2, ph, tb, [(1, 0, 1)])
    with pytest.raises(ValueError, match="kind out of range"):
        sf.evaluate(np.full(6, 2))
    with pytest.raises(ValueError, match="6 sites in the last axis"):
        sf.evaluate(np.zeros(5, dtype=np.int32))
    # the default scale: 1 / N_counted without bits, 2^(-2 bits) / N_counted with them
    assert sf.intensity_scale[0] == 1.0 / 6
    assert StructureFactor(kb, 2, ph, tb, [(1, 0, 1)], bits=10).intensity_scale[0] == 2.0 ** -20 / 6


def test_intensities_are_products_of_amplitudes_rounded_one_by_one():
    sc = load_case("fcc3_indicator_skew")["sc"]
    g = commensurate_points(sc)[:9]
    its = [(q, a, b) for q in (0, 3, 8) for a in range(3) for b in range(a, 3)]
    sf = StructureFactor.from_supercell(sc, g, intensities=its, bits=BITS)
    N = sc.num_sites
    assert sf.n_intensities == len(its) and np.all(sf.intensity_scale == 2.0 ** (-2 * BITS) / N)
    occ = _rand_occ(sc, np.random.default_rng(2), 5).reshape(5, 1, N)
    amp, inten = sf.evaluate(occ)
    assert amp.shape == (5, 1, 9, 3, 2) and inten.shape == (5, 1, len(its))
    for i, (q, a, b) in enumerate(its):
        for r in range(5):
            x, y = amp[r, 0, q, a], amp[r, 0, q, b]
            want = (float(x[0]) * float(y[0]) + float(x[1]) * float(y[1])) * sf.intensity_scale[i]
            assert inten[r, 0, i] == want
    # ... and they are the partial structure factors
    S = sf.partial_structure_factors(amp)
    for i, (q, a, b) in enumerate(its):
        np.testing.assert_allclose(inten[..., i], S[..., q, a, b], rtol=1e-12, atol=1e-12)


def test_ctypes_mirror_matches_the_header_and_the_abi_stays_8():
    import subprocess
    import tempfile

    fields = [n for n, _ in capi.smolmc_structure._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "smolmc.h"\nint main(){printf("%zu", sizeof(smolmc_structure));\n' +
           "".join(f'printf(" %zu", offsetof(smolmc_structure, {f}));\n' for f in fields) +
           'printf(" %d %d %d %d %d %d\\n", SMOLMC_SAMPLE_STRUCTURE, SMOLMC_MAX_STRUCT_POINTS, SMOLMC_MAX_STRUCT_PHASES, '
           "SMOLMC_MAX_STRUCT_CELLS, SMOLMC_MAX_STRUCT_INTENSITIES, SMOLMC_ABI_VERSION);return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"), os.path.join(d, "p.c")])
        vals = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    T = capi.smolmc_structure
    assert vals == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields] + [
        capi.SAMPLE_STRUCTURE, capi.MAX_STRUCT_POINTS, capi.MAX_STRUCT_PHASES, capi.MAX_STRUCT_CELLS, capi.MAX_STRUCT_INTENSITIES, 8]
    assert capi.SAMPLE_STRUCTURE == 64 and capi.ABI_VERSION == 8
    from smol_amd import structure

    assert (structure.MAX_POINTS, structure.MAX_PHASES, structure.MAX_CELLS, structure.MAX_INTENSITIES) == (
        capi.MAX_STRUCT_POINTS, capi.MAX_STRUCT_PHASES, capi.MAX_STRUCT_CELLS, capi.MAX_STRUCT_INTENSITIES)
    hdr = open(os.path.join(ROOT, "include", "smolmc.h")).read()
    assert re.search(r"#define SMOLMC_ABI_VERSION 8\b", hdr)
    # c_struct points at the object's own arrays
    sf = StructureFactor(np.zeros(4, np.int32), 2, np.zeros((3, 4), np.int64), np.ones((3, 2, 2), np.int64), [(2, 1, 0)])
    s, keep = sf.c_struct()
    assert (s.n_kinds, s.n_points, s.n_phases, s.n_intensities) == (2, 3, 2, 1)
    assert [s.intensity[i] for i in range(3)] == [2, 1, 0] and s.table[11] == 1 and s.phase[11] == 0 and len(keep) == 5


# ---- 7. statistics with intensity columns --------------------------------------------------------------------------------------
def test_statistics_columns_fed_by_intensities():
    rng = np.random.default_rng(11)
    ns, R, F, K, I = 5, 4, 3, 2, 3
    H, f = rng.normal(size=(ns, R)), rng.normal(size=(ns, R, F))
    cnt, inten = rng.integers(0, 9, size=(ns, R, K)), rng.random((ns, R, I))
    spec = st.Statistics.per_walker(columns=(st.ENTHALPY, st.intensity(0), st.intensity(2), st.kind(K, 1), st.ENERGY),
                                    weights=np.array([0.5, -1.0]), n_levels=3, hist=(st.intensity(2), 8, 0.0, 0.125))
    np.testing.assert_array_equal(spec.sources(F, K, I), [0, 2 + F + K, 4 + F + K, 1 + F + 1, 1 + F + K])
    assert spec.intensity_columns() == [1, 2] and spec.count_columns() == [3]
    x = spec.column_values(H, f, cnt, inten)
    np.testing.assert_array_equal(x[..., 1], inten[..., 0])
    np.testing.assert_array_equal(x[..., 2], inten[..., 2])
    np.testing.assert_array_equal(x[..., 3], cnt[..., 1].astype(float))
    s, keep = spec.c_struct(F, K, I)
    assert [s.columns[i] for i in range(5)] == [0, 7, 9, 5, 6] and s.hist_column == 2
    with pytest.raises(ValueError, match="outside the 2 intensities"):
        spec.sources(F, K, 2)
    with pytest.raises(ValueError, match="outside the 0 intensities"):
        spec.sources(F, K)
    rec = st.StatisticsRecord(spec, R)
    rec.offer(H, f, cnt, intensities=inten)
    # the same record from the columns themselves, named by plain sources of a handle without intensities
    plain = st.Statistics.per_walker(columns=(0, 1, 2, 3, 4), n_levels=3, hist=(2, 8, 0.0, 0.125))
    ref = st.StatisticsRecord(plain, R)
    ref.offer(x[..., 0], x[..., 1:])
    for name in ("n", "shift", "s1", "s2", "has", "pend", "b2", "nb", "hist", "under", "over"):
        np.testing.assert_array_equal(getattr(rec, name), getattr(ref, name), err_msg=name)
    assert rec.hist.sum() + rec.under.sum() + rec.over.sum() == ns * R


def test_statistics_calls_without_intensities_keep_their_meaning():
    rng = np.random.default_rng(12)
    H, f, cnt = rng.normal(size=(3, 2)), rng.normal(size=(3, 2, 2)), rng.integers(0, 5, size=(3, 2, 2))
    spec = st.Statistics.per_walker(columns=(st.ENTHALPY, st.feature(1), st.kind(2, 0), st.ENERGY), weights=np.array([1.0, 2.0]))
    np.testing.assert_array_equal(spec.sources(2, 2), [0, 2, 3, 5])
    np.testing.assert_array_equal(spec.sources(2, 2), spec.sources(2, 2, 4))
    np.testing.assert_array_equal(spec.column_values(H, f, cnt), spec.column_values(H, f, cnt, rng.random((3, 2, 4))))
    a, b = st.StatisticsRecord(spec, 2), st.StatisticsRecord(spec, 2)
    a.offer(H, f, cnt)
    b.offer(H, f, cnt, None, None)
    np.testing.assert_array_equal(a.s2, b.s2)
    with pytest.raises(ValueError, match="column source 6 outside 0..5"):
        st.Statistics.per_walker(columns=(6,)).column_values(H, f, cnt)


def test_structure_plan_names_the_kernel_of_a_spec():
    """capi.structure_plan mirrors smolmc_sfac_plan (tests/test_gpu_structure.py compares the two on the device)."""
    W, lds = capi.STRUCT_WAVES, capi.STRUCT_LDS_BYTES
    assert capi.structure_plan(4096, 4096, 2, 16, 64) == ("mask",)
    assert capi.structure_plan(256, 256, 2, 64, 3) == ("mask",) and capi.structure_plan(256, 256, 2, 65, 3) == ("counters", W, 3)
    # the kind masks of four rows must fit LDS: 2048 (kind, word) pairs at most
    assert capi.structure_plan(64 * 1024, 65536, 2, 1, 1) == ("mask",)
    assert capi.structure_plan(64 * 1024 + 1, 65552, 2, 1, 1) is None        # (nor does the row fit next to counters)
    assert capi.structure_plan(64 * 512 + 1, 32784, 4, 1, 1) == ("counters", W, 1)
    assert capi.structure_plan(256, 256, 2, 2040, 9) == ("counters", W, 1)
    assert capi.structure_plan(256, 256, 2, 2041, 9) == ("counters", 1, 3)
    assert capi.structure_plan(256, 256, 2, capi.MAX_STRUCT_CELLS // 2, 9) == ("counters", 1, 1)
    assert capi.structure_plan(19683, 19696, 2, capi.MAX_STRUCT_CELLS // 2, 1) is None
    assert 4 * capi.MAX_STRUCT_CELLS + 16384 <= lds   # (rows of up to 16384 bytes fit next to the largest counter set)
