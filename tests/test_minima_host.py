"""The minima record on the host (smol_amd/minima.py): ``MinimaRecord.offer`` -- the definition the device reduction
matches -- against a brute-force loop over rows, the ordered-bits mapping, the composition key, merge, the hull, and the
C-ABI additions of include/smolmc.h."""

import os
import re

import numpy as np
import pytest

from smol_amd import capi, engine
from smol_amd.minima import Minima, MinimaRecord, formation_energies, lower_hull, ordered_bits, weighted_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(spec, R, F, N, K, blocks, offers0=0):
    """The rule, row by row: offers in order, within an offer the walkers in order, a strictly lower value replaces."""
    n = spec.n_slots(R)
    rec = dict(value=np.full(n, np.inf), enthalpy=np.zeros(n), features=np.zeros((n, F)), occupancy=np.zeros((n, N), np.int32),
               counts=np.zeros((n, K), np.int32), walker=np.full(n, -1, np.int32), sample=np.full(n, -1, np.int64),
               step=np.zeros(n, np.uint64))
    if spec.n_axes == 0:
        rec["companions"] = np.zeros((n, N), np.int32)
    offer = offers0
    for H, feat, occ, cnt, st in blocks:
        for s in range(len(H)):
            for r in range(R):
                if spec.weights is None:
                    v = H[s, r]
                else:
                    v = 0.0
                    for i, w in enumerate(spec.weights):
                        v = v + w * feat[s, r, i]
                v = v + 0.0
                if spec.n_axes == 0:
                    slot = r
                else:
                    slot = 0
                    for a in range(spec.n_axes):
                        d = sum(int(spec.axis_weights[a, k]) * int(cnt[s, r, k]) for k in range(K))
                        c = d // int(spec.bins[a])  # (Python's floor division)
                        if not 0 <= c < spec.extents[a]:
                            slot = -1
                            break
                        slot = slot * int(spec.extents[a]) + c
                if slot < 0 or v != v or not v < rec["value"][slot]:
                    continue
                rec["value"][slot], rec["enthalpy"][slot], rec["features"][slot] = v, H[s, r], feat[s, r]
                rec["occupancy"][slot], rec["walker"][slot], rec["sample"][slot], rec["step"][slot] = occ[s, r], r, offer, st[s, r]
                if K:
                    rec["counts"][slot] = cnt[s, r]
                if spec.n_axes == 0 and slot == 0:  # (every walker's occupancy at the sample walker 0's entry comes from)
                    rec["companions"][:] = occ[s]
            offer += 1
    return rec


def _blocks(rng, R, F, N, K, sizes, levels=5):
    """Random blocks whose values repeat (few levels, both signs): ties within a sample, across samples and with the
    recorded value; NaN rows and both zeros."""
    out = []
    for ns in sizes:
        H = rng.integers(-levels, levels + 1, size=(ns, R)).astype(np.float64) * 0.25
        H[rng.random((ns, R)) < 0.1] = np.nan
        H[rng.random((ns, R)) < 0.1] = -0.0
        H[rng.random((ns, R)) < 0.1] = 0.0
        feat = rng.integers(-3, 4, size=(ns, R, F)).astype(np.float64)
        feat[rng.random((ns, R, F)) < 0.05] = -0.0
        occ = rng.integers(0, 3, size=(ns, R, N)).astype(np.int32)
        cnt = rng.integers(0, 6, size=(ns, R, K)).astype(np.int32)
        st = rng.integers(0, 1 << 40, size=(ns, R)).astype(np.uint64)
        out.append((H, feat, occ, cnt, st))
    return out


SPECS = {
    "walker-enthalpy": lambda: Minima.per_walker(),
    "walker-weights": lambda: Minima.per_walker(weights=[0.5, -1.25, 3.0]),
    "one-axis": lambda: Minima.by_composition(3, [1], extents=[6]),
    "two-axes": lambda: Minima.by_composition(3, [[1, -2, 0], [0, 1, 1]], bins=[2, 3], extents=[4, 3], weights=[1.0, 1.0]),
}


def _check(rec, want):
    for f, w in want.items():
        g = getattr(rec, f)
        assert g.dtype == w.dtype and g.shape == w.shape, f
        if f in ("value", "enthalpy", "features"):  # (bit for bit: -0.0 and +0.0 told apart)
            np.testing.assert_array_equal(g.view(np.uint64), w.view(np.uint64), err_msg=f)
        else:
            np.testing.assert_array_equal(g, w, err_msg=f)


@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("R", [1, 3, 70])
def test_offer_equals_the_brute_force_rule(name, R):
    spec = SPECS[name]()
    F, N, K = 4, 5, 3
    rng = np.random.default_rng(R + len(name))
    blocks = _blocks(rng, R, F, N, K, (1, 3, 17, 2))
    rec = MinimaRecord(spec, R, F, N, K)
    for b in blocks:
        rec.offer(*b)
    want = _brute(spec, R, F, N, K, blocks)
    _check(rec, want)
    assert rec.offers == 23
    assert np.array_equal(rec.filled, want["sample"] >= 0)
    assert not (np.signbit(rec.value) & (rec.value == 0)).any()  # (no -0.0 among the values)
    # an offer equal to the recorded value changes nothing; a NaN block changes nothing
    before = rec.copy()
    rec.offer(before.enthalpy[None, :R] if spec.n_axes == 0 and spec.weights is None else blocks[0][0], *blocks[0][1:])
    rec.offer(np.full((1, R), np.nan), np.full((1, R, F), np.nan), *blocks[0][2:])
    if spec.n_axes == 0 and spec.weights is None:
        assert rec.equals(before)
    # one sample given as (R,) arrays is one offer
    one = MinimaRecord(spec, R, F, N, K).offer(blocks[0][0][0], blocks[0][1][0], blocks[0][2][0], blocks[0][3][0], blocks[0][4][0])
    _check(one, _brute(spec, R, F, N, K, [blocks[0]]))


def test_planted_ties():
    spec, R = Minima.per_walker(), 4
    z = lambda ns: (np.zeros((ns, R, 1)), np.arange(ns * R * 2, dtype=np.int32).reshape(ns, R, 2))  # noqa: E731
    rec = MinimaRecord(spec, R, 1, 2)
    H = np.array([[1.0, -0.0, 2.0, np.nan], [1.0, 0.0, 1.0, np.nan], [0.5, 0.0, 1.0, np.nan]])
    rec.offer(H, *z(3))
    assert rec.sample.tolist() == [2, 0, 1, -1] and rec.walker.tolist() == [0, 1, 2, -1]
    assert rec.value.tolist() == [0.5, 0.0, 1.0, np.inf] and not np.signbit(rec.value[1])
    assert np.signbit(rec.enthalpy[1])  # (the enthalpy column is copied as it stands, the value is canonical)
    np.testing.assert_array_equal(rec.companions, z(3)[1][2])  # (walker 0's entry comes from sample 2: that sample's rows)
    rec.offer(np.array([[0.5, 0.0, 1.0, np.inf]]), *z(1))  # equal to the recorded values, and +inf against an empty entry
    assert rec.sample.tolist() == [2, 0, 1, -1] and rec.offers == 4
    # the same value on two walkers of one sample, keyed to one slot: the lowest walker
    spec = Minima.by_composition(1, [0], extents=[3])
    rec = MinimaRecord(spec, R, 1, 2, 1)
    cnt = np.array([[[1], [1], [1], [2]], [[1], [1], [2], [2]]], dtype=np.int32)
    rec.offer(np.array([[3.0, 2.0, 2.0, 5.0], [2.0, 2.0, 5.0, 4.0]]), *z(2), cnt)
    assert rec.walker.tolist() == [-1, 1, 3] and rec.sample.tolist() == [-1, 0, 1] and rec.value.tolist() == [np.inf, 2.0, 4.0]
    assert rec.filled.tolist() == [False, True, True] and rec.best(2).tolist() == [1, 2]


def test_ordered_bits_order_like_the_doubles():
    rng = np.random.default_rng(3)
    x = np.concatenate([
        rng.standard_normal(300) * 10.0 ** rng.integers(-300, 300, 300), rng.integers(0, 1 << 52, 50).astype(np.uint64).view(np.float64),
        -rng.integers(1, 1 << 52, 50).astype(np.uint64).view(np.float64), [np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0],
    ]) + 0.0
    k = ordered_bits(x)
    assert k.dtype == np.uint64
    a, b = np.meshgrid(np.arange(len(x)), np.arange(len(x)))
    assert np.array_equal(k[a] < k[b], x[a] < x[b])
    assert np.array_equal(k[a] == k[b], x[a] == x[b])
    assert ordered_bits(np.array([-0.0]) + 0.0) == ordered_bits(np.array([0.0]))
    assert ordered_bits(np.array([-0.0])) < ordered_bits(np.array([0.0]))  # (why values are canonicalised first)


def test_composition_key():
    spec = Minima.by_composition(2, [[1, -1], [0, 1]], bins=[3, 2], extents=[3, 4])
    counts = np.array([[0, 0], [5, 0], [0, 1], [0, 3], [0, 4], [9, 0], [8, 7], [3, 8], [2, 3]])
    # axis 0: d = c0 - c1 -> 0, 5, -1, -3, -4, 9, 1, -5, -1; // 3 -> 0, 1, -1, -1, -2, 3, 0, -2, -1
    # axis 1: d = c1 -> 0, 0, 1, 3, 4, 0, 7, 8, 3; // 2 -> 0, 0, 0, 1, 2, 0, 3, 4, 1
    key = spec.keys(counts[None], 9, (1, 9))[0]
    assert key.tolist() == [0, 4, -1, -1, -1, -1, 3, -1, -1]
    assert spec.n_slots(9) == 12
    assert (np.array([-1, -3, -4, -5]) // 3).tolist() == [-1, -1, -2, -2]  # (floor, not truncation)
    assert Minima.by_composition(2, [1], extents=[5]).axis_weights.tolist() == [[0, 1]]
    with pytest.raises(ValueError):
        Minima.by_composition(2, [[1, 2, 3]], extents=[3])
    # the value: left to right, every product and sum rounded on its own
    w, f = np.array([0.1, 0.2, 0.3]), np.array([[3.0, 1.5, -7.0]])
    assert weighted_value(w, f)[0] == ((0.0 + 0.1 * 3.0) + 0.2 * 1.5) + 0.3 * -7.0


@pytest.mark.parametrize("name", ["one-axis", "two-axes"])
def test_merge_of_split_blocks_equals_offer_of_the_whole(name):
    spec, R, F, N, K = SPECS[name](), 6, 4, 5, 3
    blocks = _blocks(np.random.default_rng(9), R, F, N, K, (5, 4, 7))
    whole = MinimaRecord(spec, R, F, N, K)
    parts, at = [], 0
    for b in blocks:
        whole.offer(*b)
        part = MinimaRecord(spec, R, F, N, K)
        part.offers = at  # (the part continues the numbering of the run)
        parts.append(part.offer(*b))
        at += len(b[0])
    assert MinimaRecord.merge(parts).equals(whole)
    # per walker: the ranks of a sharded sampler hold different walkers
    spec = Minima.per_walker(weights=[1.0, 2.0])
    whole = MinimaRecord(spec, R, F, N, K)
    ranks = [MinimaRecord(spec, 2, F, N, K), MinimaRecord(spec, 4, F, N, K)]
    for H, feat, occ, cnt, st in blocks:
        whole.offer(H, feat, occ, cnt, st)
        ranks[0].offer(H[:, :2], feat[:, :2], occ[:, :2], cnt[:, :2], st[:, :2])
        ranks[1].offer(H[:, 2:], feat[:, 2:], occ[:, 2:], cnt[:, 2:], st[:, 2:])
    merged = MinimaRecord.merge(ranks)
    assert merged.companions is None  # (every rank keeps the companions of its own walker 0: the merged record has none)
    np.testing.assert_array_equal(ranks[0].companions, whole.companions[:2])
    whole_plain = whole.copy()
    whole_plain.companions = None
    assert merged.equals(whole_plain)
    # ... and the record survives its dictionary form
    back = MinimaRecord.from_dict(whole.as_dict())
    assert back.equals(whole) and back.offers == whole.offers and back.spec.n_weights == 2


def test_lower_hull_and_formation_energies():
    #           0     1     2      3     4     5     6      7
    x = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 0.5, 0.25, 0.5])
    e = np.array([1.0, 0.25, -0.5, 0.5, 3.0, 0.0, 2.0, -0.5])
    ef = formation_energies(x, e)
    assert ef[0] == 0.0 and ef[4] == 0.0 and ef[2] == -0.5 - 2.0
    # (0.25, 0.25) is collinear between points 0 and 2: no vertex; points 5, 6 lie inside; 7 repeats 2; 3 lies below 2-4
    assert lower_hull(x, e).tolist() in ([0, 2, 3, 4], [0, 7, 3, 4])
    assert lower_hull(x, ef).tolist() == lower_hull(x, e).tolist()
    assert lower_hull([0.0, 1.0, 0.5], [0.0, 0.0, 0.5]).tolist() == [0, 1]
    assert lower_hull([2.0], [1.0]).tolist() == [0]


def test_the_header_declares_the_minima_calls():
    hdr = open(os.path.join(ROOT, "include", "smolmc.h")).read()
    declared = set(re.findall(r"\b(smolmc_[a-z_0-9]+)\s*\(", hdr))
    new = {"smolmc_set_minima", "smolmc_minima_shape", "smolmc_update_minima", "smolmc_reset_minima", "smolmc_get_minima",
           "smolmc_get_minima_companions"}
    assert new <= declared and new <= set(engine.SYMBOLS)
    assert re.search(r"#define\s+SMOLMC_SAMPLE_MINIMA\s+16\b", hdr) and capi.SAMPLE_MINIMA == 16
    assert re.search(r"#define\s+SMOLMC_MAX_MINIMA_AXES\s+4\b", hdr) and capi.MAX_MINIMA_AXES == 4
    assert re.search(r"#define\s+SMOLMC_ABI_VERSION\s+8\b", hdr)


def test_the_library_exports_them_and_the_struct_matches():
    import ctypes
    import subprocess
    import tempfile

    import __graft_entry__ as g

    if not os.path.exists(engine.LIB_PATH):
        g.build()
    lib = engine.load_library()
    for name in ("smolmc_set_minima", "smolmc_minima_shape", "smolmc_update_minima", "smolmc_reset_minima", "smolmc_get_minima"):
        assert hasattr(lib, name)
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "smolmc.h"
    int main(){printf("%zu %zu %zu %zu %zu\n", sizeof(smolmc_minima), offsetof(smolmc_minima, weights),
      offsetof(smolmc_minima, n_axes), offsetof(smolmc_minima, axis_weights), offsetof(smolmc_minima, axis_extent));return 0;}
    """
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"), os.path.join(d, "p.c")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "p")]).split()]
    M = capi.smolmc_minima
    assert vals == [ctypes.sizeof(M), M.weights.offset, M.n_axes.offset, M.axis_weights.offset, M.axis_extent.offset]
    # the spec fills it
    s, keep = Minima.by_composition(3, [[1, 0, 2]], bins=[2], extents=[7], weights=[1.0, 2.0]).c_struct()
    assert (s.n_weights, s.n_axes, s.weights[1], s.axis_weights[2], s.axis_bin[0], s.axis_extent[0]) == (2, 1, 2.0, 2, 2, 7)
    s, keep = Minima.per_walker().c_struct()
    assert (s.n_weights, s.n_axes) == (0, 0) and not s.weights and not s.axis_weights
