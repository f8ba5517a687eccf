"""The solo rows plan (engine.hip: solo_rows_plan; mc_lean.h: ROWS), checked WITHOUT a GPU through the library's
host-only hook smolmc_debug_solo_rows: which models take the variant and in which shape, and that the address-ordered
index rows and the reordered slot records hold exactly what the handle's lean rows (lp.idx) and slot records (lp.slots)
hold -- the kernels that read those are compared with the oracle elsewhere (tests/test_gpu_parity.py), the kernels that
read the new tables in tests/test_gpu_solo_rows.py."""

import ctypes as C
import os

import numpy as np
import pytest

from smol_amd import capi, engine, synth, workloads


class LeanSlot(C.Structure):
    _fields_ = [("doff8", C.c_uint32), ("stride8", C.c_uint32 * 3), ("feat", C.c_uint32), ("live", C.c_uint32),
                ("w", C.c_double), ("fs", C.c_double)]


class SoloRowsDebug(C.Structure):  # (the leading plain members of the hook's record)
    _fields_ = [(n, C.c_int) for n in ("shape", "row_len", "N", "Nlds", "swz_a", "swz_m", "swz_b", "nslot", "mm")] + [
        ("perm", C.POINTER(C.c_int)), ("rows", C.POINTER(C.c_uint32)), ("slots", C.POINTER(LeanSlot)),
        ("lean_rows", C.POINTER(C.c_uint16)), ("lean_slots", C.POINTER(LeanSlot))]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    if not os.path.exists(engine.LIB_PATH):
        g.build()
    L = engine.load_library()
    L.smolmc_debug_solo_rows.restype = C.c_void_p
    L.smolmc_debug_solo_rows.argtypes = [C.POINTER(capi.smolmc_tables), C.POINTER(capi.smolmc_config)]
    L.smolmc_debug_solo_rows_free.restype = None
    L.smolmc_debug_solo_rows_free.argtypes = [C.c_void_p]
    return L


def _slot_array(ptr, n):
    a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * C.sizeof(LeanSlot),)).copy()
    return a.view(np.dtype([("doff8", "<u4"), ("stride8", "<u4", 3), ("feat", "<u4"), ("live", "<u4"), ("w", "<f8"), ("fs", "<f8")]))


def _plan(lib, tab, step=capi.STEP_SWAP):
    """The hook's record as plain numpy copies (None: no lean tables for these tables at all)."""
    cfg = capi.make_config(1, capi.KERNEL_METROPOLIS, step)
    ptr = lib.smolmc_debug_solo_rows(C.byref(tab.struct), C.byref(cfg))
    assert ptr, "the hook refused valid tables"
    try:
        d = SoloRowsDebug.from_address(ptr)
        out = dict((n, getattr(d, n)) for n in ("shape", "row_len", "N", "Nlds", "swz_a", "swz_m", "swz_b", "nslot", "mm"))
        if out["nslot"]:
            nq = 64 * out["nslot"]
            out["lean_rows"] = np.ctypeslib.as_array(d.lean_rows, shape=(out["N"], 64, out["nslot"], out["mm"])).copy()
            out["lean_slots"] = _slot_array(d.lean_slots, nq)
        if out["shape"]:
            out["perm"] = np.ctypeslib.as_array(d.perm, shape=(nq,)).copy()
            out["rows"] = np.ctypeslib.as_array(d.rows, shape=(out["Nlds"], 64, out["row_len"])).copy()
            out["slots"] = _slot_array(d.slots, nq)
        return out
    finally:
        lib.smolmc_debug_solo_rows_free(ptr)


def _swz(s, p):
    return s ^ (((s >> p["swz_a"]) & p["swz_m"]) << p["swz_b"])


def _members(slots):
    """gathered members per position: its non-zero strides (padding and the point cluster have none)"""
    return np.where(slots["live"] > 0, (slots["stride8"] != 0).sum(axis=1), 0)


def _check_rows(p, widths):
    assert p["shape"] == widths[0] * 10 + widths[1] and p["row_len"] == sum(widths)
    assert (p["nslot"], p["mm"]) == (2, 2)
    perm, nm_old = p["perm"], _members(p["lean_slots"])
    assert sorted(perm) == list(range(128))
    nm = nm_old[perm]
    # sorted by member count, most first, stable
    assert np.all(np.diff(nm) <= 0)
    for k in np.unique(nm):
        assert np.all(np.diff(perm[nm == k]) > 0)
    # no lane holds more members than its slot gathers: in particular none of a one-member slot has a second entry
    width = np.repeat(np.array(widths), 64)
    off = np.repeat(np.array([0, widths[0]]), 64)
    assert np.all(nm <= width)
    # the slot records are the handle's, permuted
    assert p["slots"].tobytes() == p["lean_slots"][perm].tobytes()
    # the swizzle is a bijection on [0, Nlds) and every site's row sits at its address
    N, Nlds = p["N"], p["Nlds"]
    addr = np.array([_swz(s, p) for s in range(N)])
    assert len(set(addr)) == N and addr.min() >= 0 and addr.max() < Nlds
    rows, lean = p["rows"], p["lean_rows"]
    assert rows.max() < Nlds
    for q in range(128):
        it, ln, oit, oln = q // 64, q % 64, perm[q] // 64, perm[q] % 64
        for m in range(width[q]):
            got = rows[addr, ln, off[q] + m]
            if m < nm[q]:
                assert np.array_equal(got, lean[:, oln, oit, m]), (q, m)
            else:  # padding gathers the site itself (its stride is zero)
                assert np.array_equal(got, addr), (q, m)
                assert p["slots"]["stride8"][q][m] == 0
        # ... and nothing the lean row holds beyond that is a member
        for m in range(nm[q], p["mm"]):
            assert np.array_equal(lean[:, oln, oit, m], addr), (q, m)
    # addresses that belong to no site: rows of self-references
    spare = np.setdiff1d(np.arange(Nlds), addr)
    for a in spare:
        assert np.all(rows[a] == a)


def test_config2_plans_two_and_one(lib):
    w = workloads.config2(count=1)
    p = _plan(lib, w.tables)
    nm = _members(p["lean_slots"])
    print("config 2: members per position in the handle's order", np.bincount(nm[:64]), np.bincount(nm[64:]),
          "identity permutation:", bool(np.array_equal(p["perm"], np.arange(128))))
    assert sorted(np.bincount(nm, minlength=3)) == sorted([128 - 114, 54, 60])  # point + padding, pairs, triplets
    _check_rows(p, (2, 1))
    # three gathers per lane and flip: ceil(174 / 64)
    assert p["row_len"] == 3 == -(-(54 + 2 * 60) // 64)


def test_config1_plans_one_and_one(lib):
    w = workloads.config1(count=1)
    p = _plan(lib, w.tables)
    assert _members(p["lean_slots"]).max() == 1
    _check_rows(p, (1, 1))


@pytest.mark.parametrize("step", [capi.STEP_SWAP, capi.STEP_FLIP])
def test_small_triplet_model_rows(lib, step):
    model = synth.build_cluster_model(synth.fcc_prim(), {2: 6.0, 3: 5.0})
    sc = synth.build_supercell(model, [6, 6, 6])
    tab = capi.TableSet.from_synth(sc, synth.random_coefs(model))
    _check_rows(_plan(lib, tab, step), (2, 1))


def test_quadruplets_and_four_slots_are_left_alone(lib):
    # quadruplets: three gathered members
    model = synth.build_cluster_model(synth.fcc_prim(), {2: 5.0, 3: 4.0, 4: 3.0})
    sc = synth.build_supercell(model, [5, 5, 5])
    p = _plan(lib, capi.TableSet.from_synth(sc, synth.random_coefs(model)))
    assert p["mm"] == 3 and p["shape"] == 0, p
    # more than 128 clusters per site: four slots
    model = synth.build_cluster_model(synth.fcc_prim(), {2: 7.5, 3: 5.0})
    sc = synth.build_supercell(model, [7, 7, 7])
    p = _plan(lib, capi.TableSet.from_synth(sc, synth.random_coefs(model)))
    assert p["nslot"] == 4 and p["shape"] == 0, p


def test_more_triplets_than_one_slot_holds_are_left_alone(lib):
    """Two slots that both hold triplets (shape 2 + 2) keep the plain solo kernel."""
    model = synth.build_cluster_model(synth.fcc_prim(), {2: 4.5, 3: 6.0})
    sc = synth.build_supercell(model, [7, 7, 7])
    p = _plan(lib, capi.TableSet.from_synth(sc, synth.random_coefs(model)))
    if p["nslot"] == 2 and p["mm"] == 2:
        nm = _members(p["lean_slots"])
        assert ((nm == 2).sum() > 64) == (p["shape"] == 0), (np.bincount(nm), p["shape"])
    else:
        assert p["shape"] == 0
