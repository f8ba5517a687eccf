"""Inputs and the NumPy reference of the sweep probe (smol_amd/csrc/probe_sweeps.hip -> smol_amd/libsmolmc_probe.so).

The probe runs ONE instantiation of the Ewald potential-field sweeps of smolmc_common.h per launch, workgroup b on its own
slice of phi with na = na_list[b] entries.  What a sweep must compute is

    phi'[j] = phi[j] + sum_f dq_f * G[s_f][j]        for j < na,   nothing else written,

with G[s_f][j] = gx[a_j + b_f] for the translation-compressed forms (E8[j] = 8 a_j, S8[f] = 8 b_f, gx an array of doubles)
and G[s_1] = ga, G[s_2] = gb for the dense-row forms.

Two data sets:

* ``exact``: dq_f = k_f / 16 with 0 < |k_f| <= 64, table values m / 2^20 with 0 < |m| <= 2^20, phi = p / 2^20 with
  |p| <= 2^23.  In units of 2^-24 a product is k m (|k m| <= 2^26) and phi is 16 p (<= 2^27), so every partial sum of up to
  four products and phi is an integer below 3 * 2^27 < 2^30: float64 holds it exactly whatever the order and however the
  fmas are fused, and the comparison is BIT EQUALITY.  (`check_exact_budget` proves it against int64 arithmetic.)  The data
  are drawn so that sum_f dq_f G != 0 at every entry: a skipped entry or one updated twice always changes bits.
* ``real``: uniform float64 inputs, reference in a wider format (np.longdouble where it carries >= 63 mantissa bits,
  fractions.Fraction otherwise).  The bound is derived, not measured: a sweep is NF fused multiply-adds per entry, each
  rounds once with relative error <= 2^-53 of a partial sum bounded by S = |phi| + sum_f |dq_f G|, so
  |err| <= NF 2^-53 S (1 + O(2^-53)); the reference's own error is below (NF + 1) 2^-63 S.  Both fit in NF 2^-52 S.

Guards (all finite, nothing here can fault): GUARD doubles behind every phi slice must come back bit-unchanged; E8 and the
rows carry PAD = 27 * 64 valid entries behind each slice, which select a gx cell / hold a row value of 2^30, so a stray
entry that reaches a written value shows up as a huge error."""

import ctypes as C
import os
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_PATH = os.path.join(ROOT, "smol_amd", "libsmolmc_probe.so")

GUARD = 128        # doubles behind every phi slice (SMOLMC_PROBE_GUARD)
PAD = 27 * 64      # valid padding entries behind every E8 / row slice
MAX_GROUPS = 82    # three batches of 27 and two chunks of 4 x 9 (= 72) with room behind them
BIG = 2.0 ** 30    # what a stray table entry reads
N_A, N_B = 4096, 512  # ranges of a_j and b_f: gx has N_A + N_B cells, then N_B cells of BIG for the padding entries

# (name, NF, compressed?) in the order of enum ProbeVariant
VARIANTS = [
    ("gx_multi<1,2>", 1, True), ("gx_multi<1,1>", 1, True), ("gx_multi<1,0>", 1, True),
    ("gx_multi<2,1>", 2, True), ("gx_multi<2,0>", 2, True),
    ("gx_multi<3,1>", 3, True), ("gx_multi<3,0>", 3, True),
    ("gx_multi<4,1>", 4, True), ("gx_multi<4,0>", 4, True), ("gx_multi<4,-1>", 4, True),
    ("gx_pre27", 1, True), ("gx_groups<1,16>", 1, True), ("gx_groups<2,16>", 2, True),
    ("dense<false>", 1, False), ("dense<true>", 2, False), ("dense<false,6>", 1, False), ("dense<true,4>", 2, False),
]
VARIANT_NAMES = [v[0] for v in VARIANTS]

# Batch sizes U of the sweeps and the chunk sizes NB the kernels use them with (smolmc_common.h: field_sweep_gx_multi
# takes <U, NB> = <27, 1>, <9, 4>, <9, 1>, <4, 1>; the dense field_sweep has U = 9, 14, 6, 4 and no chunks).
BATCHES = {4: (1,), 9: (1, 4), 14: (1,), 27: (1,)}


def edge_groups():
    """Group counts at which a sweep with batches of U groups in chunks of NB batches changes path."""
    out = set()
    for U, nbs in BATCHES.items():
        out |= {U - 1, U, U + 1, 2 * U - 1, 2 * U}
        for NB in nbs:
            out |= {NB * U, NB * U + 1}
    return sorted(out)


def ladder(variant):
    """na of every workgroup: each na from 1 to 768 (every ragged length at every small group count), then every group count
    up to MAX_GROUPS with tails of 0, 1 and 63 entries.  gx_pre27 from 27 groups on; the 16-group register sweep at 1024."""
    name = VARIANT_NAMES[variant]
    if name.startswith("gx_groups"):
        return np.array([1024], dtype=np.int32)
    nas = list(range(1, 769))
    for g in range(12, MAX_GROUPS + 1):
        nas += [g * 64 + t for t in (0, 1, 63) if g * 64 + t > 768]
    nas = np.array(nas, dtype=np.int32)
    if name == "gx_pre27":
        nas = nas[nas >= 27 * 64]
    return nas


class Case:
    """Host arrays of one probe launch and its expected result."""


def _layout(nas):
    c = Case()
    c.nas = nas.astype(np.int32)
    n64 = nas.astype(np.int64)
    c.phi_off = np.concatenate([[0], np.cumsum(n64 + GUARD)[:-1]]).astype(np.int64)
    c.tab_off = np.concatenate([[0], np.cumsum(n64 + PAD)[:-1]]).astype(np.int64)
    c.phi_len = int((n64 + GUARD).sum()) + PAD  # (slack behind the last slice's guard)
    c.tab_len = int((n64 + PAD).sum())
    start = np.concatenate([[0], np.cumsum(n64)[:-1]])
    c.blk = np.repeat(np.arange(len(nas)), nas)          # workgroup of every valid entry
    c.j = np.arange(int(n64.sum())) - np.repeat(start, nas)  # its index inside the slice
    c.pos_phi = c.phi_off[c.blk] + c.j
    c.pos_tab = c.tab_off[c.blk] + c.j
    return c


def make_case(variant, kind, seed=0):
    """All inputs of one launch of `variant` on its ladder, kind 'exact' or 'real', and the expected phi.
    Deterministic; for 'exact' the seed is advanced until no entry's update is zero."""
    name, NF, compressed = VARIANTS[variant]
    assert kind in ("exact", "real")
    nas = ladder(variant)
    for attempt in range(64):
        rng = np.random.default_rng([variant, int(kind == "real"), seed, attempt])
        c = _layout(nas)
        c.variant, c.kind, c.name, c.NF, c.compressed = variant, kind, name, NF, compressed
        nv = len(c.j)

        def table(n):  # non-zero values in [-1, 1]
            if kind == "exact":
                m = rng.integers(1, 2 ** 20 + 1, size=n) * rng.choice([-1, 1], size=n)
                return m.astype(np.int64), m / 2.0 ** 20
            x = rng.uniform(2.0 ** -20, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)
            return None, x

        if kind == "exact":
            c.k = (rng.integers(1, 65, size=4) * rng.choice([-1, 1], size=4)).astype(np.int64)
            c.dq = c.k / 16.0
            c.p = rng.integers(-2 ** 23, 2 ** 23 + 1, size=c.phi_len).astype(np.int64)
            c.phi0 = c.p / 2.0 ** 20
        else:
            c.k = c.p = None
            c.dq = rng.uniform(0.25, 4.0, size=4) * rng.choice([-1.0, 1.0], size=4)
            c.phi0 = rng.uniform(-8.0, 8.0, size=c.phi_len)
        c.b = rng.choice(N_B, size=4, replace=False).astype(np.int64)
        c.s8 = (8 * c.b).astype(np.uint32)
        if compressed:
            c.a = rng.integers(0, N_A, size=nv).astype(np.int64)
            c.m_gx, gx = table(N_A + N_B)
            c.gx = np.concatenate([gx, np.full(N_B, BIG)])
            c.E8 = np.full(c.tab_len, 8 * (N_A + N_B), dtype=np.uint32)  # padding entries: a cell of BIG for every b_f
            c.E8[c.pos_tab] = (8 * c.a).astype(np.uint32)
            c.ga = c.gb = None
            c.G = [c.gx[c.a + c.b[f]] for f in range(NF)]
            c.mG = [c.m_gx[c.a + c.b[f]] for f in range(NF)] if kind == "exact" else None
        else:
            c.E8 = c.gx = None
            rows, c.G, c.mG = [], [], []
            for f in range(2):
                m, x = table(nv)
                row = np.full(c.tab_len, BIG)
                row[c.pos_tab] = x
                rows.append(row)
                if f < NF:
                    c.G.append(x)
                    c.mG.append(m)
            c.ga, c.gb = rows
            if kind != "exact":
                c.mG = None
        c.delta = np.zeros(nv)
        for f in range(NF):
            c.delta = c.delta + c.dq[f] * c.G[f]   # (exact kind: exact in float64, see check_exact_budget)
        if kind == "real" or (np.all(c.delta != 0.0) and np.all(2.0 * c.delta != 0.0)):
            break
    else:
        raise AssertionError("no seed gives a non-zero update at every entry")
    c.expected = c.phi0.copy()
    if kind == "exact":
        c.expected[c.pos_phi] = c.phi0[c.pos_phi] + c.delta
        c.bound = None
    else:
        c.expected_ld, c.bound = _wide_reference(c)
        c.expected[c.pos_phi] = c.expected_ld.astype(np.float64)
    return c


def _wide_reference(c):
    """phi + sum_f dq_f G in a wider format, and the derived bound NF 2^-52 (|phi| + sum_f |dq_f G|) per valid entry."""
    phi = c.phi0[c.pos_phi]
    if np.finfo(np.longdouble).nmant >= 63:
        ref = phi.astype(np.longdouble)
        S = np.abs(ref)
        for f in range(c.NF):
            t = np.longdouble(c.dq[f]) * c.G[f].astype(np.longdouble)
            ref = ref + t
            S = S + np.abs(t)
        return ref, S * np.longdouble(c.NF * 2.0 ** -52)
    ref = np.empty(len(phi), dtype=object)  # exact rationals where long double is no wider than double
    S = np.empty(len(phi), dtype=object)
    for i in range(len(phi)):
        t = [Fraction(float(c.dq[f])) * Fraction(float(c.G[f][i])) for f in range(c.NF)]
        ref[i] = Fraction(float(phi[i])) + sum(t)
        S[i] = (abs(Fraction(float(phi[i]))) + sum(abs(x) for x in t)) * c.NF * Fraction(1, 2 ** 52)
    return ref, S


def check_exact_budget(c):
    """The exact data set in int64 units of 2^-24: every partial sum stays below 2^30 and the float64 reference equals the
    integer result bit for bit; no entry's update, nor twice it, is zero."""
    assert c.kind == "exact"
    assert np.all(c.k != 0) and np.all(np.abs(c.k) <= 64)
    acc = 16 * c.p[c.pos_phi]
    assert np.abs(c.p).max() <= 2 ** 23
    worst = np.abs(acc).max()
    upd = np.zeros_like(acc)
    for f in range(c.NF):
        assert np.all(c.mG[f] != 0) and np.abs(c.mG[f]).max() <= 2 ** 20
        upd = upd + c.k[f] * c.mG[f]
        worst = max(worst, np.abs(acc + upd).max(), np.abs(upd).max())
    assert worst < 2 ** 30, worst
    assert np.all(upd != 0) and np.all(2 * upd != 0)
    want = (acc + upd).astype(np.float64) / 2.0 ** 24  # (an integer below 2^53 and a power of two: exact)
    assert np.array_equal(want.view(np.int64), c.expected[c.pos_phi].view(np.int64))
    assert np.array_equal((upd.astype(np.float64) / 2.0 ** 24).view(np.int64), c.delta.view(np.int64))
    return int(worst)


def first_mismatch(c, got, where=""):
    """None when `got` (the whole phi buffer after the launch) is right, else a message naming the variant, na, the first
    wrong entry and its group of 64."""
    tag = f"{c.name} [{where}{c.kind}]"
    valid = np.zeros(len(got), dtype=bool)
    valid[c.pos_phi] = True
    outside = ~valid & (got.view(np.int64) != c.phi0.view(np.int64))
    if c.kind == "exact":
        bad = got[c.pos_phi].view(np.int64) != c.expected[c.pos_phi].view(np.int64)
    elif c.expected_ld.dtype == object:
        bad = np.array([abs(Fraction(float(g)) - r) > s for g, r, s in zip(got[c.pos_phi], c.expected_ld, c.bound)])
    else:
        bad = ~(np.abs(got[c.pos_phi].astype(np.longdouble) - c.expected_ld) <= c.bound)
    msgs = []
    if bad.any():
        i = int(np.argmax(bad))
        b, j = int(c.blk[i]), int(c.j[i])
        g0, d = float(got[c.pos_phi[i]]), float(c.delta[i])
        p0 = float(c.phi0[c.pos_phi[i]])
        kind = "skipped" if g0 == p0 else "updated twice" if g0 == p0 + 2 * d else "wrong"
        msgs.append(f"{tag}: na={int(c.nas[b])} ({int(c.nas[b]) >> 6} groups + {int(c.nas[b]) & 63}): entry {j} (group {j >> 6}, "
                    f"lane {j & 63}) {kind}: got {g0!r}, want {float(c.expected[c.pos_phi[i]])!r} (phi {p0!r}, update {d!r}); "
                    f"{int(bad.sum())} wrong entries in {len(np.unique(c.blk[bad]))} of {len(c.nas)} slices")
    if outside.any():
        pos = int(np.argmax(outside))
        b = int(np.searchsorted(c.phi_off, pos, side="right") - 1)
        j = pos - int(c.phi_off[b])
        msgs.append(f"{tag}: na={int(c.nas[b])}: guard entry {j} ({j - int(c.nas[b])} past na, group {j >> 6}) written: "
                    f"{float(c.phi0[pos])!r} -> {float(got[pos])!r}; {int(outside.sum())} guard entries changed")
    return "\n".join(msgs) if msgs else None


_PROBE = None


def load_probe():
    """ctypes handle of libsmolmc_probe.so (torch first: one HIP runtime per process, as smol_amd.engine.load_library)."""
    global _PROBE
    if _PROBE is None:
        if not os.path.exists(PROBE_PATH):
            raise RuntimeError(f"{PROBE_PATH} not found: build it (python -c 'import __graft_entry__ as g; g.build()' "
                               "or make -C smol_amd/csrc probe)")
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(PROBE_PATH)
        lib.smolmc_probe_variant_count.restype, lib.smolmc_probe_variant_count.argtypes = C.c_int, []
        lib.smolmc_probe_guard.restype, lib.smolmc_probe_guard.argtypes = C.c_int, []
        lib.smolmc_probe_sweep.restype = C.c_int
        lib.smolmc_probe_sweep.argtypes = [C.c_int] * 5 + [C.c_void_p] * 10
        _PROBE = lib
    return _PROBE


def run_on_device(c, lds, device="cuda:0"):
    """Upload the case through torch, run the probe once, return the whole phi buffer."""
    import torch

    lib = load_probe()
    dev = torch.device(device)
    keep = []

    def up(a, dtype=None):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.view(dtype))).to(dev)
        keep.append(t)
        return t.data_ptr()

    phi = torch.from_numpy(c.phi0.copy()).to(dev)
    args = [up(c.phi_off), up(c.tab_off), up(c.nas), up(c.E8, np.int32), up(c.gx), up(c.ga), up(c.gb),
            c.s8.ctypes.data, c.dq.ctypes.data]  # (the four flips go by value: host arrays)
    torch.cuda.synchronize(dev)
    rc = lib.smolmc_probe_sweep(c.variant, int(lds), len(c.nas), int(c.nas.min()), int(c.nas.max()), phi.data_ptr(), *args)
    assert rc == 0, f"smolmc_probe_sweep({c.name}) returned {rc}"
    out = phi.cpu().numpy()
    del keep
    return out
