"""The dispatched kernel instantiations: coordinates, prediction, and one oracle case per cell.

A handle reaches one of the library's Monte-Carlo kernels in three steps (engine.hip: family_of, lean_launcher; then
one or two first_match lists inside the launcher: launch.h and the ends of mc_lean.h, mc_lean_multi.h, mc_wl.h,
mc_general.h).  This module restates that path ONCE, in Python, so that a test can say which instantiation it ran:

* ``coords(symbol)``      a demangled kernel name of ``smol_amd.codeobj.kernel_digests`` -> named coordinates
                          (template, launcher F, NSLOT, MM, STEP, variant word V);
* ``predict(info, facts)`` the symbol a handle launches, from its ``kernel_info()`` string and what the case knows
                          about its own model (``Facts``): the key arithmetic of the launchers, list by list;
* ``NEVER_DISPATCHED``    predicates over coordinates no handle can produce, each with its reason and source line;
* ``HELPERS``             the kernels that are no Monte-Carlo template, each with the module that tests it;
* ``CASES``               the reduced matrix: the smallest models that land on each cell (``TARGETS`` pins the cell);
* ``UNREACHED``           required coordinates without a case, each with what was tried and what refused it.

Nothing here needs a device: tests/test_dispatch_matrix_host.py runs it on the built library's symbol table,
tests/test_gpu_dispatch_matrix.py runs the cases against the CPU oracle."""

import collections
import contextlib
import functools
import itertools
import os
import re

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# 1. coordinates of a symbol
# ---------------------------------------------------------------------------------------------------------------------
Coords = collections.namedtuple("Coords", "template F nslot mm step V")
STEPS = {0: "flip", 1: "swap"}  # SMOLMC_STEP_FLIP, SMOLMC_STEP_SWAP (include/smolmc.h); TableFlip kernels: "table"
MC_TEMPLATES = ("mc_lean_kernel", "mc_lean_multi_kernel", "mc_table_kernel", "mc_table_multi_kernel", "mc_wl_kernel",
                "mc_kernel", "mc_univ_kernel", "mc_dist_kernel")
_SYM = re.compile(r"^(?:void )?(\w+)<(.*)>\((.*)\)$")


def _args(text):
    return [{"true": True, "false": False}.get(a.strip(), a.strip()) for a in text.split(",")]


def _v(*pairs):
    """The variant word: the names whose condition holds, in the order given, joined by '|' ('-' for none)."""
    return "|".join(n for n, on in pairs if on) or "-"


def template_of(symbol):
    m = _SYM.match(symbol)
    return m.group(1) if m else None


def coords(symbol):
    """Coordinates of a Monte-Carlo kernel symbol; None for any other kernel (HELPERS)."""
    m = _SYM.match(symbol)
    if not m or m.group(1) not in MC_TEMPLATES:
        return None
    t, a = m.group(1), _args(m.group(2))
    if t == "mc_lean_kernel":  # <NSLOT, MM, STEP, MU, EWX, WL, BIAS, SOLO, KF, OCC, REPLAY>: lean_variant, mc_lean.h
        nslot, mm, step, mu, ewx, wl, bias, solo, kf, occ, replay = a
        nslot, mm, step, ewx, kf, occ = int(nslot), int(mm), int(step), int(ewx), int(kf), int(occ)
        wmu = bool(ewx & 4)
        F = ("rows" if mm in (21, 11) else "legacy-wl" if wl
             else ("bias-wmu" if bias else "corr-wmu" if kf else "wmu") if wmu
             else ("bias-replay" if bias else "replay") if replay
             else "bias" if bias else "corr" if kf else "run")
        V = _v(("MU", mu), ("EW1", ewx & 3 == 1), ("EW2", ewx & 3 == 2), ("WL", wl), ("BIAS", bias), ("SOLO", solo), ("KF", kf),
               ("OCC6", occ == 6), ("REPLAY", replay), ("WMU", wmu))
        return Coords(t, F, nslot, mm, STEPS[step], V)
    if t == "mc_lean_multi_kernel":  # <NSLOT, MM, STEP, MU, EWX, REG, BIAS, REPLAY, WLX>: multi_variant, mc_lean_multi.h
        nslot, mm, step, ewx, wlx = int(a[0]), int(a[1]), int(a[2]), int(a[4]), int(a[8])
        mu, reg, bias, replay = a[3], a[5], a[6], a[7]
        wmu, wwin, wlk = bool(ewx & 4), bool(wlx & 4), wlx & 3
        F = "multi-" + ("wl-win" if wwin else "wl-kf" if wlk == 2 else ("wl-replay" if replay else "wl") if wlk == 1
                        else ("bias-wmu" if bias else "wmu") if wmu
                        else "bias-replay" if bias and replay else "bias" if bias else "replay" if replay else "run")
        V = _v(("MU", mu), ("EW1", ewx & 3 == 1), ("EW2", ewx & 3 == 2), ("REG", reg), ("BIAS", bias), ("REPLAY", replay),
               ("WL", wlk == 1), ("WL_KF", wlk == 2), ("WMU", wmu), ("WWIN", wwin))
        return Coords(t, F, nslot, mm, STEPS[step], V)
    if t in ("mc_table_kernel", "mc_table_multi_kernel"):
        # mc_table_kernel<NSLOT, MM, EWX, REPLAY, BIAS, WL>; mc_table_multi_kernel<NSLOT, MM, EWX, REPLAY, WL, BIAS>
        nslot, mm, ewx, replay = int(a[0]), int(a[1]), int(a[2]), a[3]
        bias, wl = (a[4], a[5]) if t == "mc_table_kernel" else (a[5], a[4])
        wmu = bool(ewx & 4)
        F = ("table-" if t == "mc_table_kernel" else "multi-table-") + (
            ("bias-wmu" if bias else "wmu") if wmu else "wl" if wl else "bias" if bias else "replay" if replay else "run")
        V = _v(("EW1", ewx & 3 == 1), ("EW2", ewx & 3 == 2), ("REPLAY", replay), ("BIAS", bias), ("WL", wl), ("WMU", wmu))
        return Coords(t, F, nslot, mm, "table", V)
    if t == "mc_wl_kernel":  # <NSLOT, MM, STEPX, REPLAY, MU, EW>: launch_wl_kern, mc_wl.h
        nslot, mm, stepx, replay, mu, ew = int(a[0]), int(a[1]), int(a[2]), a[3], a[4], a[5]
        win = bool(stepx & 16)
        F = "wl-win" if win else "wl-replay" if replay else "wl"
        return Coords(t, F, nslot, mm, STEPS[stepx & 15], _v(("REPLAY", replay), ("MU", mu), ("EW", ew), ("WIN", win)))
    if t == "mc_kernel":  # <IdxT, NSLOT, MM, GENERIC, WL>: launch_general_nslot, mc_general.h
        idx16 = a[0] == "unsigned short"
        return Coords(t, "general", int(a[1]), int(a[2]), "any", _v(("WL", a[4]), ("GENERIC", a[3]), ("IDX16", idx16)))
    if t == "mc_univ_kernel":  # <OCC_LDS, K1, TABLE, WPS, DICT>: univ_select, mc_univ.h
        return Coords(t, "univ-dict" if a[4] else "univ", 0, 0, "table" if a[2] else "any",
                      _v(("OCC_LDS", a[0]), ("K1", a[1]), ("TABLE", a[2]), ("WPS4", int(a[3]) == 4)))
    return Coords(t, "dist-replay" if a[1] else "dist", int(a[0]), 0, "any", "-")  # mc_dist_kernel<NSLOT, REPLAY>


def show(c):
    return f"{c.F} nslot={c.nslot} mm={c.mm} {c.step} {c.V}"


# ---------------------------------------------------------------------------------------------------------------------
# 2. from a handle to its symbol
# ---------------------------------------------------------------------------------------------------------------------
def first_match(key, variants):
    """launch.h: the first entry equal to ``key``; the LAST entry is the `else` and takes every other key."""
    for v in variants[:-1]:
        if key == v:
            return v
    return variants[-1]


def falls_through(key, variants):
    """Does ``key`` reach the list's `else` without naming it?"""
    return key not in variants


def _b(x):
    return "true" if x else "false"


# the flags of the variant words, as in the enums next to each kernel
LV_MU, LV_WL, LV_BIAS, LV_SOLO, LV_KF, LV_OCC6, LV_REPLAY, LV_WMU = 4, 8, 16, 32, 64, 128, 256, 512  # (LV_EW = 3)
TV_REPLAY, TV_BIAS, TV_WL, TV_WMU = 1, 2, 4, 8
MV_MU, MV_REG, MV_BIAS, MV_REPLAY, MV_WL, MV_WL_KF, MV_WMU, MV_WWIN = 4, 8, 16, 32, 64, 128, 256, 512  # (MV_EW = 3)
WV_REPLAY, WV_MU, WV_EW, WV_WIN = 1, 2, 4, 8
GV_WL, GV_GENERIC, GV_IDX16 = 1, 2, 4
STEP_FLIP, STEP_SWAP, STEP_TABLE = 0, 1, 2


def lean_symbol(nslot, mm, step, v):  # lean_variant<NSLOT, MM, STEP, V>()
    return (f"void mc_lean_kernel<{nslot}, {mm}, {step}, {_b(v & LV_MU)}, {(v & 3) | (4 if v & LV_WMU else 0)}, {_b(v & LV_WL)}, "
            f"{_b(v & LV_BIAS)}, {_b(v & LV_SOLO)}, {6 if v & LV_KF else 0}, {6 if v & LV_OCC6 else 0}, {_b(v & LV_REPLAY)}>(LeanParams)")


def multi_symbol(nslot, mm, step, v):  # multi_variant<NSLOT, MM, STEP, V>()
    wlx = (2 if v & MV_WL_KF else 1 if v & MV_WL else 0) | (4 if v & MV_WWIN else 0)
    return (f"void mc_lean_multi_kernel<{nslot}, {mm}, {step}, {_b(v & MV_MU)}, {(v & 3) | (4 if v & MV_WMU else 0)}, {_b(v & MV_REG)}, "
            f"{_b(v & MV_BIAS)}, {_b(v & MV_REPLAY)}, {wlx}>(LeanParams)")


class Facts(collections.namedtuple("Facts", "step wl bias mu ewald replay ncls1 aliased", defaults=(False,) * 7)):
    """What a case knows about its handle beyond kernel_info(): the step type (0 flip, 1 swap, 2 TableFlip), a
    Wang-Landau kernel, an MCBias term, a chemical-potential table (has_mu), an Ewald term, whether the launch is a
    replay, one site class (lp.m_ncls == 1) and an aliased supercell (a cluster holds a site twice: mc_kernel's GENERIC)."""


Info = collections.namedtuple("Info", "family nslot mm field solo occ6 kf rows walker_mu wl_windows wl_tag")


def parse_info(info):
    """The fields of smolmc_kernel_info (engine.hip) that the dispatch reads."""
    head = info.split(" | not lean:")[0].split(" env=")[0]
    num = lambda key, default=0: int(m.group(1)) if (m := re.search(rf" {key}=(\d+)", head)) else default
    tag = re.search(r" wl=([\w-]+)", head)
    return Info(head.split()[0], num("nslot"), num("mm"), num("field"), " solo=1" in head, " occ=6" in head, " kf=1" in head,
                num("rows"), " walker_mu=1" in head, " wl_windows=1" in head, tag.group(1) if tag else None)


# engine.hip: lean_families[] -- per family the launcher of run, replay, table_replay, walker_mu, wl_win (None: no such
# instantiation) and whether NSLOT = 8 exists (L3) or not (L2)
LEAN_FAMILIES = {
    "K_LEAN": ("lean", "lean_replay", "table_replay", "lean_wmu", None, 2),
    "K_LEAN_BIAS": ("lean_bias", "lean_bias_replay", None, "lean_bias_wmu", None, 2),
    "K_LEAN_CORR": ("lean_corr", "lean_replay", None, "lean_corr_wmu", None, 2),
    "K_WL": ("wl", "wl_replay", None, None, "wl_win", 2),
    "K_TABLE_BIAS": ("table_bias", None, None, "table_bias_wmu", None, 2),
    "K_TABLE_WL": ("table_wl", None, None, None, None, 2),
    "K_MULTI": ("multi", "multi_replay", "multi_table_replay", "multi_wmu", None, 3),
    "K_MULTI_BIAS": ("multi_bias", "multi_bias_replay", None, "multi_bias_wmu", None, 3),
    "K_MULTI_WL": ("multi_wl", "multi_wl_replay", None, None, "multi_wl_win", 3),
    "K_MULTI_WL_KF": ("multi_wl_kf", None, None, None, None, 3),
    "K_MULTI_TABLE_BIAS": ("multi_table_bias", None, None, "multi_table_bias_wmu", None, 3),
    "K_MULTI_TABLE_WL": ("multi_table_wl", None, None, None, None, 3),
}


class NoLeanLauncher(LookupError):
    """The family has no launcher for this request (a NULL of lean_families[]): smolmc_replay then takes mc_kernel or the
    universal kernel, and smolmc_set_walker_mu / smolmc_set_wl_windows refuse the handle.

    Which kernel a replay cell runs is engine.hip's replay_route -- a function of the handle, the records' facts (longest
    record, a repeated site, a given a-priori factor), nsteps and the two SMOLMC_REPLAY_* switches -- and
    tests/test_gpu_replay_routes.py holds one case per row of it.  The replay cells here are the lean and lean-table
    routes: the oracle's own trajectory, no switch set."""


def family_of(k, f):
    """engine.hip: family_of, for a handle one of the two lean planners took."""
    table = f.step == STEP_TABLE
    if k.family == "lean":
        return (("K_TABLE_BIAS" if table else "K_LEAN_BIAS") if f.bias else "K_TABLE_WL" if f.wl and table
                else "K_LEAN_CORR" if k.kf else "K_WL" if f.wl else "K_LEAN")
    return (("K_MULTI_WL_KF" if k.kf else "K_MULTI_TABLE_WL" if table else "K_MULTI_WL") if f.wl
            else ("K_MULTI_TABLE_BIAS" if table else "K_MULTI_BIAS") if f.bias else "K_MULTI")


def lean_launcher(k, f):
    """engine.hip: lean_launcher -> the launcher's name (smolmc_launch_<name>_<nslot>)."""
    fam = family_of(k, f)
    run, replay, table_replay, walker_mu, wl_win, width = LEAN_FAMILIES[fam]
    if not f.replay and k.walker_mu:
        name = walker_mu
    elif not f.replay and k.wl_windows:
        name = wl_win
    elif not f.replay and fam == "K_LEAN" and k.rows and k.nslot == 2:
        name = "lean_rows"
    else:
        name = run if not f.replay else table_replay if f.step == STEP_TABLE else replay
    if name is None or (k.nslot == 8 and width == 2):
        raise NoLeanLauncher(f"{fam} has no launcher here: {k} {f}")
    return name


def lean_key(k, f, solo_variants):
    """mc_lean.h: lean_key.  Ewald maps to 1 / 2 by `ew_field ? 2 : 1` (launch_multi_variant passes ew_field through)."""
    mu = LV_MU if f.mu else 0
    if f.ewald:
        return mu | (2 if k.field else 1)
    if not solo_variants or not k.solo:
        return mu
    return mu | LV_SOLO | (LV_OCC6 if k.occ6 else 0)


def _mm_step(k, f):  # launch.h: with_mm_step (a TableFlip step would take the `else`: flip)
    return first_match(k.mm, [2, 3]), first_match(f.step, [STEP_SWAP, STEP_FLIP])


def _lean(k, f, variants, key):
    mm, step = _mm_step(k, f)
    return lean_symbol(k.nslot, mm, step, first_match(key, variants)), key, variants


def _mu_ew(k, f, B):  # launch_lean_mu_ew<NSLOT, B>
    return _lean(k, f, [B | LV_MU | 2, B | LV_MU | 1, B | 2, B | 1, B | LV_MU, B], B | lean_key(k, f, False))


def _wmu_mu_ew(k, f, F):  # launch_lean_wmu_mu_ew<NSLOT, F>
    B = F | LV_WMU | LV_MU
    return _lean(k, f, [B | 2, B | 1, B], F | LV_WMU | lean_key(k, f, False))


def _table(k, f, T):  # launch_table_nslot<NSLOT, T>
    ewm = 0 if not f.ewald else 2 if (T & TV_WL) or k.field else 1  # (Wang-Landau: the Ewald term from the field only)
    variants = [0, 2] if T & TV_WL else [0, 2, 1]
    ewx = first_match(ewm, variants) | (4 if T & TV_WMU else 0)
    return (f"void mc_table_kernel<{k.nslot}, {first_match(k.mm, [2, 3])}, {ewx}, {_b(T & TV_REPLAY)}, {_b(T & TV_BIAS)}, "
            f"{_b(T & TV_WL)}>(LeanParams)"), ewm, variants


def _table_multi(k, f, T):  # launch_table_multi_nslot<NSLOT, T>
    ewm = k.field if k.field in (1, 2) else 0
    variants = [2, 0, 1]
    ewx = first_match(ewm, variants) | (4 if T & TV_WMU else 0)
    return (f"void mc_table_multi_kernel<{k.nslot}, {first_match(k.mm, [2, 3])}, {ewx}, {_b(T & TV_REPLAY)}, {_b(T & TV_WL)}, "
            f"{_b(T & TV_BIAS)}>(LeanParams)"), ewm, variants


def _multi(k, f, B):  # launch_multi_variant<NSLOT, B>
    key = B | (MV_MU if f.mu else 0) | (k.field if k.field in (1, 2) else 0)
    variants = [B | MV_MU | 1, B | 1, B | MV_MU | 2, B | 2, B | MV_MU, B]
    mm, step = _mm_step(k, f)
    v = first_match(key, variants) | (MV_REG if k.nslot == 8 and f.ncls1 else 0)
    return multi_symbol(k.nslot, mm, step, v), key, variants


def _multi_wmu(k, f, F):  # launch_multi_wmu_variant<NSLOT, F>
    B = F | MV_WMU | MV_MU
    key = B | (k.field if k.field in (1, 2) else 0)
    variants = [B | 1, B | 2, B]
    mm, step = _mm_step(k, f)
    v = first_match(key, variants) | (MV_REG if k.nslot == 8 and f.ncls1 else 0)
    return multi_symbol(k.nslot, mm, step, v), key, variants


def _wl(k, f, B):  # launch_wl_variant<NSLOT, B> (Ewald: only with the field in LDS)
    key = B | (WV_MU if f.mu else 0) | (WV_EW if f.ewald else 0)
    variants = [B | WV_MU | WV_EW, B | WV_EW, B | WV_MU, B]
    v = first_match(key, variants)
    mm, step = _mm_step(k, f)
    return (f"void mc_wl_kernel<{k.nslot}, {mm}, {step | (16 if v & WV_WIN else 0)}, {_b(v & WV_REPLAY)}, {_b(v & WV_MU)}, "
            f"{_b(v & WV_EW)}>(LeanParams)"), key, variants


def _lean_run(k, f):  # launch_lean_nslot
    if f.step == STEP_TABLE:
        return _table(k, f, 0)
    key = LV_WL if f.wl else lean_key(k, f, True)
    return _lean(k, f, [LV_WL, LV_MU | 2, LV_MU | 1, 2, 1, LV_MU | LV_SOLO | LV_OCC6, LV_SOLO | LV_OCC6, LV_MU | LV_SOLO, LV_SOLO,
                        LV_MU, 0], key)


def _lean_wmu(k, f):  # launch_lean_wmu_nslot
    if f.step == STEP_TABLE:
        return _table(k, f, TV_WMU)
    B = LV_WMU | LV_MU
    return _lean(k, f, [B | 2, B | 1, B | LV_SOLO | LV_OCC6, B | LV_SOLO, B], LV_WMU | lean_key(k, f, True))


def _lean_replay(k, f):  # launch_lean_replay_nslot -> launch_lean_replay_kf<NSLOT, B>
    B = LV_REPLAY | (LV_KF if k.kf else 0)
    key = B | (lean_key(k, f, not (B & LV_KF)) & ~LV_OCC6)
    if B & LV_KF:
        return _lean(k, f, [B | LV_MU | 2, B | 2, B | LV_MU | 1, B | 1, B | LV_MU, B], key)
    return _lean(k, f, [B | LV_MU | 2, B | 2, B | LV_MU | 1, B | 1, B | LV_MU | LV_SOLO, B | LV_SOLO, B | LV_MU, B], key)


def _lean_rows(k, f):  # launch_lean_rows_nslot
    key = lean_key(k, f, True)
    variants = [LV_SOLO, LV_MU | LV_SOLO, LV_SOLO | LV_OCC6, LV_MU | LV_SOLO | LV_OCC6]
    return lean_symbol(k.nslot, first_match(k.rows, [21, 11]), first_match(f.step, [STEP_SWAP, STEP_FLIP]),
                       first_match(key, variants)), key, variants


LAUNCHERS = {
    "lean": _lean_run,
    "lean_bias": lambda k, f: _mu_ew(k, f, LV_BIAS),
    "lean_bias_replay": lambda k, f: _mu_ew(k, f, LV_BIAS | LV_REPLAY),
    "lean_corr": lambda k, f: _mu_ew(k, f, LV_KF),
    "lean_replay": _lean_replay,
    "lean_wmu": _lean_wmu,
    "lean_bias_wmu": lambda k, f: _wmu_mu_ew(k, f, LV_BIAS),
    "lean_corr_wmu": lambda k, f: _wmu_mu_ew(k, f, LV_KF),
    "lean_rows": _lean_rows,
    "table_bias": lambda k, f: _table(k, f, TV_BIAS),
    "table_wl": lambda k, f: _table(k, f, TV_WL),
    "table_replay": lambda k, f: _table(k, f, TV_REPLAY),
    "table_bias_wmu": lambda k, f: _table(k, f, TV_BIAS | TV_WMU),
    "wl": lambda k, f: _wl(k, f, 0),
    "wl_replay": lambda k, f: _wl(k, f, WV_REPLAY),
    "wl_win": lambda k, f: _wl(k, f, WV_WIN),
    "multi": lambda k, f: _table_multi(k, f, 0) if f.step == STEP_TABLE else _multi(k, f, 0),
    "multi_bias": lambda k, f: _multi(k, f, MV_BIAS),
    "multi_replay": lambda k, f: _multi(k, f, MV_REPLAY),
    "multi_bias_replay": lambda k, f: _multi(k, f, MV_BIAS | MV_REPLAY),
    "multi_wl": lambda k, f: _multi(k, f, MV_WL),
    "multi_wl_replay": lambda k, f: _multi(k, f, MV_WL | MV_REPLAY),
    "multi_wl_kf": lambda k, f: _multi(k, f, MV_WL_KF),
    "multi_wl_win": lambda k, f: _multi(k, f, MV_WL | MV_WWIN),
    "multi_wmu": lambda k, f: _table_multi(k, f, TV_WMU) if f.step == STEP_TABLE else _multi_wmu(k, f, 0),
    "multi_bias_wmu": lambda k, f: _multi_wmu(k, f, MV_BIAS),
    "multi_table_bias": lambda k, f: _table_multi(k, f, TV_BIAS),
    "multi_table_wl": lambda k, f: _table_multi(k, f, TV_WL),
    "multi_table_replay": lambda k, f: _table_multi(k, f, TV_REPLAY),
    "multi_table_bias_wmu": lambda k, f: _table_multi(k, f, TV_BIAS | TV_WMU),
}


def _general(k, f):  # launch_general_nslot (mc_general.h); engine.hip: general_tables sets generic, idx16 and mm
    key = (GV_GENERIC if f.aliased else GV_IDX16) | (GV_WL if f.wl else 0)  # (int32 rows: more than 65535 sites)
    variants = [GV_GENERIC | GV_WL, GV_GENERIC, GV_IDX16 | GV_WL, GV_IDX16, GV_WL, 0]
    v = first_match(key, variants)
    mm = (3 if k.mm == 3 else 6) if f.aliased else (k.mm if k.mm in (2, 3) else 5)
    mm = first_match(mm, [3, 6, 2, 5])
    return (f"void mc_kernel<{'unsigned short' if v & GV_IDX16 else 'int'}, {k.nslot}, {mm}, {_b(v & GV_GENERIC)}, {_b(v & GV_WL)}>"
            "(KParams, int)"), key, variants


def _universal(info):  # smolmc_univ_selector (univ.hip): kernel_info prints the selector's bits, univ_select names all sixteen
    w = dict(re.findall(r" (\w+)=(\w+)", info.split(" (")[0]))
    if not {"occ", "dict", "k1", "table", "dense"} <= set(w):
        raise NoLeanLauncher(f"no prediction for the universal kernel: this kernel_info does not carry its selector: {info}")
    occ, k1, table, dense, dl = w["occ"] == "lds", w["k1"] == "1", w["table"] == "1", w["dense"] == "1", w["dict"] == "1"
    key = (8 if occ else 0) | (4 if k1 else 0) | (2 if table else 0) | (1 if dense else 0)
    return (f"void mc_univ_kernel<{_b(occ)}, {_b(k1)}, {_b(table)}, {4 if dense else 2}, {_b(dl)}>(UParams, int)"), key, list(range(16))


def trace(info, facts):
    """(symbol, key, variant list) of the launch: the key and the list it was matched against, for the fall-through check."""
    if isinstance(info, str) and info.startswith("universal"):
        return _universal(info)
    k = parse_info(info) if isinstance(info, str) else info
    if k.family == "general":
        return _general(k, facts)
    if k.family not in ("lean", "lean-multi"):
        raise NoLeanLauncher(f"no prediction for the {k.family} kernel: kernel_info does not carry its selector")
    return LAUNCHERS[lean_launcher(k, facts)](k, facts)


def predict(info, facts):
    """The demangled symbol a handle with this kernel_info() launches, given the case's own facts."""
    return trace(info, facts)[0]


# ---------------------------------------------------------------------------------------------------------------------
# 3. what is never dispatched, and the kernels that are no Monte-Carlo template
# ---------------------------------------------------------------------------------------------------------------------
def _has(c, flag):
    return flag in c.V.split("|")


NEVER_DISPATCHED = [
    # (name, predicate over Coords, reason, file:line)
    ("lean LV_WL", lambda c: c.template == "mc_lean_kernel" and _has(c, "WL"),
     "round 2's Wang-Landau variant of mc_lean_kernel: family_of sends every single-class Wang-Landau handle to K_WL or K_TABLE_WL, "
     "so launch_lean_nslot never sees kernel_type == WANGLANDAU; kept so that the other kernels of lean_n*.hip do not move",
     "smol_amd/csrc/mc_lean.h:2544 (and engine.hip:2305)"),
    ("mc_kernel MM outside its index type", lambda c: c.template == "mc_kernel" and c.mm in ((2, 5) if _has(c, "GENERIC") else (6,)),
     "GENERIC rows run MM 3 or 6, the others 2, 3 or 5; all four are instantiated for every combination",
     "smol_amd/csrc/mc_general.h:796-798"),
    ("SOLO with Ewald", lambda c: c.template == "mc_lean_kernel" and _has(c, "SOLO") and (_has(c, "EW1") or _has(c, "EW2")),
     "lean_key returns the Ewald mode before it looks at the solo layout, and decide_lean plans solo only without Ewald; no list "
     "holds such a variant, so the library has no such symbol either (the predicate guards against one being added)",
     "smol_amd/csrc/mc_lean.h:2497 (and engine.hip:1825)"),
    ("SOLO replay with OCC6", lambda c: c.F == "replay" and _has(c, "OCC6"),
     "launch_lean_replay_kf masks LV_OCC6 out of the key: a six-waves handle replays on the plain solo kernel",
     "smol_amd/csrc/mc_lean.h:2577"),
]

HELPERS = {
    # kernel: the test module that holds it against its definition
    "pack_occ_kernel": "tests/test_gpu_sample_block.py", "unpack_occ_kernel": "tests/test_gpu_sample_block.py",
    "sample_snapshot_kernel": "tests/test_gpu_sample_ring.py", "eval_full_kernel": "tests/test_gpu_parity.py",
    "eval_delta_kernel": "tests/test_gpu_parity.py", "dot_features_kernel": "tests/test_gpu_device_plumbing.py",
    "beta_from_T_kernel": "tests/test_gpu_device_plumbing.py", "rex_decide_kernel": "tests/test_gpu_device_plumbing.py",
    "lazy_scalars_kernel": "tests/test_gpu_lazy_features.py", "ewald_field_init_kernel": "tests/test_gpu_fuzz.py",
    "wl_meanf_convert_kernel": "tests/test_gpu_wl_multi.py", "walker_mu_reprice_kernel": "tests/test_gpu_walker_mu.py",
    "grid_exchange_kernel": "tests/test_gpu_grid_exchange.py", "wl_exchange_kernel": "tests/test_gpu_wl_windows.py",
    "pop_clone_kernel": "tests/test_gpu_pop_anneal.py", "pop_parent_kernel": "tests/test_gpu_pop_anneal.py",
    "observables_kernel": "tests/test_gpu_observables.py", "statistics_kernel": "tests/test_gpu_statistics.py",
    "structure_kernel": "tests/test_gpu_structure.py", "structure_mask_kernel": "tests/test_gpu_structure.py",
    "connectivity_kernel": "tests/test_gpu_connectivity.py", "minima_copy_kernel": "tests/test_gpu_minima.py",
    "minima_rows_kernel": "tests/test_gpu_minima.py", "minima_clear_kernel": "tests/test_gpu_minima.py",
    "minima_winners_kernel": "tests/test_gpu_minima.py", "minima_companions_kernel": "tests/test_gpu_minima.py",
}


def never_dispatched(c):
    """The name of the first NEVER_DISPATCHED entry that holds for ``c``, or None."""
    return next((name for name, pred, _, _ in NEVER_DISPATCHED if pred(c)), None)


def helper_name(symbol):
    m = re.match(r"^(?:void )?(\w+)\(", symbol)
    return m.group(1) if m else None


# ---------------------------------------------------------------------------------------------------------------------
# 4. the cases: knobs -> the smallest model that lands on a cell
# ---------------------------------------------------------------------------------------------------------------------
# The planners read clusters per site (NSLOT 2 / 4 / 8: <= 128, <= 256, <= 512; engine.hip: build_mc_tables) and the
# largest cluster (MM 2 / 3: up to triplets, quadruplets; lean_need_mm).  Aliased cells are accepted on the lean
# families, so long cutoffs in a 3x3x3 cell reach the large NSLOT on 27 (fcc) or 54 (rocksalt) sites.
# kind: fcc2 / fcc3 = one class, 2 / 3 species; salt1 / salt1t = rocksalt with inert anions, 2 / 3 cation species (one class,
# Ewald possible); salt2 / salt2t = anions active too (two classes)            clusters per site, largest cluster
MODELS = {
    "fcc-p": ("fcc2", {2: 4.5}, [3, 3, 3]),                                 # 19, pairs
    "fcc-22": ("fcc2", {2: 6.0, 3: 5.0}, [3, 3, 3]),                        # 115, triplets
    "fcc-23": ("fcc2", {2: 5.0, 3: 4.2, 4: 3.0}, [3, 3, 3]),                # 87, quadruplets
    "fcc-42": ("fcc2", {2: 6.5, 3: 4.5}, [3, 3, 3]),                        # 139, triplets
    "fcc-43": ("fcc2", {2: 6.0, 3: 5.0, 4: 4.2}, [3, 3, 3]),                # 183, quadruplets
    "fcc-82": ("fcc2", {2: 6.5, 3: 5.2}, [3, 3, 3]),                        # 451, triplets
    "fcc-83": ("fcc2", {2: 6.0, 3: 5.2, 4: 4.2}, [3, 3, 3]),                # 495, quadruplets
    "fcc-rows21": ("fcc2", {2: 6.0, 3: 5.0}, [6, 6, 6]),                    # the solo rows shapes (lean_rows, mc_lean.h)
    "fcc-rows11": ("fccc2", {2: 6.0}, [4, 4, 4]),
    "fcc3-22": ("fcc3", {2: 5.0, 3: 3.0}, [3, 3, 3]),                       # ternary: several correlation functions per orbit
    "fcc3-23": ("fcc3", {2: 4.5, 3: 3.2, 4: 3.0}, [3, 3, 3]),
    "fcc3-42": ("fcc3", {2: 6.5, 3: 4.5}, [3, 3, 3]),
    "fcc3-43": ("fcc3", {2: 8.0, 3: 3.0, 4: 3.0}, [3, 3, 3]),                 # 167 (33 functions: the KF kernels take <= 64)
    "fcc3-82": ("fcc3", {2: 11.0}, [4, 4, 4]),                              # 321, pairs (48 functions; ternary triplets beyond the
                                                                            # nearest have more than SMOLMC_LEAN_MAX_KF per orbit)
    "fcc3-83": ("fcc3", {2: 10.0, 3: 3.0, 4: 3.0}, [4, 4, 4]),              # 257 (48 functions)
    "salt1-22": ("salt1", {2: 6.2, 3: 5.1}, [3, 3, 3]),
    "salt1-23": ("salt1", {2: 5.2, 3: 4.3, 4: 3.1}, [3, 3, 3]),
    "salt1-42": ("salt1", {2: 6.7, 3: 4.65}, [3, 3, 3]),
    "salt1-43": ("salt1", {2: 6.2, 3: 5.1, 4: 4.3}, [3, 3, 3]),
    "salt1-82": ("salt1", {2: 6.7, 3: 5.35}, [3, 3, 3]),
    "salt1-83": ("salt1", {2: 6.2, 3: 5.35, 4: 4.3}, [3, 3, 3]),
    "salt1t-22": ("salt1t", {2: 4.5, 3: 3.2}, [3, 3, 3]),
    "salt1t-82": ("salt1t", {2: 11.3}, [4, 4, 4]),
    "salt2-22": ("salt2", {2: 4.5, 3: 3.2}, [3, 3, 3]),                     # 93
    "salt2-23": ("salt2", {2: 4.3, 3: 3.2, 4: 3.0}, [3, 3, 3]),
    "salt2-42": ("salt2", {2: 5.5, 3: 3.2}, [3, 3, 3]),                     # 141
    "salt2-43": ("salt2", {2: 4.5, 3: 3.2, 4: 3.2}, [3, 3, 3]),             # 145
    "salt2-82": ("salt2", {2: 6.0, 3: 4.5}, [3, 3, 3]),                     # 306
    "salt2-83": ("salt2", {2: 6.0, 3: 4.5, 4: 3.2}, [3, 3, 3]),             # 358
    "fcc-22a": ("fcc2", {2: 6.0, 3: 5.0}, [2, 2, 2]),                       # aliased cells: mc_kernel's GENERIC rows
    "fcc-23a": ("fcc2", {2: 5.0, 3: 4.2, 4: 3.0}, [2, 2, 2]),
    "fcc-43a": ("fcc2", {2: 6.0, 3: 5.0, 4: 4.2}, [2, 2, 2]),
    "fcc-83a": ("fcc2", {2: 6.0, 3: 5.2, 4: 4.2}, [2, 2, 2]),
    "fcc-g16qa": ("fcc2", {2: 7.5, 3: 5.8, 4: 3.0}, [2, 2, 2]),
    "fcc-g16": ("fcc2", {2: 7.5, 3: 5.8}, [3, 3, 3]),                       # 717: beyond the lean families, mc_kernel NSLOT 16
    "fcc-g16q": ("fcc2", {2: 7.5, 3: 5.8, 4: 3.0}, [3, 3, 3]),
    "salt2t-22": ("salt2t", {2: 4.5}, [3, 3, 3]),                           # ternary cations: the KF Wang-Landau kernel
    "salt2t-23": ("salt2t", {2: 4.3, 3: 3.0, 4: 3.0}, [3, 3, 3]),
    "salt2t-42": ("salt2t", {2: 5.2, 3: 3.2}, [3, 3, 3]),
}
ONE_CLASS = ("fcc2", "fccc2", "fcc3", "salt1", "salt1t")
CHUNKS = (1, 7, 70, 300)  # the 64-step random batch boundary is crossed in several phases
RTOL, ATOL, FEATURE_ATOL = 1e-10, 1e-9, 1e-8  # the suite's bounds (tests/test_gpu_parity.py)


class Case(collections.namedtuple("Case", "model step kernel mu ewald bias mode drive env R update_period",
                                  defaults=("int", "run", (), 6, 1))):
    """One cell's knobs.  step 0 flip / 1 swap / 2 TableFlip; kernel 'm' Metropolis / 'wl' Wang-Landau; drive 'run', 'replay',
    'wmu' (per-walker chemical potentials) or 'win' (per-walker Wang-Landau windows); env: dispatch switches."""

    @property
    def id(self):
        flags = "".join(c for c, on in (("u", self.mu), ("e", self.ewald), ("b", self.bias)) if on) or "0"
        env = "+".join(e.replace("SMOLMC_", "").lower() for e in self.env) or "auto"
        return (f"{self.model}-{('flip', 'swap', 'table')[self.step]}-{self.kernel}{self.update_period if self.kernel == 'wl' else ''}"
                f"-{flags}-{self.mode}-{self.drive}-{env}-R{self.R}")

    @property
    def handle_id(self):
        """The knobs smolmc_create sees: cases that differ in the drive alone share one handle description."""
        return self._replace(drive="run").id

    @property
    def kind(self):
        return MODELS[self.model][0]

    @property
    def facts(self):
        return Facts(self.step, self.kernel == "wl", self.bias, self.mu, self.ewald, self.drive == "replay", self.kind in ONE_CLASS,
                     built(self.model)["aliased"])


DISPATCH_ENV = ("SMOLMC_NO_SOLO", "SMOLMC_NO_OCC6", "SMOLMC_NO_SOLO_ROWS", "SMOLMC_MULTI_PHI_HBM", "SMOLMC_MULTI_PHI_LDS",
                "SMOLMC_NO_EWALD_FIELD", "SMOLMC_DENSE_EWALD", "SMOLMC_FORCE_GENERAL", "SMOLMC_FORCE_UNIVERSAL",
                "SMOLMC_LAZY_FEATURES_ONLY", "SMOLMC_NO_LEAN_MULTI", "SMOLMC_NO_WL_MULTI", "SMOLMC_NO_TABLE_WL", "SMOLMC_NO_TABLE_BIAS",
                "SMOLMC_NO_LEAN_ALIASED", "SMOLMC_WL_RUNNING_MEAN", "SMOLMC_NO_ROTATE", "SMOLMC_LAUNCH_CHUNK", "SMOLMC_FAST_EPS_SCALE",
                "SMOLMC_REPLAY_GENERAL", "SMOLMC_REPLAY_UNIVERSAL", "SMOLMC_NO_LAZY_FEATURES", "SMOLMC_NO_SITE_RELABEL")


def candidates():
    """Every knob combination a handle can be asked for, by loops; TARGETS keeps the ones that cover the reduced matrix."""
    for model, (kind, _, _) in MODELS.items():
        ionic, one, ternary = kind.startswith("salt"), kind in ONE_CLASS, kind.endswith("3") or kind.endswith("t")
        for step, kernel, mu, bias, ewald in itertools.product((0, 1, 2), ("m", "wl"), (False, True), (False, True),
                                                               (False, True) if ionic else (False,)):
            if kernel == "wl" and bias:
                continue
            modes = ("corr",) if ternary else ("int",)  # (ternary: several correlation functions per orbit, the KF kernels)
            plain = kernel == "m" and not ewald and not bias and step != 2
            envs = [()]
            if plain and one:
                envs += [("SMOLMC_NO_SOLO",), ("SMOLMC_NO_SOLO_ROWS",)]
            if ewald:
                envs += [("SMOLMC_NO_EWALD_FIELD",), ("SMOLMC_MULTI_PHI_HBM",)] if one else [("SMOLMC_MULTI_PHI_HBM",)]
            if model in ("fcc-22", "fcc-43", "fcc-82", "salt2-22", "fcc-22a", "fcc-23a", "fcc-43a", "fcc-83a") and not mu and not bias and not ewald and step != 2:
                envs += [("SMOLMC_FORCE_GENERAL",)]
            for mode, env, up in itertools.product(modes, envs, (1, 3) if kernel == "wl" else (1,)):
                # Walkers: 3 where the planner can take a solo layout (one wave per workgroup: the grid IS the walker count), 10 on
                # the TableFlip and multi-class kernels, whose workgroups hold 1, 2, 4 or 8 walkers (one full and one partly
                # filled workgroup at 4 and 8, an odd tail at 2), 6 on the four-walker kernels (one full, one partly filled);
                # more than 16 walkers per CU for the six-waves-per-SIMD solo kernels (decide_lean)
                solo_able = plain and one and "SMOLMC_NO_SOLO" not in env and "SMOLMC_FORCE_GENERAL" not in env
                small = 3 if solo_able else 10 if (step == 2 or not one or up == 3 or model.endswith(("-82", "-83"))) else 6
                sizes = (small, 4100) if solo_able and not env and model in ("fcc-22", "fcc-23", "fcc-rows21", "fcc-rows11") else (small,)
                for R in sizes:
                    base = Case(model, step, kernel, mu, ewald, bias, mode, "run", env, R, up)
                    yield base
                    if "SMOLMC_FORCE_GENERAL" in env:
                        continue
                    yield base._replace(drive="replay")
                    if mu and kernel == "m":
                        yield base._replace(drive="wmu")
                    if kernel == "wl" and step != 2:
                        yield base._replace(drive="win")


@functools.lru_cache(maxsize=None)
def built(model):
    """dict(model, sc, nsp (per site), subs (active sites per sublattice), aliased, ewald) of a MODELS entry."""
    from smol_amd import synth

    kind, cutoffs, dims = MODELS[model]
    prim = {"fcc2": lambda: synth.fcc_prim(), "fccc2": lambda: synth.fcc_conventional_prim(), "fcc3": lambda: synth.fcc_prim(nspecies=3),
            "salt1": lambda: synth.rocksalt_prim(cation_charges=(1.0, 3.0)), "salt1t": lambda: synth.rocksalt_prim(),
            "salt2": lambda: synth.rocksalt_prim(cation_charges=(1.0, 3.0), anion_charges=(-2.0, -1.0)),
            "salt2t": lambda: synth.rocksalt_prim(anion_charges=(-2.0, -1.0))}[kind]()
    m = synth.build_cluster_model(prim, cutoffs)
    sc = synth.build_supercell(m, dims)
    nsp = np.array([prim.nspecies[b] for b in sc.site_b])
    aliased = any(len(set(row)) < len(row) for idx in sc.full_indices for row in np.asarray(idx).reshape(len(idx), -1).tolist())
    return dict(model=m, sc=sc, nsp=nsp, aliased=aliased)


@functools.lru_cache(maxsize=None)
def _ewald_of(model):
    from smol_amd import ewald

    return ewald.supercell_ewald(built(model)["sc"])


@functools.lru_cache(maxsize=None)
def tables(model, step, mu, ewald, bias, mode, mu_scale=1.0):
    """The TableSet of a case's handle (shared by the cases that differ in kernel, drive, env or R)."""
    from smol_amd import capi, synth

    b = built(model)
    sc, nsp = b["sc"], b["nsp"]
    W = int(nsp.max())
    mu_table = None
    if mu:  # one row per sublattice (the planners refuse per-site rows), different on cations and anions
        mu_table = mu_table_of(model, mu_scale)
    flip_table = None
    if step == STEP_TABLE:  # one exchange direction per active sublattice: species 0 <-> the last one
        prim = b["model"].prim  # (basis sites of one label are one sublattice: TableSet.from_synth)
        widths = [int(prim.nspecies[i]) for i in range(prim.nb) if prim.nspecies[i] > 1 and prim.labels[i] not in prim.labels[:i]]
        flip_table = np.zeros((len(widths), sum(widths)), dtype=np.int64)
        for k, w in enumerate(widths):
            flip_table[k, sum(widths[:k])], flip_table[k, sum(widths[:k]) + w - 1] = 1, -1
    tab = capi.TableSet.from_synth(sc, synth.random_coefs(b["model"], seed=11, scale=0.03),
                                   feature_mode=capi.FEATURES_CORRELATIONS if mode == "corr" else capi.FEATURES_INTERACTIONS,
                                   ewald=_ewald_of(model) if ewald else None, ewald_coef=0.1, mu_table=mu_table, flip_table=flip_table,
                                   swap_weight=0.2)
    if bias:  # FugacityBias (bias.py:208-226): fugacity fractions per site and species
        fu = np.ones((sc.num_sites, W))
        for site in np.flatnonzero(nsp > 1):
            fu[site, :nsp[site]] = np.linspace(0.2, 0.8, nsp[site])
        tab.set_bias(capi.BIAS_FUGACITY, fu)
    return tab


def start(case):
    """(occupancies (R, N), seeds, temperatures) of a case: random codes at every site, a temperature ladder."""
    b = built(case.model)
    rng = np.random.default_rng(sum(map(ord, case.model)))
    occ = (rng.random((case.R, b["sc"].num_sites)) * b["nsp"]).astype(np.int32)
    seeds = np.arange(case.R, dtype=np.uint64) * np.uint64(7919) + np.uint64(1001)
    return occ, seeds, np.linspace(1500.0, 6000.0, case.R)


WL_BIN, WIN_L = 0.25, 24


def config(case, R=None, window=None):
    from smol_amd import capi
    from tests.wl_window_oracle import enthalpies

    R = case.R if R is None else R
    if case.kernel == "m":
        return capi.make_config(R, capi.KERNEL_METROPOLIS, case.step)
    if window is None:  # edges NOT commensurate with the starting enthalpies (tests/test_gpu_fuzz.py)
        h = enthalpies(case_tables(case), start(case)[0])
        window = (float(h.min()) - 3.0371, float(h.max()) + 3.0113) if case.drive != "win" else windows(case, h)[2]
    return capi.make_config(R, capi.KERNEL_WANGLANDAU, case.step, min_enthalpy=window[0], max_enthalpy=window[1], bin_size=WL_BIN,
                            check_period=50, update_period=case.update_period, flatness=0.3)


def windows(case, h0):
    """Per-walker windows of WIN_L bins, each a non-integer number of bins below its walker's start: (vmin, vmax, window 0)."""
    from tests.wl_window_oracle import top

    # (1.37 r + 2.3 is no integer for r < 100: a walker that returns to its start must not sit on a bin edge, where the last
    # bit of the accumulated enthalpy decides the bin -- tests/test_gpu_fuzz.py)
    vmin = h0 - (np.arange(case.R) * 1.37 + 2.3) * WL_BIN
    vmax = np.array([top(v, WIN_L, WL_BIN) for v in vmin])
    return vmin, vmax, (float(vmin[0]), float(vmax[0]))


def case_tables(case, mu_scale=1.0):
    return tables(case.model, case.step, case.mu, case.ewald, case.bias, case.mode, mu_scale)


def walker_rows(case):
    """(R, n_sublattices, W) rows of chemical potentials: the table's own row scaled by factors spread over [-2, 2]."""
    tab = case_tables(case)
    subs = tab.active_sites()
    table = mu_table_of(case.model)
    base = np.array([table[s[0]] for s in subs])
    return np.array([base * s for s in np.linspace(-2.0, 2.0, case.R)])


def mu_table_of(model, scale=1.0):
    """The per-site chemical-potential table of a model: one row per sublattice, scaled."""
    b = built(model)
    sc, nsp = b["sc"], b["nsp"]
    t = np.zeros((sc.num_sites, int(nsp.max())))
    for site in np.flatnonzero(nsp > 1):
        t[site, :nsp[site]] = np.linspace(-0.3, 0.4, nsp[site]) * (1.0 if sc.site_b[site] == 0 else -0.5) * scale
    return t


# ---------------------------------------------------------------------------------------------------------------------
# 5. a case against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def dispatch_env(case):
    """The dispatch switches of smolmc_common.h as the case wants them, and nothing else; restored afterwards."""
    saved = {e: os.environ.pop(e, None) for e in DISPATCH_ENV}
    try:
        for e in case.env:
            os.environ[e] = "1"
        yield
    finally:
        for e in DISPATCH_ENV:
            os.environ.pop(e, None)
            if saved[e] is not None:
                os.environ[e] = saved[e]


def _wl_kw(case):
    return dict(step_type=case.step, bin_size=WL_BIN, check_period=50, update_period=case.update_period, flatness=0.3)


class _Walkers:
    """R one-walker oracles as one object (per-walker chemical potentials or windows): states stacked walker by walker."""

    def __init__(self, walkers):
        self.walkers = walkers

    def run(self, n):
        for w in self.walkers:
            w.run(n)

    def get_state(self):
        st = [w.get_state() for w in self.walkers]
        return {k: np.concatenate([s[k] for s in st]) for k in st[0]}

    def get_wl(self):
        st = [w.get_wl() for w in self.walkers]
        return {k: np.concatenate([s[k] for s in st]) for k in st[0]}

    def get_bias(self):
        return np.concatenate([w.get_bias() for w in self.walkers])


@functools.lru_cache(maxsize=None)
def reference(case):
    """The oracle's side of a case, computed once for both libraries: dict(occ0, seeds, temps, states [per chunk],
    wl [per chunk] or None, and for replay cells steps, uniforms, accepted, H of the oracle's own trajectory)."""
    from oracle import oracle as orc

    tab = case_tables(case)
    occ0, seeds, temps = start(case)
    ref = dict(occ0=occ0, seeds=seeds, temps=temps, wl=None)
    if case.drive == "wmu":
        rows = ref["rows"] = walker_rows(case)
        scales = np.linspace(-2.0, 2.0, case.R)
        assert len({r.tobytes() for r in rows}) >= 2
        ora = _Walkers([orc.OracleMC(case_tables(case, float(s)), config(case, 1)) for s in scales])
        for r, w in enumerate(ora.walkers):
            w.set_state(occ0[r:r + 1], seeds[r:r + 1], temps[r:r + 1])
    elif case.drive == "win":
        from tests.wl_window_oracle import enthalpies, one_walker_oracle

        vmin, vmax, _ = ref["windows"] = windows(case, enthalpies(tab, occ0))
        assert len(set(vmin)) >= 2
        ora = _Walkers([one_walker_oracle(tab, occ0[r], seeds[r], vmin[r], vmax[r], **_wl_kw(case)) for r in range(case.R)])
    else:
        ora = orc.OracleMC(tab, config(case))
        ora.set_state(occ0, seeds, temps)
    ref["start"] = ora.get_state()
    if case.drive == "replay":
        # the oracle's own trajectory: the proposal of every step from the state it was made in, and its acceptance uniform
        from tests.fast_band import uniforms_of

        n = sum(CHUNKS)
        steps = np.full((case.R, n, 16), -1, dtype=np.int32)
        propose = ora.proposer()
        for k in range(n):
            for r in range(case.R):
                nf, rec = propose(r, k)
                steps[r, k, :2 * nf] = rec[:2 * nf]
            ora.run(1)
        ref["steps"], ref["uniforms"] = steps, uniforms_of(seeds[:, None], np.arange(n, dtype=np.uint64)[None, :])
        walked = ora.get_state()
        ora = orc.OracleMC(tab, config(case))  # ... replayed on the oracle: the same chain, or the records are not its trajectory
        ora.set_state(occ0, seeds, temps)
        ref["accepted"], ref["H"], ref["states"], ref["wl"] = [], [], [], [] if case.kernel == "wl" else None
        at = 0
        for chunk in CHUNKS:
            acc, H = ora.replay(steps[:, at:at + chunk], ref["uniforms"][:, at:at + chunk])
            at += chunk
            ref["accepted"].append(acc), ref["H"].append(H), ref["states"].append(ora.get_state())
            if case.kernel == "wl":
                ref["wl"].append(ora.get_wl())
        assert np.array_equal(walked["occupancy"], ref["states"][-1]["occupancy"]), "the records are not the oracle's own trajectory"
        assert np.array_equal(walked["n_accepted"], ref["states"][-1]["n_accepted"])
    else:
        ref["states"], ref["wl"] = [], [] if case.kernel == "wl" else None
        for chunk in CHUNKS:
            ora.run(chunk)
            ref["states"].append(ora.get_state())
            if case.kernel == "wl":
                ref["wl"].append(ora.get_wl())
    ref["bias"] = None
    if case.bias:
        ref["bias"] = ora.get_bias()
    return ref


def feature_columns(case, F):
    """(Ewald column, chemical-work column) of a feature row, None where the model has no such term: the cluster features
    come first, then the Ewald term, then the chemical work (tests/test_gpu_walker_mu.py reads it as the last column)."""
    mu = F - 1 if case.mu else None
    ew = (F - 2 if case.mu else F - 1) if case.ewald else None
    return ew, mu


def liveness(case, tab, ref, final, bias_now=None, bias_start=None):
    """The variant's own term must be live, or the case proves nothing (asserted on the engine's final state)."""
    n_acc, n_steps = int(final["n_accepted"].sum()), int(final["n_steps"].sum())
    assert 0 < n_acc < n_steps, (n_acc, n_steps)
    for k, sites in enumerate(tab.active_sites()):  # an accepted change on the sublattice was proposed there
        if case.drive == "replay":
            assert np.isin(ref["steps"][:, :, 0::2], sites).any(), f"sublattice {k} is never proposed on"
        else:
            assert (final["occupancy"][:, sites] != ref["occ0"][:, sites]).any(), f"sublattice {k} is never proposed on"
    ew, mu = feature_columns(case, final["features"].shape[1])
    if ew is not None:
        assert (final["features"][:, ew] != ref["start"]["features"][:, ew]).any(), "the Ewald feature never changes"
    # (canonical swaps conserve the composition: the chemical work and a composition bias cannot change under them)
    if mu is not None and case.step != STEP_SWAP:
        assert (final["features"][:, mu] != ref["start"]["features"][:, mu]).any(), "the chemical work never changes"
    if case.bias and case.step != STEP_SWAP and bias_now is not None:
        assert (np.asarray(bias_now) != np.asarray(bias_start)).any(), "the bias value never changes"


def same_state(a, b):
    assert np.array_equal(a["occupancy"], b["occupancy"])
    assert np.array_equal(a["n_accepted"], b["n_accepted"])
    assert np.array_equal(a["n_steps"], b["n_steps"])
    assert np.array_equal(a["accepted"], b["accepted"])
    np.testing.assert_allclose(a["enthalpy"], b["enthalpy"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(a["features"], b["features"], rtol=RTOL, atol=FEATURE_ATOL)


def same_wl(x, y):
    np.testing.assert_allclose(x["entropy"], y["entropy"], rtol=0, atol=0)
    assert np.array_equal(x["histogram"], y["histogram"])
    assert np.array_equal(x["occurrences"], y["occurrences"])
    np.testing.assert_allclose(x["mean_features"], y["mean_features"], rtol=RTOL, atol=ATOL)


def run_case(case, engine_cls):
    """Run one case on the loaded library against ``reference(case)``; returns (kernel_info, predicted symbol)."""
    ref = reference(case)
    tab = case_tables(case)
    with dispatch_env(case):
        eng = engine_cls(tab, config(case))
        try:
            if case.drive == "wmu":
                eng.set_walker_mu(ref["rows"])
            if case.drive == "win":
                eng.set_wl_windows(ref["windows"][0], ref["windows"][1])
            info = eng.kernel_info()
            symbol = predict(info, case.facts)
            if case.drive == "win":
                eng.set_state(ref["occ0"], ref["seeds"])
            else:
                eng.set_state(ref["occ0"], ref["seeds"], ref["temps"])
            bias0 = eng.get_bias() if case.bias else None
            at = 0
            for j, chunk in enumerate(CHUNKS):
                if case.drive == "replay":
                    acc, H = eng.replay(ref["steps"][:, at:at + chunk], ref["uniforms"][:, at:at + chunk])
                    at += chunk
                    assert np.array_equal(acc, ref["accepted"][j])
                    np.testing.assert_allclose(H, ref["H"][j], rtol=RTOL, atol=ATOL)
                else:
                    eng.run(chunk)
                a = eng.get_state()
                same_state(a, ref["states"][j])
                if ref["wl"] is not None:
                    same_wl(eng.get_wl(), ref["wl"][j])
            full = eng.eval_full(a["occupancy"])
            if case.drive == "wmu":  # (eval_full prices the handle's own table: the chemical work of the rows is the last column)
                np.testing.assert_allclose(a["features"][:, :-1], full[:, :-1], rtol=RTOL, atol=FEATURE_ATOL)
                np.testing.assert_allclose(a["features"][:, -1], eng.chemical_work(a["occupancy"], ref["rows"]), rtol=RTOL, atol=FEATURE_ATOL)
            else:
                np.testing.assert_allclose(a["features"], full, rtol=RTOL, atol=FEATURE_ATOL)
            bias1 = eng.get_bias() if case.bias else None
            if ref["bias"] is not None:
                np.testing.assert_allclose(bias1, ref["bias"], rtol=RTOL, atol=ATOL)
            liveness(case, tab, ref, a, bias1, bias0)
        finally:
            eng.close()
    return info, symbol


# ---------------------------------------------------------------------------------------------------------------------
# 6. the reduced matrix, what it must cover, and what no small model reached
# ---------------------------------------------------------------------------------------------------------------------
from tests.dispatch_targets import TARGETS  # noqa: E402

CASES = [c for c in candidates() if c.id in TARGETS]
assert len(CASES) == len(TARGETS), sorted(set(TARGETS) - {c.id for c in CASES})[:5]
# the universal kernel's cells: the cases of tests/univ_layout.py (run by tests/test_gpu_univ_layout.py, which holds
# predict() of their kernel_info() against these), each on the instantiation its layout selects
from tests import univ_layout  # noqa: E402

UNIV_TARGETS = {name: show(coords(univ_layout.case_layout(name).symbol())) for name in univ_layout.CASE_IDS}


def coordinates_of(c):
    """The two reduced-matrix coordinates of a cell: its (F, V) pair and its (F, NSLOT, MM, STEP) tuple."""
    return {("FV", c.F, c.V), ("shape", c.F, c.nslot, c.mm, c.step)}


def classify(symbols, cases=None):
    """{symbol: 'covered' | 'dispatchable, not in the reduced matrix' | 'never dispatched' | 'helper'}; a symbol that is
    none of them raises.  ``cases``: the target strings of the cases that count (default: TARGETS and UNIV_TARGETS)."""
    covered = set(TARGETS.values()) | set(UNIV_TARGETS.values()) if cases is None else set(cases)
    out = {}
    for s in symbols:
        c = coords(s)
        if c is None:
            if helper_name(s) not in HELPERS:
                raise LookupError(f"unclassified kernel {s}: a Monte-Carlo template needs coords(), any other kernel a HELPERS entry")
            out[s] = "helper"
        elif never_dispatched(c):
            out[s] = "never dispatched"
        else:
            out[s] = "covered" if show(c) in covered else "dispatchable, not in the reduced matrix"
    return out


def required(symbols):
    """Every coordinate of a dispatchable symbol: the reduced matrix has a case, or an UNREACHED entry, for each."""
    need = set()
    for s in symbols:
        c = coords(s)
        if c is not None and not never_dispatched(c):
            need |= coordinates_of(c)
    return need


def covered_by(targets, symbols):
    """The coordinates that the cells ``targets`` (show() strings) cover."""
    by_show = {show(c): c for c in map(coords, symbols) if c is not None}
    got = set()
    for t in targets:
        got |= coordinates_of(by_show[t])
    return got


# Required coordinates without a case.  Each entry: a predicate over a coordinate, the knobs tried, and the planner
# condition that refused them.
UNREACHED = [
    (lambda q: q[0] == "shape" and q[1].startswith("multi-") and q[1] != "multi-wl" and q[1] != "multi-wl-replay" and q[1] != "multi-wl-win"
     and q[1] != "multi-wl-kf" and q[2:4] == (2, 3),
     "NSLOT 2 with quadruplets on two site classes: rocksalt with both sublattices active at {2: 3.0, 3: 3.0, 4: 3.0}, its shortest "
     "quadruplet cutoff, has 131 clusters per site (NSLOT 4); a conventional fcc cell with the corner and the face sites as two "
     "sublattices has 87",
     "plan_lean_multi: 'sites of one sublattice in different site classes (cluster environments)' for the fcc cell; one class "
     "reaches this shape only on the Wang-Landau families (update_period 3)"),
    (lambda q: q[:2] == ("FV", "general") and "GENERIC" not in q[2] and "IDX16" not in q[2],
     "mc_kernel with 32-bit index rows: needs more than 65535 sites, the matrix stops at 216",
     "engine.hip:439 (idx16 = !aliased && N <= 65535); tests/test_gpu_parity.py::test_more_than_65535_sites_uses_32bit_rows runs it"),
    (lambda q: q[:2] == ("shape", "general") and q[3] == 5,
     "mc_kernel MM 5: clusters of five or six sites on a cell that is not aliased; smol_amd.synth builds clusters up to quadruplets",
     "engine.hip:438 (need_mm > 3 on a cell that is not aliased)"),
    (lambda q: q == ("shape", "general", 2, 6, "any"),
     "mc_kernel MM 6 at NSLOT 2: fcc {2: 5.0, 3: 4.2, 4: 3.0} in a 2x2x2 cell is aliased, but its quadruplets keep three distinct "
     "other sites (MM 3); MM 6 is covered at NSLOT 4, 8 and 16",
     "engine.hip:438 (aliased ? (need_mm <= 3 ? 3 : 6))"),
    # NOT planner refusals.  The universal kernel's 32 instantiations have cells of their own (UNIV_TARGETS: 10 of them, every
    # Flip / Swap instantiation with the occupancy in LDS); the two entries below are the other 22, which a switch or a flip table
    # reaches on any model.  The distance kernels are not modelled.  With them UNREACHED holds 56 of the 550 required
    # coordinates (10.2 %), above the 5 % the matrix was meant to keep; without the universal and distance entries 25 of 506.
    (lambda q: q[1] in ("univ", "univ-dict") and q[0] == "FV" and "OCC_LDS" not in q[2].split("|") and (q[1], q[2]) != ("univ-dict", "K1|WPS4"),
     "15 coordinates: the occupancy in HBM (SMOLMC_UNIV_OCC_HBM, or a cell beyond a CU's LDS) on every instantiation but the one "
     "cell of the layout cases (dense-hbm).  Without the occupancy block the LDS layout has nothing left that these instantiations "
     "vary, so the layout cases stop at one; tests/test_gpu_universal.py runs the HBM kernels on every golden model, TableFlip shape "
     "and a 262 144-site cell (3 to 5 walkers, release library) without pinning their cells",
     "smol_amd/csrc/univ.hip: smolmc_univ_selector (UNIV_SEL_OCC_LDS); engine.hip: univ_lds_layout"),
    (lambda q: q[1] in ("univ", "univ-dict") and ((q[0] == "FV" and "TABLE" in q[2].split("|") and "OCC_LDS" in q[2].split("|")
                                                   and (q[1], q[2]) != ("univ-dict", "OCC_LDS|K1|TABLE|WPS4")) or q == ("shape", "univ", 0, 0, "table")),
     "8 coordinates: TableFlip handles with the occupancy in LDS beyond the one cell of the layout cases (crowded-table: K1, dense, "
     "dictionaries).  The others need a flip table on a model with several functions per record, with more than 64 records or with "
     "long tensors; tests/test_gpu_universal.py::test_table_flip_chains_on_the_universal_kernel runs nine TableFlip shapes of the "
     "reference at 4 walkers (release library) without pinning their cells",
     "smol_amd/csrc/univ.hip: smolmc_univ_selector (UNIV_SEL_TABLE)"),
    (lambda q: q[1] in ("dist", "dist-replay"),
     "NOT MODELLED, 8 coordinates: the distance-objective kernels' 6 instantiations (NSLOT 1 / 2 / 4, run and replay).  They are "
     "created by smolmc_create_distance, not by the planners above, and OracleMC has no distance objective to compare a stream with",
     "smol_amd/csrc/mc_dist.h:369; tests/test_gpu_sqs.py holds them against a restatement of the chain on the release and the bounds library"),
]


def unreached(q):
    return next((why for pred, why, _ in UNREACHED if pred(q)), None)
