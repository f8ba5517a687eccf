"""The exact transition law of the Wang-Landau chains in the two situations where they have one, and the statistics
that hold a batch of walkers against it (tests/test_wl_law_host.py on the CPU oracle, tests/test_gpu_wl_law.py on the
device).  The machinery -- proposals, grown state set, from-scratch energies, Sample / Expected, the chi-square with its
pooling and zero-probability rule, the power calculation -- is that of tests/chain_law.py; this module adds the accept
rule, the cases and its own family-wise level.

The law, restated in float64 NumPy from the semantics of the reference's smol/moca/kernel/wanglandau.py (the oracle
cites its lines in do_step of oracle/smolmc_oracle.c):

* proposals are exactly ``Law._proposals``: Flip, Swap, TableFlip with its log a-priori factor;
* b(H) = floor((H - min) / bin); a proposal y from x is rejected when H(y) < min or H(y) >= max (:191); otherwise
  exponent = S[b(x)] - S[b(y)] + log_priori (:197-198), accepted when exponent >= 0, else with probability
  exp(exponent).  An empty Swap step has dH = 0 and is accepted;
* after every step, accepted or not, with c the bin of the state the walker is now in (:222-245): the walker's step
  counter gains 1, mean_features[c] takes the running mean with the current features, and when the counter is a
  multiple of update_period S[c] += m, histogram[c] += 1, occurrences[c] += 1.  The start state is not counted.

check_period is 0 everywhere: the modification factor never changes and the histogram is never emptied.

FROZEN tier (``WLFrozenLaw``).  With entropies S0 >= 1 set through ``set_wl`` and m = 2^-64, S + m == S in float64: the
chain is a plain Markov chain with the acceptance above, reversible with pi(x) ~ exp(-S0[b(x)]) on the states inside the
window (``stationary_residual``).  ``matrices`` carries the acceptance, everything else (``expected``, the joint law over
(state, n_accepted) for n <= 2) is ``Law``'s.  State points are entropy vectors, walker groups of one handle: point 0 is
S0 = 1 + ln g[b] with g the number of enumerated states of bin b inside the window (the flat-histogram point; on the cells
grown to depth 2 g counts the grown set, which is all the law can see), point 1 is S0 = 1 + c |b - b(start)| with c
solved so that the first step is rejected with probability 1/2.  n in (1, 2, 3, 8, 64) on cells grown to closure, (1, 2)
on cells grown to depth 2.

LIVE tier (``WLPathLaw``, ``path_expected``).  With m = 0.75 the entropy moves; the law is over paths of n in (2, 3) steps from a set
S0, update_period 1 and 2: the tree of (state, histogram row, n_accepted) is enumerated, S after step t is S0 + m *
histogram.  The outcome row is [occupancy | histogram row | n_accepted].

Per law the three statistics of chain_law: (a) the pooled Pearson chi-square with the zero-probability rule, (b) at n = 1
z of the accepted count, (c) z of the mean running enthalpy.  Exact per-walker identities are asserted outright
(``identities``): histogram.sum() == n // update_period, occurrences == histogram, the entropy bitwise S0 (frozen) or
allclose(S0 + m * histogram, rtol 1e-12) (live: mc_wl.h builds S from per-launch step counts, so the last bit may differ
from a repeated add -- the tolerance of tests/test_gpu_long_streams.py), the running enthalpy equal to the from-scratch
H of the final state (rtol 1e-10, atol 1e-9, inside ``evaluate``), and at n = 1 mean_features[b(final)] equal to the
from-scratch features of the final state.

One family-wise level of its own, 1e-3, split evenly over this tier's ``N_STATISTICS`` (three per law and module), so the
thresholds of chain_law do not move.  Seeds are fixed; group g owns the seeds base + g * 2^18 .. so that the first
walkers of a group are the same chains at every R.

Conditions on the inputs, asserted on the law before any chain runs (``conditions``): the pooled cell holds at most 5 %
of the mass; every enumerated state's H lies at least 1e-6 bin from every edge of the window's grid (tests/fast_band.py
owns the edges); the window holds at least 4 occupied bins; the first step is rejected by the entropy rule with
probability in [0.25, 0.75] at every state point; in the live tier at least 10 % of the path mass of some later step
passes through a decision whose acceptance differs between S0 and the updated S; the window-cut cases have at least 5 %
of the first step's proposal mass outside the window.  The window is chosen by ``_design`` from the law alone: the
smallest number of bins (from 5) of a grid laid 0.37 bin around the enumerated enthalpies that meets these.

Defects, each a variation of THIS law: ``entropy-1.02`` (the exponent scaled), the four proposal defects of chain_law,
``uniform-reused`` at n = 2, ``priori-dropped`` for TableFlip, ``window-top-open`` (a proposal with H(y) >= max is decided
by the entropy of the last bin instead of rejected); live tier: ``update-on-accept-only``, ``update-old-bin`` (m and the
histogram count go to the bin the walker left), ``stale-entropy`` (step t + 1 decides on S from before step t's
update).  A case's R is the smallest power of two >= 2^12 at which every defect the case detects at the cap, 2^18 (a
Wang-Landau walker owns L * F doubles of feature sums, and the CPU tier runs every case), is detected with probability
>= 0.99 by some statistic; tests/test_wl_law_host.py asserts that every defect is detected by some case at its R.

Cases and the kernel family each must report: see ``CASES``.  The general and universal twins run the n = 8 frozen law
of the fcc 2x2x2 cells (the two-sublattice cell, grown to depth 2, its n = 2 law).

Cells that differ from the ones first intended (the cells of chain_law's cases of the same name): fcc 2x2x2 swap has
three distinct enthalpies, so no window of it holds 4 occupied bins: fcc 2x2x3 swap stands for it (also under the general
and universal switches).  On rocksalt 2x2x4 flip with Ewald a few far outliers leave nearly every grown state in the
start's bin and the flat point never rejects: its window is the "core" one and its points are a ramp and the tilted one.
At update period 2 the single-class cells leave mc_wl_kernel (per-bin sums, period 1 only) for mc_lean_multi_kernel's
running-mean kernel, so the period-2 live laws of the fcc cells hold that kernel (``Case.family_ok``).  A 2 % error of
the exponent shows in one case only, fcc223-swap-descent, by the mean enthalpy after 64 steps (it also runs under the
general and universal switches); the other cases see gross acceptance errors.  The multi TableFlip family
(K_MULTI_TABLE_WL) runs on a cell of its own, ``_table_flip_two_sublattices``; kernel_info gives the multi families one
tag, so that case asserts lean-multi without kf=1 on a TableFlip handle.

Not covered: ``uniform-reused`` in the live tier (the frozen n = 2 laws carry it).  Live laws on the cells grown to
depth 2 other than rocksalt 3x2x2; n = 3 live on fcc 2x2x3 swap at period 1 (its outcomes pool 7 % of the mass at 2^18
walkers; it runs at period 2) and on rocksalt 3x2x2 (that needs the cell grown to depth 3).  The laws of exchange_wl,
wl_synchronise, grid exchange and population annealing: their decisions are bit-equal to NumPy
definitions and their uniforms come from the host.  Flatness checks (check_period > 0): the chain then has no fixed law;
tests/test_gpu_wl_windows.py's enumeration stands for them."""

import collections
import functools

import numpy as np

from smol_amd import capi, synth
from tests import chain_law as cl
from tests.chain_law import (Expected, Law, Sample, _fcc, _rocksalt_ewald, _table_flip, _two_sublattices, detection,  # noqa: F401
                             evaluate, passes)
from tests.wl_window_oracle import top as _top

FAMILY_ALPHA = cl.FAMILY_ALPHA
R_MIN, R_CAP = 1 << 12, 1 << 18
HOST_R = 1 << 16
M_FROZEN, M_LIVE = 2.0 ** -64, 0.75
LIVE_NS, LIVE_PERIODS = (2, 3), (1, 2)
START_QUANTILES = (0.5, 0.25, 0.75, 0.1, 0.9, 0.0, 0.999)  # of H over the grown set: the starts tried, in this order
PAD = 0.37  # the grid lies this fraction of a bin around the enumerated enthalpies

LIVE_DEFECTS = ("update-on-accept-only", "update-old-bin", "stale-entropy")
DEFECTS = ("entropy-1.02", "last-site-never", "partner-any-site", "flip-any-code", "uniform-reused", "uniform-sublattice",
           "priori-dropped", "window-top-open") + LIVE_DEFECTS

Window = collections.namedtuple("Window", "vmin vmax bin L")


def bins_of(w, H):
    """(bin of every H clipped into the window's rows, inside the window)"""
    H = np.asarray(H, dtype=np.float64)
    b = np.floor((H - w.vmin) / w.bin)
    return np.clip(b, 0, w.L - 1).astype(np.int64), (H >= w.vmin) & (H < w.vmax)


def edge_distance(w, H):
    """Smallest distance, in bins, of any H from an edge of the window's grid (continued beyond the window)."""
    f = np.mod((np.asarray(H) - w.vmin) / w.bin, 1.0)
    return float(np.minimum(f, 1.0 - f).min())


class WLFrozenLaw(Law):
    """The Wang-Landau chain with entropies that do not move: ``points`` one (window kind, S0 kind) per state point,
    window kind None / "top" / "bottom" (bins of the grid cut off there; ``need_outside``: at least 5 % of the first
    step's proposals must fall outside) / "core" (the grid spans the 5 % .. 95 % quantiles of the enumerated enthalpies:
    for a cell whose few far outliers would leave nearly every state in the start's bin), S0 kind "flat" / "tilted" /
    "ramp" (1 + c b) / "descent" (1 + c (L - 1 - b), c solved for a first-step rejection of 1/3).  The start is the
    first of the ``START_QUANTILES`` of H over the set grown from the cell's own start at which ``_design`` finds a window."""

    defects = DEFECTS

    def __init__(self, tab, step, start, points, depth=None, need_outside=True):
        self.points, self._shared, self.need_outside = tuple(points), {}, need_outside
        kinds = sorted({k for k, _ in points}, key=str)
        args = ([tab] * len(points), step)
        super().__init__(*args, start, (1.0,) * len(points), depth=depth)
        st = self.structure(None)  # the candidates for the start: quantiles of H over the set grown from the cell's own start
        ranked = st["states"][np.argsort(st["H"][0], kind="stable")]
        for quantile in START_QUANTILES:
            super().__init__(*args, ranked[min(int(quantile * len(ranked)), len(ranked) - 1)], (1.0,) * len(points), depth=depth)
            wins = _design(self, kinds)
            if wins:
                break
        else:
            raise AssertionError("no start and window meet the conditions")
        self.start_quantile = quantile
        self.windows = [wins[k] for k, _ in points]
        self.S0 = [_entropy(self, wins[k], s) for k, s in points]

    def _energy(self, g, key):  # (one table for every state point, and for every start tried)
        hit = self._shared.get(key)
        if hit is None:
            hit = self._shared[key] = Law._energy(self, 0, key)
        return hit

    # ---- the accept rule ---------------------------------------------------------------------------------------
    def _exponent(self, st, g, S, edges=slice(None), priori=True):
        w = self.windows[g]
        b, inside = bins_of(w, st["H"][g])
        row, col = st["row"][edges], st["col"][edges]
        ex = S[b[row]] - S[b[col]] + (st["lp"][edges] if priori else 0.0)
        return ex, inside[col], st["H"][g][col] >= w.vmax

    def _acceptance(self, st, g, defect=None, S=None, edges=slice(None)):
        ex, inside, above = self._exponent(st, g, self.S0[g] if S is None else S, edges, priori=defect != "priori-dropped")
        if defect == "entropy-1.02":
            ex = 1.02 * ex
        a = np.exp(np.minimum(ex, 0.0))
        a[~(inside | above if defect == "window-top-open" else inside)] = 0.0  # (above: b is clipped to the last bin)
        a[st["forced"][edges]] = 0.0
        return a

    def _log_weight(self, st, g):
        b, inside = bins_of(self.windows[g], st["H"][g])
        return np.where(inside, -self.S0[g][b], -np.inf)

    def first_step(self, g):
        """(mass proposed outside the window, mass rejected by the entropy rule) of the first step"""
        st = self.structure(None)
        e = np.flatnonzero(st["row"] == 0)
        ex, inside, _ = self._exponent(st, g, self.S0[g], e)
        q = st["q"][e]
        return float(q[~inside].sum()), float((q * (1.0 - np.exp(np.minimum(ex, 0.0))))[inside].sum())

    def top_mass(self, g):
        """mass of the enumerated proposals from inside the window to H(y) >= max (what window-top-open can show)"""
        st = self.structure(None)
        return float(st["q"][(st["H"][g][st["col"]] >= self.windows[g].vmax) & (st["H"][g][st["row"]] < self.windows[g].vmax)].sum())

    def applicable(self, n):
        d = ["entropy-1.02" if x == "beta-1.02" else x for x in super().applicable(n)]
        if any(self.top_mass(g) > 0 for g in range(self.G)):
            d.append("window-top-open")
        return d

    def features(self, g, occ):
        return self._ev[g].feature_vector(np.asarray(occ, dtype=np.int32))


def _grid(H, L):
    b = float(np.ptp(H)) / (L - 2.0 * PAD)
    return float(H.min()) - PAD * b, b


def _design(law, kinds):
    """{window kind: Window} on one grid: the smallest L >= 5 (and the smallest cut) at which every kind's window holds
    the start and at least 4 occupied bins, no state lies within 1e-6 bin of an edge, a cut window has at least 5 % of
    the first step's proposals outside, and the kind's first state point rejects the first step with probability in
    [0.25, 0.75] (the solved entropies reach their own target, or 0.8 of what the cell allows); None when there is none."""
    st = law.structure(None)
    H = st["H"][0]
    whole = kinds in ([None], ["core"])
    core = H[(H >= np.quantile(H, 0.05)) & (H <= np.quantile(H, 0.95))] if kinds == ["core"] else H
    for L in range(5, 25):
        v0, bsz = _grid(core, L)
        for k in range(0 if whole else 1, L - 3):
            out = {}
            for kind in kinds:
                lo, n = (k, L - k) if kind == "bottom" else (0, L - k if kind == "top" else L)
                vmin = v0 + lo * bsz
                w = Window(vmin, _top(vmin, n, bsz), bsz, n)
                b, inside = bins_of(w, H)
                if not inside[0] or len(np.unique(b[inside])) < 4 or edge_distance(w, H) < 1e-6:
                    break
                probe = next(s0 for kd, s0 in law.points if kd == kind)  # (the other points solve for their rejection)
                law.windows, law.S0 = [w] * law.G, [_entropy(law, w, probe)] * law.G
                outside, rejected = law.first_step(0)
                if not 0.25 <= rejected <= 0.75 or (kind in ("top", "bottom") and law.need_outside and outside < 0.05):
                    break
                out[kind] = w
            if len(out) == len(kinds):
                return out
            if whole:
                break
    return None


def _entropy(law, w, kind):
    st = law.structure(None)
    b, inside = bins_of(w, st["H"][0])
    if kind == "flat":
        g = np.bincount(b[inside], minlength=w.L)
        return 1.0 + np.log(np.maximum(g, 1))
    shape = {"ramp": np.arange(w.L), "descent": np.arange(w.L)[::-1], "tilted": np.abs(np.arange(w.L) - b[0])}[kind].astype(np.float64)
    e = np.flatnonzero(st["row"] == 0)
    q, col = st["q"][e], st["col"][e]
    ok = inside[col] & ~st["forced"][e]

    def rejected(c):
        return float((q * (1.0 - np.exp(np.minimum(c * (shape[b[0]] - shape[b[col]]) + st["lp"][e], 0.0))))[ok].sum())
    lo, hi = 0.0, 64.0
    target = min(1.0 / 3.0 if kind == "descent" else 0.5, 0.8 * rejected(hi))
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if rejected(mid) < target else (lo, mid)
    return 1.0 + hi * shape


# ---- the live tier: the law over paths -----------------------------------------------------------------------------
def path_expected(law, g, n, period, defect=None, m=M_LIVE):
    """Expected over the rows [occupancy | histogram row | n_accepted] after n steps from S0 with modification factor m.
    ``dependent`` (attribute): per step, the path mass through a decision whose acceptance differs from that under S0."""
    key = ("live", g, n, period, defect, m)
    if key in law._laws:
        return law._laws[key]
    assert law.depth is None or n <= law.depth
    st = law.structure(defect)
    order = np.argsort(st["row"], kind="stable")
    lo = np.searchsorted(st["row"][order], np.arange(len(st["states"]) + 1))
    w, S0 = law.windows[g], law.S0[g]
    b, _ = bins_of(w, st["H"][g])
    zero = (0,) * w.L
    nodes = {(0, zero, zero, 0): 1.0}  # (state, histogram, the histogram the next decision sees, n_accepted)
    pacc, dependent = [], []
    for t in range(1, n + 1):
        nxt = collections.defaultdict(float)
        acc = dep = 0.0
        update = t % period == 0
        for (x, hist, seen, k), pr in nodes.items():
            e = order[lo[x]:lo[x + 1]]
            a = law._acceptance(st, g, defect, S0 + m * np.array(seen), e)
            dep += pr * float(st["q"][e][np.abs(a - law._acceptance(st, g, defect, S0, e)) > 1e-12].sum())
            moves = collections.defaultdict(float)
            for y, qa in zip(st["col"][e], st["q"][e] * a):
                if qa > 0.0:
                    moves[(int(y), 1)] += qa
            stay = float((st["q"][e] * (1.0 - a)).sum())
            if stay > 0.0:
                moves[(x, 0)] += stay
            for (y, accepted), pm in moves.items():
                new = hist
                if update and (accepted or defect != "update-on-accept-only"):
                    c = b[x] if defect == "update-old-bin" else b[y]
                    new = hist[:c] + (hist[c] + 1,) + hist[c + 1:]
                nxt[(y, new, hist if defect == "stale-entropy" else new, k + accepted)] += pr * pm
                acc += pr * pm * accepted
        nodes = nxt
        pacc.append(acc)
        dependent.append(dep)
    out = collections.defaultdict(float)
    for (x, hist, _, k), pr in nodes.items():
        out[(x, hist, k)] += pr
    keys = list(out)
    rows = np.array([np.concatenate([st["states"][x], hist, [k]]) for x, hist, k in keys], dtype=np.int8)
    p = np.array([out[k] for k in keys])
    assert abs(p.sum() - 1.0) < 1e-12, p.sum()
    exp = Expected(rows, p[:, None], st["H"][g][[x for x, _, _ in keys]], pacc, n)
    exp.dependent = dependent
    law._laws[key] = exp
    return exp


class WLPathLaw:
    """The live tier of a ``WLFrozenLaw``'s cell: its proposals, windows and S0 with a modification factor that moves S."""

    def __init__(self, law, m=M_LIVE):
        self.law, self.m = law, m

    def expected(self, g, n, period, defect=None):
        return path_expected(self.law, g, n, period, defect, self.m)


# ---- the cases -----------------------------------------------------------------------------------------------------
def _wl(build, points=((None, "flat"), (None, "tilted")), depth=None, need_outside=True):
    """A WLFrozenLaw on the cell of a chain_law builder (its tables, step type and start)."""
    def make():
        base = build() if callable(build) else build
        src = base["law"]
        law = WLFrozenLaw(base["tab"], src.step, src.start, points, depth=depth, need_outside=need_outside)
        return dict(tab=base["tab"], law=law)
    make.groups = len(points)
    return make


def _table_flip_two_sublattices():
    """Two charge-neutral directions that span both sublattices of rocksalt 2x2x2 with two anions (Mn3+ -> Li+ with 2 O2- ->
    2 F-; Ti4+ -> Mn3+ with O2- -> F-), from 5 Li+ + 2 Mn3+ + Ti4+ | 7 O2- + F-: the smallest cell on the multi TableFlip
    kernels."""
    model = synth.build_cluster_model(synth.rocksalt_prim(anion_charges=(-2.0, -1.0)), {2: 6.0, 3: 4.5})
    sc = synth.build_supercell(model, [2, 2, 2])
    tab = capi.TableSet.from_synth(sc, synth.random_coefs(model, seed=11, scale=0.03),
                                   flip_table=np.array([[1, -1, 0, -2, 2], [0, 1, -1, -1, 1]]), swap_weight=0.3)
    occ = np.zeros(sc.num_sites, dtype=np.int32)
    occ[: sc.size] = [0, 1, 0, 0, 2, 0, 1, 0]
    occ[sc.size + 3] = 1
    return dict(tab=tab, law=Law([tab], capi.STEP_TABLE_FLIP, occ, (1.0,), depth=2))


class Case:
    """name; build() -> dict(tab, law); the n of the frozen tier and of the live tier; update_period of the frozen tier;
    the substrings kernel_info must / must not hold under ``env``; ``twin`` = the case whose law and seeds it shares."""

    def __init__(self, name, build, ns, live=(), period=1, want=("^lean ", " wl=v3"), wont=(), env=None, host=True, twin=None):
        self.name, self._build, self.ns, self.period = name, build, tuple(ns), period
        # (live: n alone = at every period of LIVE_PERIODS, or (n, period))
        self.live = tuple(x for item in live
                          for x in ([item] if isinstance(item, tuple) else [(item, p) for p in LIVE_PERIODS]))
        self.want, self.wont, self.env, self.host, self.twin = tuple(want), tuple(wont), dict(env or {}), host, twin

    @functools.cached_property
    def built(self):
        return CASES[self.twin].built if self.twin else self._build()

    @property
    def law(self):
        return self.built["law"]

    @property
    def groups(self):
        return CASES[self.twin].groups if self.twin else self._build.groups

    @property
    def seed_base(self):
        return 2_000_003 * (1 + list(CASES).index(self.twin or self.name))

    def family_ok(self, info, period=1):
        """mc_wl_kernel keeps per-bin feature sums and runs at update period 1 only: at another period the single-class
        cells run mc_lean_multi_kernel's running-mean kernel; the TableFlip kernel has a running-mean variant of its own."""
        want = self.want
        if period != 1 and "^lean " in want:
            swap = ({" wl=table": " wl=table-mean"} if " wl=table" in want
                    else {"^lean ": "^lean-multi", " wl=v3": " wl=multi-mean", " gx=": " wl=multi-mean"})
            want = tuple(swap.get(w, w) for w in want)
        head = info.split(" env=")[0]
        return all((head.startswith(w[1:]) if w.startswith("^") else w in head) for w in want) and not any(w in head for w in self.wont)

    def laws(self):
        """("frozen", g, n, period) and ("live", g, n, period)"""
        G = self.law.G
        return ([("frozen", g, n, self.period) for g in range(G) for n in self.ns]
                + [("live", g, n, p) for g in range(G) for n, p in self.live])

    def runs(self):
        """(tier, n, period): one launch each"""
        return [("frozen", n, self.period) for n in self.ns] + [("live", n, p) for n, p in self.live]

    def expected(self, key, defect=None):
        tier, g, n, period = key
        return self.law.expected(g, n, defect) if tier == "frozen" else WLPathLaw(self.law).expected(g, n, period, defect)

    def applicable(self, key):
        tier, g, n, period = key
        d = self.law.applicable(n)
        if tier == "live":
            d = [x for x in d if x != "uniform-reused"] + list(LIVE_DEFECTS)
        return d

    @property
    def r_cap(self):
        """walkers per state point at most: one launch holds every state point and at most 2^18 walkers"""
        return R_CAP >> int(np.ceil(np.log2(self.groups)))

    @functools.cached_property
    def R(self):
        return cap_respecting_R(self, choose_R(self)[0])


SWAP, FLIP = capi.STEP_SWAP, capi.STEP_FLIP
TINY_NS = cl.TINY_NS
WINDOWS = (("top", "flat"), ("top", "tilted"), ("bottom", "flat"), ("bottom", "tilted"))
GENERAL, UNIVERSAL = {"SMOLMC_FORCE_GENERAL": "1"}, {"SMOLMC_FORCE_UNIVERSAL": "1"}
CASES = {c.name: c for c in [
    # mc_wl_kernel: the tiny cells to closure, frozen and live
    Case("fcc222-flip", _wl(_fcc([2, 2, 2], FLIP, mu=cl.MU2, depth=None)), TINY_NS, live=LIVE_NS),
    Case("fcc223-swap", _wl(_fcc([2, 2, 3], SWAP, depth=None)), TINY_NS, live=(2, (3, 2))),
    # a gentle descending entropy: the point at which the mean enthalpy after 64 steps shows a 2 % error of the exponent
    Case("fcc223-swap-descent", _wl(_fcc([2, 2, 3], SWAP, depth=None), ((None, "descent"), (None, "tilted"))), (8, 64)),
    Case("fcc222-flip-top-cut", _wl(_fcc([2, 2, 2], FLIP, mu=cl.MU2, depth=None), (("top", "flat"), ("top", "tilted"))), TINY_NS, live=(2,)),
    Case("fcc223-swap-bottom-cut", _wl(_fcc([2, 2, 3], SWAP, depth=None), (("bottom", "flat"), ("bottom", "tilted"))), TINY_NS),
    # ... with the Ewald field (kernel_info: mc_wl_kernel's tag gives way to the one of the translation-compressed field)
    Case("rocksalt224-ewald-flip", _wl(_rocksalt_ewald(FLIP), (("core", "ramp"), ("core", "tilted")), depth=2), (1, 2),
         want=("^lean ", "field=1", " gx=")),
    Case("rocksalt224-ewald-swap", _wl(_rocksalt_ewald(SWAP), depth=2), (1, 2), want=("^lean ", "field=1", " gx=")),
    # per-walker windows: two overlapping windows, two entropies each, four groups of one handle
    Case("fcc223-swap-windows", _wl(_fcc([2, 2, 3], SWAP, depth=None), WINDOWS, need_outside=False), TINY_NS,
         want=("^lean ", " wl=v3", "wl_windows=1")),
    # mc_lean_multi_kernel: per-bin sums at update period 1, running means at 2; its windows variant
    Case("rocksalt322-two-sublattices", _wl(_two_sublattices(), depth=2), (1, 2), live=(2,), want=("^lean-multi", " wl=multi")),
    Case("rocksalt322-two-sublattices-period2", None, (1, 2), period=2, want=("^lean-multi", " wl=multi-mean"),
         twin="rocksalt322-two-sublattices"),
    Case("rocksalt322-two-sublattices-windows", _wl(_two_sublattices(), WINDOWS, depth=2, need_outside=False), (1, 2),
         want=("^lean-multi", " wl=multi", "wl_windows=1")),
    Case("fcc223-ternary-corr-kf", _wl(_fcc([2, 2, 3], SWAP, nspecies=3, mode=capi.FEATURES_CORRELATIONS), depth=2), (1, 2),
         want=("^lean-multi", " kf=1", " wl=multi")),
    # TableFlip with its a-priori factor
    Case("rocksalt222-table-flip", _wl(_table_flip, depth=2), (1, 2), want=("^lean ", " wl=table")),
    Case("rocksalt222-table-flip-two-sublattices", _wl(_table_flip_two_sublattices, depth=2), (1, 2),
         want=("^lean-multi", " wl=multi"), wont=(" kf=1",)),
    # mc_kernel and the universal kernel: the n = 8 law of the tiny cells (the two-sublattice cell: its n = 2 law)
    Case("fcc223-swap-general", None, (8,), want=("^general",), env=GENERAL, host=False, twin="fcc223-swap"),
    Case("fcc222-flip-general", None, (8,), want=("^general",), env=GENERAL, host=False, twin="fcc222-flip"),
    Case("fcc223-swap-descent-general", None, (64,), want=("^general",), env=GENERAL, host=False, twin="fcc223-swap-descent"),
    Case("rocksalt322-general", None, (2,), want=("^general",), env=dict(GENERAL, SMOLMC_NO_WL_MULTI="1"), host=False,
         twin="rocksalt322-two-sublattices"),
    Case("fcc223-swap-universal", None, (8,), want=("^universal",), env=UNIVERSAL, host=False, twin="fcc223-swap"),
    Case("fcc222-flip-universal", None, (8,), want=("^universal",), env=UNIVERSAL, host=False, twin="fcc222-flip"),
    Case("fcc223-swap-descent-universal", None, (64,), want=("^universal",), env=UNIVERSAL, host=False, twin="fcc223-swap-descent"),
    Case("rocksalt322-universal", None, (2,), want=("^universal",), env=dict(UNIVERSAL, SMOLMC_NO_WL_MULTI="1"), host=False,
         twin="rocksalt322-two-sublattices"),
]}
DISPATCH_SWITCHES = cl.DISPATCH_SWITCHES + ("SMOLMC_NO_WL_MULTI", "SMOLMC_NO_LEAN_MULTI", "SMOLMC_WL_RUNNING_MEAN", "SMOLMC_LAUNCH_CHUNK",
                                            "SMOLMC_FAST_EPS_SCALE", "SMOLMC_MULTI_PHI_HBM", "SMOLMC_MULTI_PHI_LDS", "SMOLMC_NO_ROTATE")

HOST_RUNS = [(c.name,) + r for c in CASES.values() if c.host for r in c.runs()]
DEVICE_RUNS = [(c.name,) + r for c in CASES.values() for r in c.runs()]
N_STATISTICS = 3 * sum(CASES[r[0]].groups for r in HOST_RUNS + DEVICE_RUNS)
ALPHA = FAMILY_ALPHA / N_STATISTICS


@functools.lru_cache(maxsize=None)
def power_of(case, R):
    """{defect: (best detection probability over the case's laws, the law)} at R walkers per state point."""
    out = {}
    for key in case.laws():
        exp = case.expected(key)
        for d in case.applicable(key):
            p = detection(exp, case.expected(key, d), R, ALPHA)
            if p > out.get(d, (-1.0, None))[0]:
                out[d] = (p, key)
    return out


@functools.lru_cache(maxsize=None)
def choose_R(case):
    """(R, {defect: (detection probability at R, law)}, defects the case cannot detect at the cap)."""
    cap = power_of(case, case.r_cap)
    drive = [d for d, (p, _) in cap.items() if p >= 0.99]
    R = R_MIN
    while R < case.r_cap and not all(power_of(case, R)[d][0] >= 0.99 for d in drive):
        R *= 2
    return R, power_of(case, R), sorted(set(cap) - set(drive))


@functools.lru_cache(maxsize=None)
def pooled_mass(case, R):
    return max(case.expected(key).cells(R)[2] for key in case.laws())


def cap_respecting_R(case, R):
    """R doubled until the pooled cell of every law of the case holds at most 5 % of the mass."""
    while R < case.r_cap and pooled_mass(case, R) > 0.05:
        R *= 2
    return R


def assert_pooling_cap(case, R):
    assert pooled_mass(case, R) <= 0.05, (case.name, R, pooled_mass(case, R))


def conditions(case):
    """The conditions on the inputs, asserted on the law alone; returns what it measured."""
    law, out = case.law, {}
    st = law.structure(None)
    for g in range(law.G):
        w = law.windows[g]
        b, inside = bins_of(w, st["H"][g])
        assert inside[0] and np.all(law.S0[g] >= 1.0) and len(law.S0[g]) == w.L
        assert int(np.ceil((w.vmax - w.vmin) / w.bin)) == w.L == law.windows[0].L
        assert edge_distance(w, st["H"][g]) >= 1e-6, (case.name, g)
        assert len(np.unique(b[inside])) >= 4, (case.name, g)
        outside, rejected = law.first_step(g)
        assert 0.25 <= rejected <= 0.75, (case.name, g, rejected)
        if law.points[g][0] in ("top", "bottom") and law.need_outside:
            assert outside >= 0.05, (case.name, g, outside)
        out[g] = dict(L=w.L, occupied=len(np.unique(b[inside])), outside=outside, rejected=rejected)
    assert np.ptp(law.S0[0]) > 0 and not np.array_equal(law.S0[0], law.S0[1])
    for key in case.laws():
        if key[0] == "live":  # (at period 2 the first update follows step 2: only the third step can see it)
            dep = case.expected(key).dependent
            out[key] = max(dep[1:])
            assert out[key] >= 0.10 or (key[3] == 2 and key[2] == 2 and out[key] == 0.0), (case.name, key, dep)
    return out


# ---- running a case on an engine or the oracle ----------------------------------------------------------------------
FULL_R = ("fcc223-swap-descent", "frozen", 8, 1)  # the run the CPU tier makes at the device's R (2^17, twice its own)
_ORACLE = {}


def host_R(case, run=None):
    """Walkers per state point of the CPU tier: 2^16 (doubled while the pooling cap asks for it), never beyond the
    device's R; the device's R for FULL_R."""
    if run is not None and (case.name,) + tuple(run) == FULL_R:
        return case.R
    return min(case.R, cap_respecting_R(case, HOST_R))


def seeds_for(case, g, R, run):
    tier, n, period = run
    return (np.arange(R, dtype=np.uint64) + np.uint64(case.seed_base + g * R_CAP + 7919 * n + 104_729 * period
                                                     + (300_000_000 if tier == "live" else 0)))


def config_for(case, groups, R, run):
    tier, n, period = run
    w = case.law.windows[groups[0]]
    return capi.make_config(len(groups) * R, capi.KERNEL_WANGLANDAU, case.law.step, min_enthalpy=w.vmin, max_enthalpy=w.vmax,
                            bin_size=w.bin, mod_factor=1.0, check_period=0, update_period=period)


def prepare(case, handle, groups, R, run, m):
    """The state of the run (tier, n, period) on a handle whose walkers are the ``groups`` (state points) of the case, R
    each: the windows where they differ, the start, the seeds, the entropies and the modification factor.  Returns the
    entropies (len(groups) * R, L)."""
    law = case.law
    wins = [law.windows[g] for g in groups]
    if len(set(wins)) > 1:
        handle.set_wl_windows(np.repeat([w.vmin for w in wins], R), np.repeat([w.vmax for w in wins], R))
    occ = np.tile(law.start.astype(np.int32), (len(groups) * R, 1))
    handle.set_state(occ, np.concatenate([seeds_for(case, g, R, run) for g in groups]), np.full(len(groups) * R, 1000.0))
    S0 = np.repeat(np.array([law.S0[g] for g in groups]), R, axis=0)
    handle.set_wl(entropy=S0, mod_factor=np.full(len(groups) * R, m))
    return S0


def run_handle(case, handle, groups, R, run, head=None):
    """One launch of the run (tier, n, period): ``prepare``, n steps, the per-walker identities asserted; returns [Sample
    per group] -- with ``head``, ([Sample per group], [Sample of the first ``head`` walkers per group])."""
    tier, n, period = run
    law = case.law
    m = M_FROZEN if tier == "frozen" else M_LIVE
    S0 = prepare(case, handle, groups, R, run, m)
    handle.run(n)
    st, wl = handle.get_state(), handle.get_wl()
    assert np.all(st["n_steps"] == n)
    hist = wl["histogram"]
    assert np.all(hist.sum(axis=1) == n // period), "histogram.sum() != n // update_period"
    assert np.array_equal(wl["occurrences"], hist), "occurrences != histogram"
    assert np.all(wl["mod_factor"] == m)
    if tier == "frozen":
        assert np.array_equal(wl["entropy"], S0), "the frozen entropy moved"
    else:
        np.testing.assert_allclose(wl["entropy"], S0 + m * hist, rtol=1e-12, atol=0)
    def sample(sl):
        if tier == "frozen":
            return Sample(st["occupancy"][sl], st["n_accepted"][sl], st["enthalpy"][sl])
        return Sample(np.column_stack([st["occupancy"][sl], hist[sl], st["n_accepted"][sl].astype(np.int64)]),
                      np.zeros(sl.stop - sl.start, dtype=np.int64), st["enthalpy"][sl])

    out, heads = [], []
    for k, g in enumerate(groups):
        sl = slice(k * R, (k + 1) * R)
        s = sample(sl)
        if head is not None:
            heads.append(s if head == R else sample(slice(k * R, k * R + head)))
        if n == 1:  # mean_features[b(final)] is the final state's features: one entry, the mean of one
            rows, inverse = np.unique(st["occupancy"][sl], axis=0, return_inverse=True)
            feat = np.array([law.features(g, r) for r in rows])
            b, inside = bins_of(law.windows[g], feat @ law._nat[g])
            assert inside.all()
            got = wl["mean_features"][sl][np.arange(R), b[inverse.ravel()]]
            np.testing.assert_allclose(got, feat[inverse.ravel()], rtol=1e-10, atol=1e-9)
        out.append(s)
    return out if head is None else (out, heads)


def oracle_samples(name, run, R=None):
    """[Sample per state point] of the CPU oracle's chains (one oracle per state point: it has one window)."""
    from oracle import oracle as orc

    case = CASES[name]
    R = host_R(case, run) if R is None else R
    key = (case.twin or name, tuple(run), R)
    if key not in _ORACLE:
        out = []
        for g in range(case.law.G):
            ora = orc.OracleMC(case.built["tab"], config_for(case, [g], R, run))
            out += run_handle(case, ora, [g], R, run)
            del ora
        _ORACLE[key] = out
    return _ORACLE[key]


def report(case, key, res, where):
    tier, g, n, period = key
    line = (f"[wl law] {case.name} {tier} g={g} n={n} period={period} on {where}: R={res['R']} df={res['df']} "
            f"p_chi2={res['p_chi2']:.3g}" + (f" z_acc={res['z_acc']:+.2f}" if "z_acc" in res else "")
            + f" z_H={res['z_H']:+.2f} zero={res['zero']} trace_err={res.get('trace_err', 0.0):.1e} alpha={ALPHA:.2e}")
    print(line)
    return line
