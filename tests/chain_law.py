"""The exact transition law of the plain Flip / Swap Metropolis chains, and the statistics that hold a batch of
walkers against it (tests/test_chain_law_host.py on the CPU oracle, tests/test_gpu_chain_law.py on the device).

The parity suite pins the kernels to the CPU oracle bit for bit; the oracle's energies are pinned to the reference,
its native random stream is pinned to nothing.  Here the chain is held against the law of the reference's ushers and
accept rule, restated in float64 NumPy from their documented semantics:

* sublattice with probability ``sub_probs`` (MCUsher.get_random_sublattice, mcusher.py:146-148);
* Flip (mcusher.py:167-170): site uniform over the sublattice's active sites, new code uniform over its OTHER codes;
* Swap (mcusher.py:189-200): site 1 uniform over the active sites, site 2 uniform over the active sites of the
  sublattice whose species differs; no such site: the step is the empty list;
* Metropolis (metropolis.py:40-48): exponent = -beta dH (+ d bias); accepted when exponent >= 0, else with
  probability exp(exponent).  An EMPTY step has dH = 0, so exponent = 0 >= 0: it IS accepted (base.py:160-163 run
  the accept rule on every proposed step, the empty one included), the occupancy stays and the accept counter
  moves.  So on a one-species start every step counts as accepted, and with all-zero coefficients every step does.

Energies and bias terms of a state come from the from-scratch evaluators of the oracle that the golden fixtures pin
to the reference (OracleEvaluator.feature_vector @ natural_parameters -- the chemical work is the last feature,
with parameter -1 -- and OracleEvaluator.bias), never from a running trace or a delta.

From a fixed start state the law after n steps is e_start P^n.  The reachable set is grown step by step from the
start (to closure on the tiny cells, to depth 2 on the small ones), P is a sparse matrix over it.  A walker's outcome
is (final occupancy, n_accepted) for n <= 2 and the final occupancy for larger n; R walkers with different seeds are
R independent draws.  Per law three statistics:

  (a) Pearson chi-square over the outcomes, outcomes of expected count < 5 pooled into one cell (at most 5 % of the
      mass, asserted on the law before any chain runs); p-value from chi2.sf.  A walker on an outcome of
      probability zero is a failure on its own;
  (b) at n = 1, z of the total accepted count against R p (1 - p) (or equality where p is 0 or 1);
  (c) z of the mean of the handle's running enthalpy against the exact mean and variance of H under the law; every
      walker's running enthalpy must also equal the from-scratch H of its final state (rtol 1e-10, atol 1e-9).

One family-wise level, 1e-3, split evenly over ``N_STATISTICS``: three per (case, state point, n) and per module that
runs the case -- an upper bound of what is evaluated (a statistic whose variance is zero becomes an equality), so the
split is conservative.  Seeds are fixed.

Power: six defects (and a seventh for TableFlip), each a variation of THIS law (never of the engine); for each law
of a case and each defect that applies, the non-centrality R sum (p_def - p)^2 / p over the cells gives the detection probability of (a) from
scipy.stats.ncx2, the shift in standard errors that of (b) and (c), mass on outcomes the law excludes that of the
zero-probability rule.  A case's R is the smallest power of two (>= 2^12, <= 2^21) at which every defect the case
can detect at all at 2^21 is detected with probability >= 0.99 by at least one statistic of the case; a defect a
case cannot detect at 2^21 does not drive that case's R (it would only pin the case at the cap), and
tests/test_chain_law_host.py asserts that every defect is detected by some case at that case's R.

Not covered by any case: no defect (tests/test_chain_law_host.py::test_every_defect_is_detected_by_some_case); one law
the plan named: the TWO-step law of the half-filled fcc 4x4x4 swap (with and without energies).  It has 247 041 states,
a two-swap state has probability 4 / 1024^2 at most, so the pooled cell holds 94 % of the mass at 2^20 walkers and the
5 % cap is met only at the 2^21 ceiling (expected count 8 per state): 2^21 walkers of 64 sites per launch and 10 s to
grow the law, against a few seconds per test.  The two-step swap law on 4x4x4 runs from the skewed start (2016
states) and on 3x3x3; the half-filled 4x4x4 swap runs its one-step law.  Wang-Landau has a tier of its own, tests/wl_law.py: its
chain has a fixed law while the entropies are frozen, and a law over short paths while they move.  Out of scope: the
replica-exchange moves, population annealing (its own enumeration test).  TableFlip has one case (the one- and two-step law of a one-direction table);
the two detailed-balance tests of tests/test_gpu_table_flip.py stay."""

import functools

import numpy as np
from scipy import sparse, stats

from smol_amd import capi
from smol_amd import ewald as ew
from smol_amd import moca, synth

KB = moca.kB
FAMILY_ALPHA = 1e-3
R_MIN, R_CAP = 1 << 12, 1 << 21
HOST_R = 1 << 16  # walkers per state point of the CPU tier

DEFECTS = ("beta-1.02", "last-site-never", "partner-any-site", "flip-any-code", "uniform-reused", "uniform-sublattice",
           "priori-dropped")  # (the seventh is TableFlip's own: the a-priori factor left out of the exponent)
_PROPOSAL_DEFECTS = ("last-site-never", "partner-any-site", "flip-any-code", "uniform-sublattice")

_HASH_W = np.random.default_rng(20261018).integers(1, 1 << 63, size=4096, dtype=np.uint64) | np.uint64(1)


def state_hash(rows, nacc=None):
    """A 64-bit word per row of ``rows`` (n, N): sum of code * odd weight, wrapping (+ the accept count's share)."""
    rows = np.asarray(rows)
    out = np.empty(len(rows), dtype=np.uint64)
    W = _HASH_W[: rows.shape[1]]
    for a in range(0, len(rows), 1 << 17):
        out[a:a + (1 << 17)] = (rows[a:a + (1 << 17)].astype(np.uint64) * W).sum(axis=1, dtype=np.uint64)
    if nacc is not None:
        out += np.asarray(nacc).astype(np.uint64) * _HASH_W[-1]
    return out


class Sample:
    """The outcomes of R walkers, compacted: distinct (occupancy, n_accepted) rows and how many walkers ended there."""

    def __init__(self, occupancy, n_accepted, enthalpy=None):
        occupancy, n_accepted = np.asarray(occupancy), np.asarray(n_accepted).astype(np.int64)
        _, first, inverse, counts = np.unique(state_hash(occupancy, n_accepted), return_index=True, return_inverse=True,
                                              return_counts=True)
        self.rows = occupancy[first].astype(np.int8)
        self.nacc, self.counts, self.R = n_accepted[first], counts.astype(np.int64), int(len(occupancy))
        self.hsum = self.hmin = self.hmax = None
        if enthalpy is not None:  # the handle's running enthalpy of the walkers of every outcome: sum, smallest, largest
            h = np.asarray(enthalpy, dtype=np.float64)
            self.hsum = np.bincount(inverse, weights=h, minlength=len(first))
            self.hmin, self.hmax = np.full(len(first), np.inf), np.full(len(first), -np.inf)
            np.minimum.at(self.hmin, inverse, h)
            np.maximum.at(self.hmax, inverse, h)

    def same_as(self, other):
        def key(s):
            o = np.lexsort(np.column_stack([s.rows, s.nacc]).T)
            return s.rows[o], s.nacc[o], s.counts[o]
        return self.R == other.R and len(self.counts) == len(other.counts) and all(
            np.array_equal(a, b) for a, b in zip(key(self), key(other)))


class Expected:
    """The law of one (state point, n): states (S, N) int8, p (S, n + 1) over (state, n_accepted) for n <= 2, else
    (S, 1) over the state; H (S,), the accept probability of every step and the exact mean enthalpy."""

    def __init__(self, states, p, H, p_accept, n):
        self.states, self.p, self.H, self.p_accept, self.n = states, p, H, p_accept, n
        self.joint = p.shape[1] > 1
        self.mean_H = float((p.sum(axis=1) * H).sum())
        self.var_H = float(max((p.sum(axis=1) * (H - self.mean_H) ** 2).sum(), 0.0))
        self._hash = state_hash(states)
        self._order = np.argsort(self._hash)
        assert len(np.unique(self._hash)) == len(states)

    def locate(self, rows):
        """Index of every row among the law's states, -1 where the law does not hold it."""
        h = state_hash(rows)
        pos = np.clip(np.searchsorted(self._hash[self._order], h), 0, len(self._order) - 1)
        idx = self._order[pos]
        ok = (self._hash[idx] == h) & np.all(self.states[idx] == np.asarray(rows, dtype=np.int8), axis=1)
        return np.where(ok, idx, -1)

    def cells(self, R):
        """(cell of every outcome (flat, -1 = probability zero), expected probability per cell, pooled mass): the
        outcomes of expected count >= 5 are cells of their own, the others share the last one; a pooled cell of
        expected count < 5 joins the smallest of the others."""
        p = self.p.ravel()
        own = R * p >= 5.0
        cell = np.full(len(p), -1, dtype=np.int64)
        cell[own] = np.arange(int(own.sum()))
        pe = list(p[own])
        pooled = float(p[~own].sum())
        rest = (~own) & (p > 0)
        if rest.any():
            if R * pooled >= 5.0 or not pe:
                cell[rest] = len(pe)
                pe.append(pooled)
            else:
                k = int(np.argmin(pe))
                cell[rest] = k
                pe[k] += pooled
        return cell, np.array(pe), pooled


def _sf2(z):
    return float(2.0 * stats.norm.sf(abs(z)))


def evaluate(exp, sample):
    """The statistics of ``sample`` under the law ``exp``: dict(R, zero, df, chi2, p_chi2, z_acc, p_acc, z_H, p_H,
    trace_err, worst) -- p-values of statistics that do not exist (one cell, zero variance) are 1.0 when the equality they turn
    into holds and 0.0 when not; ``worst`` lists the outcomes with the largest chi-square contributions."""
    R, n = sample.R, exp.n
    idx = exp.locate(sample.rows)
    known = idx >= 0
    known &= (sample.nacc >= 0) & (sample.nacc <= n)  # (an accept counter beyond the steps taken is no outcome of the law)
    flat = np.where(known, idx * exp.p.shape[1] + (sample.nacc if exp.joint else 0), 0)
    cell, pe, _ = exp.cells(R)
    c = np.where(known, cell[flat], -1)
    out = dict(R=R, zero=int(sample.counts[c < 0].sum()))
    obs = np.bincount(c[c >= 0], weights=sample.counts[c >= 0], minlength=len(pe))
    out["df"] = len(pe) - 1
    if len(pe) > 1:
        contrib = (obs - R * pe) ** 2 / (R * pe)
        out["chi2"] = float(contrib.sum())
        out["p_chi2"] = float(stats.chi2.sf(out["chi2"], len(pe) - 1))
        top = np.argsort(contrib)[::-1][:5]
        out["worst"] = [(int(k), float(obs[k]), float(R * pe[k]), float(contrib[k])) for k in top]
    else:
        out["chi2"], out["p_chi2"], out["worst"] = 0.0, 1.0, []
    if n == 1:
        pa = exp.p_accept[0]
        acc = float((sample.counts * sample.nacc).sum())
        var = R * pa * (1.0 - pa)
        if var > 1e-9:
            out["z_acc"] = (acc - R * pa) / np.sqrt(var)
            out["p_acc"] = _sf2(out["z_acc"])
        else:
            out["z_acc"], out["p_acc"] = 0.0, float(acc == round(R * pa))
    if sample.hsum is not None:  # the handle's running trace: its mean, and per outcome against the from-scratch H
        Hm = float(sample.hsum.sum() / R)
        want = exp.H[idx[known]]
        err = np.maximum(np.abs(sample.hmin[known] - want), np.abs(sample.hmax[known] - want)) - 1e-10 * np.abs(want)
        out["trace_err"] = float(err.max(initial=0.0))
    else:
        Hm = float((sample.counts[known] * exp.H[idx[known]]).sum() / R)
    if exp.var_H > 1e-24:
        out["z_H"] = (Hm - exp.mean_H) / np.sqrt(exp.var_H / R)
        out["p_H"] = _sf2(out["z_H"])
    else:
        out["z_H"], out["p_H"] = 0.0, float(out["zero"] > 0 or abs(Hm - exp.mean_H) <= 1e-9 * max(1.0, abs(exp.mean_H)))
    return out


def passes(res, alpha):
    return res["zero"] == 0 and res.get("trace_err", 0.0) <= 1e-9 and all(res.get(k, 1.0) >= alpha for k in ("p_chi2", "p_acc", "p_H"))


def detection(exp, bad, R, alpha):
    """Probability that R walkers drawn from the law ``bad`` fail the best single statistic of ``exp`` at level
    ``alpha``: max over (a) chi-square by its non-centrality, (b), (c) by their shift, and the zero rule."""
    if getattr(bad, "_projected", None) is None:  # the defect's law over the outcomes of ``exp``
        idx = exp.locate(bad.states)
        pd = np.zeros_like(exp.p)
        np.add.at(pd, idx[idx >= 0], bad.p[idx >= 0] if exp.joint else bad.p[idx >= 0].sum(axis=1, keepdims=True))
        bad._projected = (pd.ravel(), float(bad.p[idx < 0].sum()))
    pd, outside = bad._projected
    cell, pe, _ = exp.cells(R)
    outside += float(pd[cell < 0].sum())
    best = 1.0 - (1.0 - min(outside, 1.0)) ** R
    if len(pe) > 1:
        pdc = np.bincount(cell[cell >= 0], weights=pd[cell >= 0], minlength=len(pe))
        lam = float(R * ((pdc - pe) ** 2 / pe).sum())
        df = len(pe) - 1
        crit = stats.chi2.isf(alpha, df)
        if lam <= 1e-12:
            power = alpha
        elif lam < 1e3:
            power = float(stats.ncx2.sf(crit, df, lam))
        else:  # (ncx2.sf loses its footing at large non-centrality: the normal limit, mean df + lam, variance 2 (df + 2 lam))
            power = float(stats.norm.sf((crit - df - lam) / np.sqrt(2.0 * (df + 2.0 * lam))))
        best = max(best, power)
    zc = stats.norm.isf(alpha / 2.0)

    def shifted(mean0, sd0, mean1, sd1):
        if sd0 <= 0.0:
            return 0.0
        if sd1 <= 0.0:
            return float(abs(mean1 - mean0) > zc * sd0)
        return float(stats.norm.sf((mean0 + zc * sd0 - mean1) / sd1) + stats.norm.cdf((mean0 - zc * sd0 - mean1) / sd1))

    if exp.n == 1:
        p0, p1 = exp.p_accept[0], bad.p_accept[0]
        if R * p0 * (1 - p0) > 1e-9:
            best = max(best, shifted(R * p0, np.sqrt(R * p0 * (1 - p0)), R * p1, np.sqrt(R * p1 * (1 - p1))))
        else:
            best = max(best, 1.0 - (1.0 - abs(p1 - p0)) ** R)
    if exp.var_H > 1e-24:
        best = max(best, shifted(exp.mean_H, np.sqrt(exp.var_H / R), bad.mean_H, np.sqrt(bad.var_H / R)))
    return best


class Law:
    """The chain of one model from one start state: ``tabs`` one TableSet per state point (they differ in the
    chemical potentials only), ``temperature_factors`` c of T = c std(H) / k_B per state point (std over the grown
    set, state point 0), ``depth`` None = grow to closure."""

    def __init__(self, tabs, step, start, temperature_factors, depth=None):
        from oracle import oracle as orc

        self.tabs, self.step, self.depth = tabs, step, depth
        self.start = np.asarray(start, dtype=np.int8)
        self.N = len(self.start)
        uniq = {}
        self._ev = [uniq.setdefault(id(t), orc.OracleEvaluator(t)) for t in tabs]
        self._nat = [e.natural_parameters() for e in self._ev]
        t0 = tabs[0]
        self.subs = [(np.asarray(s["active_sites"], dtype=np.int64), [int(c) for c in s["codes"]]) for s in t0.sublattices]
        self.sub_probs = np.array(t0._keep["sub_probs"], dtype=np.float64)
        self.has_bias = bool(t0.struct.bias_type)
        self._cache = [dict() for _ in tabs]
        self._struct, self._laws = {}, {}
        H0 = self.structure(None)["H"][0]
        self.std_H = float(H0.std())
        self.temperatures = np.array([c * self.std_H / KB if self.std_H > 0 else 1000.0 * c for c in temperature_factors])
        self.G = len(tabs)

    # ---- energies: from scratch, per state -------------------------------------------------
    def _energy(self, g, key):
        hit = self._cache[g].get(key)
        if hit is None:
            occ = np.frombuffer(key, dtype=np.int8).astype(np.int32)
            ev = self._ev[g]
            hit = (float(ev.feature_vector(occ) @ self._nat[g]), float(ev.bias(occ)) if self.has_bias else 0.0)
            self._cache[g][key] = hit
        return hit

    def enthalpy(self, g, occ):
        return self._energy(g, np.asarray(occ, dtype=np.int8).tobytes())[0]

    # ---- proposals: (new state, probability, never accepted, log a-priori factor) ------------
    def _proposals(self, key, defect, scale=1.0, step=None):
        step = self.step if step is None else step
        if step == capi.STEP_TABLE_FLIP:
            return self._table_proposals(key)
        s = np.frombuffer(key, dtype=np.int8)
        probs = self.sub_probs
        if defect == "uniform-sublattice":
            probs = np.full(len(probs), 1.0 / len(probs))
        out = []
        for (sites, codes), ps in zip(self.subs, probs * scale):
            na = len(sites)
            w = np.full(na, 1.0 / na)
            if defect == "last-site-never":
                w[-1], w[0] = 0.0, 2.0 / na
            sub = s[sites]
            for a in range(na):
                if w[a] == 0.0:
                    continue
                i, cur = int(sites[a]), int(sub[a])
                if step == capi.STEP_FLIP:
                    new = codes if defect == "flip-any-code" else [c for c in codes if c != cur]
                    for c in new:
                        b = bytearray(key)
                        b[i] = c
                        out.append((bytes(b), ps * w[a] / len(new), False, 0.0))
                    continue
                partners = sites[sub != cur]
                if len(partners) == 0:  # the empty step
                    out.append((key, ps * w[a], False, 0.0))
                    continue
                q = ps * w[a] / (na - 1 if defect == "partner-any-site" else len(partners))
                for j in partners:
                    b = bytearray(key)
                    b[i], b[int(j)] = s[j], cur
                    out.append((bytes(b), q, False, 0.0))
                if defect == "partner-any-site" and len(partners) < na - 1:
                    out.append((key, ps * w[a] - q * len(partners), True, 0.0))
        return out

    def _table_proposals(self, key):
        """TableFlip.propose_step (mcusher.py:577-639): with probability swap_weight, or when no table direction is
        feasible at the current counts, a Swap; else a direction with probability proportional to its masked weight,
        the sites that lose a species a uniform subset of the sites holding it, the species they gain dealt out
        uniformly; a-priori factor of compute_log_priori_factor (:656-711) through composition.table_log_priori_factor."""
        import itertools

        from smol_amd import composition

        tab = self.tabs[0]
        table, weights = tab._keep["flip_table"], tab._keep["flip_weights"]
        sw = float(tab.struct.swap_weight)
        s = np.frombuffer(key, dtype=np.int8)
        n = np.array([int((s[sites] == c).sum()) for sites, codes in self.subs for c in codes])
        max_n = [len(sites) for sites, codes in self.subs for _ in codes]
        mw = weights * composition.flip_weights_mask(table, n, max_n)
        if not mw.sum() > 0:
            return self._proposals(key, None, 1.0, capi.STEP_SWAP)
        out = self._proposals(key, None, sw, capi.STEP_SWAP)
        for idx in np.flatnonzero(mw):
            u = table[idx // 2] * (1 if idx % 2 == 0 else -1)
            lp = composition.table_log_priori_factor(table, weights, sw, n, u, max_n)
            choices = [([], (1.0 - sw) * mw[idx] / mw.sum())]  # (flips so far, probability)
            base = 0
            for sites, codes in self.subs:
                us = u[base:base + len(codes)]
                base += len(codes)
                taken = [[]]  # every way to take the sites that lose their species, each equally likely
                for c, k in zip(codes, us):
                    if k < 0:
                        taken = [t + list(cmb) for t in taken for cmb in itertools.combinations(sites[s[sites] == c].tolist(), -k)]
                dealt = [([], t) for t in taken]  # (flips, sites left): every way to deal out the gained species
                for c, k in zip(codes, us):
                    if k > 0:
                        dealt = [(f + [(i, c) for i in cmb], [i for i in left if i not in cmb])
                                 for f, left in dealt for cmb in itertools.combinations(left, k)]
                assert all(not left for _, left in dealt)
                choices = [(f0 + f, q / len(dealt)) for f0, q in choices for f, _ in dealt]
            for flips, q in choices:
                b = bytearray(key)
                for i, c in flips:
                    b[i] = c
                out.append((bytes(b), q, False, lp))
        return out

    def structure(self, defect):
        """The grown set and the proposal matrix in coordinate form: dict(states, row, col, q, forced, H (G, S),
        B (S,))."""
        if defect not in _PROPOSAL_DEFECTS:
            defect = None
        if defect in self._struct:
            return self._struct[defect]
        start = self.start.tobytes()
        index, states = {start: 0}, [start]
        row, col, q, forced, lp = [], [], [], [], []
        frontier, d = [0], 0
        while frontier and (self.depth is None or d < self.depth):
            nxt = []
            for r in frontier:
                for new, prob, never, prior in self._proposals(states[r], defect):
                    c = index.get(new)
                    if c is None:
                        c = index[new] = len(states)
                        states.append(new)
                        nxt.append(c)
                    row.append(r), col.append(c), q.append(prob), forced.append(never), lp.append(prior)
            frontier, d = nxt, d + 1
        st = dict(states=np.frombuffer(b"".join(states), dtype=np.int8).reshape(len(states), self.N),
                  row=np.array(row), col=np.array(col), q=np.array(q), forced=np.array(forced, dtype=bool), lp=np.array(lp),
                  expanded=len(states) - len(frontier) if self.depth is not None else len(states))
        E = [[self._energy(g, k) for k in states] for g in range(len(self.tabs))]
        st["H"] = np.array([[e[0] for e in Eg] for Eg in E])
        st["B"] = np.array([e[1] for e in E[0]])
        np.testing.assert_allclose(np.bincount(st["row"], weights=st["q"])[: st["expanded"]], 1.0, rtol=0, atol=1e-12)
        self._struct[defect] = st
        return st

    defects = DEFECTS  # (the defects ``expected`` knows; tests/wl_law.py has its own)

    def _accept(self, st, g, beta, priori=True):
        a = np.minimum(1.0, np.exp(np.minimum(-beta * (st["H"][g][st["col"]] - st["H"][g][st["row"]])
                                              + (st["B"][st["col"]] - st["B"][st["row"]]) + (st["lp"] if priori else 0.0), 0.0)))
        a[st["forced"]] = 0.0
        return a

    def _acceptance(self, st, g, defect=None):
        """The accept probability of every proposal of ``st`` at state point g (the hook of tests/wl_law.py)."""
        beta = 1.0 / (KB * self.temperatures[g]) * (1.02 if defect == "beta-1.02" else 1.0)
        return self._accept(st, g, beta, priori=defect != "priori-dropped")

    def _log_weight(self, st, g):
        """log of the unnormalised stationary weight of every state."""
        return -1.0 / (KB * self.temperatures[g]) * st["H"][g] + st["B"]

    def matrices(self, g, defect=None):
        """(P_accepted (S, S) csr, rejected (S,)) of state point g."""
        st = self.structure(defect)
        a = self._acceptance(st, g, defect)
        S = len(st["states"])
        P = sparse.csr_matrix((st["q"] * a, (st["row"], st["col"])), shape=(S, S))
        rej = np.bincount(st["row"], weights=st["q"] * (1.0 - a), minlength=S)
        return st, P, rej

    def expected(self, g, n, defect=None):
        if defect not in self.defects:
            defect = None
        k = (g, n, defect)
        if k in self._laws:
            return self._laws[k]
        assert self.depth is None or n <= self.depth
        st, P, rej = self.matrices(g, defect)
        S = len(st["states"])
        if defect == "uniform-reused":
            assert n == 2
            v, pacc = self._reused(st, g), [np.nan, np.nan]
        else:
            W = n + 1 if n <= 2 else 1
            v = np.zeros((S, W))
            v[0, 0] = 1.0
            PT, pacc = P.T.tocsr(), []
            out = np.asarray(P.sum(axis=1)).ravel()
            for _ in range(n):
                pacc.append(float(v.sum(axis=1) @ out))
                moved = PT @ v
                nv = rej[:, None] * v
                if W > 1:
                    nv[:, 1:] += moved[:, :-1]
                else:
                    nv += moved
                v = nv
        assert abs(v.sum() - 1.0) < 1e-12, v.sum()
        e = Expected(st["states"], v, st["H"][g], pacc, n)
        self._laws[k] = e
        return e

    def _reused(self, st, g):
        """Two steps deciding on ONE uniform u: step k accepted when u < a_k."""
        a = self._acceptance(st, g)
        order = np.argsort(st["row"], kind="stable")
        lo = np.searchsorted(st["row"][order], np.arange(len(st["states"]) + 1))
        v = np.zeros((len(st["states"]), 3))
        first = order[lo[0]:lo[1]]
        for e1 in first:
            c1, q1, a1 = st["col"][e1], st["q"][e1], a[e1]
            e2 = order[lo[c1]:lo[c1 + 1]]  # step 1 accepted (u < a1): step 2 from c1
            np.add.at(v[:, 2], st["col"][e2], q1 * st["q"][e2] * np.minimum(a1, a[e2]))
            v[c1, 1] += float((q1 * st["q"][e2] * np.maximum(0.0, a1 - a[e2])).sum())
            np.add.at(v[:, 1], st["col"][first], q1 * st["q"][first] * np.maximum(0.0, a[first] - a1))
            v[0, 0] += float((q1 * st["q"][first] * (1.0 - np.maximum(a1, a[first]))).sum())
        return v

    def stationary_residual(self, g):
        """max |pi P - pi| of the Boltzmann weights (with the bias) over a set grown to closure."""
        assert self.depth is None
        st, P, rej = self.matrices(g)
        lw = self._log_weight(st, g)
        pi = np.exp(lw - lw.max())
        pi /= pi.sum()
        return float(np.max(np.abs(P.T @ pi + rej * pi - pi)))

    def applicable(self, n):
        d = ["last-site-never", "partner-any-site" if self.step == capi.STEP_SWAP else "flip-any-code"]
        if self.step == capi.STEP_TABLE_FLIP:  # (the proposal defects are variations of Flip and Swap)
            d = ["priori-dropped"]
        if self.std_H > 0:
            d.append("beta-1.02")
            if n == 2:
                d.append("uniform-reused")
        if len(self.subs) > 1 and np.ptp(self.sub_probs) > 0:
            d.append("uniform-sublattice")
        return d


# ---- the cases ---------------------------------------------------------------------------------------------
class Case:
    """name; build() -> dict(tab (the handle's tables), law, mu_rows or None); ns; the kernel family the device
    handle must report (substrings of kernel_info that must / must not be there) under ``env``."""

    def __init__(self, name, build, ns, want=("^lean",), wont=(), env=None, host=True, gpu=True, twin=None, groups=1,
                 r_cap=R_CAP):
        self.name, self._build, self.ns, self.want, self.wont = name, build, tuple(ns), tuple(want), tuple(wont)
        self.env, self.host, self.gpu, self.twin, self.groups, self.r_cap = dict(env or {}), host, gpu, twin, groups, r_cap

    @functools.cached_property
    def built(self):
        return CASES[self.twin].built if self.twin else self._build()

    @property
    def law(self):
        return self.built["law"]

    @property
    def seed_base(self):
        return 1_000_003 * (1 + list(CASES).index(self.twin or self.name))

    def family_ok(self, info):
        head = info.split(" env=")[0]
        return all((head.startswith(w[1:]) if w.startswith("^") else w in head) for w in self.want) and not any(
            w in head for w in self.wont)

    @functools.cached_property
    def R(self):
        return min(cap_respecting_R(self, choose_R(self)[0]), self.r_cap)

    def laws(self):
        return [(g, n) for g in range(self.law.G) for n in self.ns]


DISPATCH_SWITCHES = ("SMOLMC_NO_SOLO_ROWS", "SMOLMC_FORCE_GENERAL", "SMOLMC_FORCE_UNIVERSAL", "SMOLMC_NO_SOLO",
                     "SMOLMC_NO_LEAN_ALIASED", "SMOLMC_NO_LAZY_FEATURES", "SMOLMC_NO_OCC6")
TINY_NS, TINY_C = (1, 2, 3, 8, 64), (0.5, 1.0, 4.0)
CUTOFFS = {2: 6.0, 3: 5.0}


def _alternating(sc):
    """code = (index among the sites of its sublattice) mod (species of the site)"""
    n = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    occ = np.zeros(sc.num_sites, dtype=np.int32)
    for b in range(sc.model.prim.nb):
        sites = np.flatnonzero(sc.site_b == b)
        occ[sites] = np.arange(len(sites)) % n[sites]
    return occ


def _mu_table(sc, row):
    mu = np.zeros((sc.num_sites, len(row)))
    mu[:] = np.asarray(row)[None, :]
    return mu


def _fcc(dims, step, nspecies=2, mu=None, zero=False, start=None, factors=(1.0,), depth=2, mode=capi.FEATURES_INTERACTIONS):
    def build():
        model = synth.build_cluster_model(synth.fcc_prim(nspecies=nspecies), CUTOFFS)
        sc = synth.build_supercell(model, dims)
        coefs = synth.random_coefs(model, seed=11, scale=0.03)
        if zero:
            coefs = np.zeros_like(coefs)
        tab = capi.TableSet.from_synth(sc, coefs, feature_mode=mode, mu_table=None if mu is None else _mu_table(sc, mu))
        occ = _alternating(sc) if start is None else start(sc)
        law = Law([tab] * len(factors), step, occ, factors, depth=depth)
        return dict(tab=tab, law=law, mu_rows=None)
    return build


def _skewed(sc):
    occ = np.zeros(sc.num_sites, dtype=np.int32)
    occ[[5, 40]] = 1
    return occ


def _one_species(sc):
    return np.zeros(sc.num_sites, dtype=np.int32)


def _rocksalt_ewald(step):
    def build():
        model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 6.0, 3: 4.5})
        sc = synth.build_supercell(model, [2, 2, 4])
        mu = _mu_table(sc, [0.0, 0.05, -0.04]) if step == capi.STEP_FLIP else None
        tab = capi.TableSet.from_synth(sc, synth.random_coefs(model, seed=11, scale=0.03), ewald=ew.supercell_ewald(sc),
                                       ewald_coef=0.1, mu_table=mu)
        return dict(tab=tab, law=Law([tab], step, _alternating(sc), (1.0,), depth=2), mu_rows=None)
    return build


def _two_sublattices(mode=capi.FEATURES_INTERACTIONS):
    def build():
        model = synth.build_cluster_model(synth.rocksalt_prim(anion_charges=(-2.0, -1.0)), {2: 6.0, 3: 4.5})
        sc = synth.build_supercell(model, [3, 2, 2])
        tab = capi.TableSet.from_synth(sc, synth.random_coefs(model, seed=11, scale=0.03), feature_mode=mode,
                                       sublattice_probabilities=[0.3, 0.7])
        return dict(tab=tab, law=Law([tab], capi.STEP_SWAP, _alternating(sc), (1.0,), depth=2), mu_rows=None)
    return build


def _biased(kind):
    def build():
        model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 6.0, 3: 4.5})
        sc = synth.build_supercell(model, [2, 2, 2])
        ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=11, scale=0.03))
        names = ens.active_sublattices[0].species
        bias = (moca.FugacityBias(ens.sublattices, [{names[0]: 0.15, names[1]: 0.25, names[2]: 0.6}])
                if kind == "fugacity" else moca.SquareChargeBias(ens.sublattices, penalty=0.05))
        tab = ens.make_tables().set_bias(bias.bias_type, bias._table, bias.penalty)
        return dict(tab=tab, law=Law([tab], capi.STEP_FLIP, _alternating(sc), (1.0,), depth=2), mu_rows=None, keep=(ens, bias))
    return build


def _table_flip():
    """The charge-neutral table Li+ - 3 Mn3+ + 2 Ti4+ on the 8 cations of rocksalt 2x2x2, from 4 Li+ + 4 Mn3+."""
    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 6.0, 3: 4.5})
    sc = synth.build_supercell(model, [2, 2, 2])
    tab = capi.TableSet.from_synth(sc, synth.random_coefs(model, seed=11, scale=0.03), flip_table=np.array([[1, -3, 2]]),
                                   swap_weight=0.3)
    occ = np.zeros(sc.num_sites, dtype=np.int32)
    occ[: sc.size] = [0, 0, 1, 1, 0, 1, 1, 0]  # (from the alternating start every first step runs downhill: accepted with certainty)
    return dict(tab=tab, law=Law([tab], capi.STEP_TABLE_FLIP, occ, (1.0,), depth=2), mu_rows=None)


WALKER_MU = np.array([[[0.0, 0.02]], [[0.0, -0.05]], [[0.03, 0.0]], [[0.0, 0.08]]])  # (state point, sublattice, code)


def _walker_mu():
    model = synth.build_cluster_model(synth.fcc_prim(), CUTOFFS)
    sc = synth.build_supercell(model, [2, 2, 2])
    coefs = synth.random_coefs(model, seed=11, scale=0.03)
    tabs = [capi.TableSet.from_synth(sc, coefs, mu_table=_mu_table(sc, row[0])) for row in WALKER_MU]
    tab = capi.TableSet.from_synth(sc, coefs, mu_table=_mu_table(sc, [0.0, 0.0]))
    return dict(tab=tab, law=Law(tabs, capi.STEP_FLIP, _alternating(sc), (1.0, 1.0, 0.5, 4.0), depth=None), mu_rows=WALKER_MU)


def _sampler_ensemble():
    """The tiny binary swap cell as a moca.Ensemble: Sampler.from_ensemble(...).run(n, occ, thin_by=n)."""
    model = synth.build_cluster_model(synth.fcc_prim(), CUTOFFS)
    sc = synth.build_supercell(model, [2, 2, 2])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=11, scale=0.03))
    tab = ens.make_tables()
    return dict(tab=tab, law=Law([tab], capi.STEP_SWAP, _alternating(sc), (1.0,), depth=None), mu_rows=None, ensemble=ens)


SWAP, FLIP = capi.STEP_SWAP, capi.STEP_FLIP
MU2, MU3 = [0.0, 0.02], [0.0, 0.05, -0.04]
CASES = {c.name: c for c in [
    # tiny cells: the full law at n in {1, 2, 3, 8, 64}, three temperatures in one handle
    Case("fcc222-swap", _fcc([2, 2, 2], SWAP, factors=TINY_C, depth=None), TINY_NS, groups=3),
    Case("fcc222-flip", _fcc([2, 2, 2], FLIP, mu=MU2, factors=TINY_C, depth=None), TINY_NS, groups=3),
    Case("fcc222-ternary-flip", _fcc([2, 2, 2], FLIP, nspecies=3, mu=MU3, factors=TINY_C, depth=None), TINY_NS, groups=3),
    Case("fcc223-swap", _fcc([2, 2, 3], SWAP, factors=TINY_C, depth=None), TINY_NS, groups=3),
    # small cells: the one- and two-step law
    Case("fcc333-swap", _fcc([3, 3, 3], SWAP), (1, 2)),
    Case("fcc333-flip", _fcc([3, 3, 3], FLIP, mu=MU2), (1, 2)),
    Case("fcc444-swap", _fcc([4, 4, 4], SWAP, depth=1), (1,), want=("^lean ", "solo=1", " rows=")),
    Case("fcc444-flip", _fcc([4, 4, 4], FLIP, mu=MU2), (1, 2), want=("^lean ", "solo=1", " rows=")),
    Case("fcc333-swap-zero", _fcc([3, 3, 3], SWAP, zero=True), (1, 2)),
    Case("fcc333-flip-zero", _fcc([3, 3, 3], FLIP, mu=[0.0, 0.0], zero=True), (1, 2)),
    Case("fcc444-flip-zero", _fcc([4, 4, 4], FLIP, mu=[0.0, 0.0], zero=True), (1, 2)),
    Case("fcc444-swap-zero", _fcc([4, 4, 4], SWAP, zero=True, depth=1), (1,)),
    Case("fcc444-swap-skewed", _fcc([4, 4, 4], SWAP, start=_skewed), (1, 2)),
    Case("fcc444-swap-skewed-zero", _fcc([4, 4, 4], SWAP, start=_skewed, zero=True), (1, 2)),
    Case("fcc444-swap-one-species", _fcc([4, 4, 4], SWAP, start=_one_species), (1, 2)),
    Case("rocksalt224-ewald-flip", _rocksalt_ewald(FLIP), (1, 2), want=("^lean ",)),
    Case("rocksalt224-ewald-swap", _rocksalt_ewald(SWAP), (1, 2), want=("^lean ",)),
    Case("rocksalt322-two-sublattices", _two_sublattices(), (1, 2), want=("^lean-multi",)),
    Case("rocksalt222-fugacity", _biased("fugacity"), (1, 2), want=("^lean ",)),
    Case("rocksalt222-square-charge", _biased("square-charge"), (1, 2), want=("^lean ",)),
    Case("fcc222-walker-mu", _walker_mu, (1, 8), want=("^lean", "walker_mu=1"), groups=4),
    # the other kernel families on the fcc 4x4x4 one-step laws (the oracle is one: the CPU tier runs the default only)
    Case("fcc444-swap-plain-solo", None, (1,), want=("^lean ", "solo=1"), wont=(" rows=",), env={"SMOLMC_NO_SOLO_ROWS": "1"},
         host=False, twin="fcc444-swap"),
    Case("fcc444-flip-plain-solo", None, (1,), want=("^lean ", "solo=1"), wont=(" rows=",), env={"SMOLMC_NO_SOLO_ROWS": "1"},
         host=False, twin="fcc444-flip"),
    Case("fcc444-swap-general", None, (1,), want=("^general",), env={"SMOLMC_FORCE_GENERAL": "1"}, host=False, twin="fcc444-swap"),
    Case("fcc444-flip-general", None, (1,), want=("^general",), env={"SMOLMC_FORCE_GENERAL": "1"}, host=False, twin="fcc444-flip"),
    Case("fcc444-swap-universal", None, (1,), want=("^universal",), env={"SMOLMC_FORCE_UNIVERSAL": "1"}, host=False,
         twin="fcc444-swap"),
    Case("fcc444-flip-universal", None, (1,), want=("^universal",), env={"SMOLMC_FORCE_UNIVERSAL": "1"}, host=False,
         twin="fcc444-flip"),
    # ... and on the n = 8 law of the tiny cells, where beta x 1.02 shows: the accept path of mc_kernel and the universal kernel
    Case("fcc222-swap-general", None, (8,), want=("^general",), env={"SMOLMC_FORCE_GENERAL": "1"}, host=False, twin="fcc222-swap",
         groups=3),
    Case("fcc222-flip-general", None, (8,), want=("^general",), env={"SMOLMC_FORCE_GENERAL": "1"}, host=False, twin="fcc222-flip",
         groups=3),
    Case("fcc222-swap-universal", None, (8,), want=("^universal",), env={"SMOLMC_FORCE_UNIVERSAL": "1"}, host=False,
         twin="fcc222-swap", groups=3),
    Case("fcc222-flip-universal", None, (8,), want=("^universal",), env={"SMOLMC_FORCE_UNIVERSAL": "1"}, host=False,
         twin="fcc222-flip", groups=3),
    # several correlation functions per orbit: the KF kernels and the lazy-features path
    Case("fcc223-ternary-corr-kf", _fcc([2, 2, 3], SWAP, nspecies=3, mode=capi.FEATURES_CORRELATIONS), (1, 2),
         want=("^lean ", "kf=1")),
    Case("rocksalt322-corr-lazy", _two_sublattices(capi.FEATURES_CORRELATIONS), (1, 2), want=("^lean-multi", "lazy-features")),
    # TableFlip with its a-priori factor
    Case("rocksalt222-table-flip", _table_flip, (1, 2)),
    # moca.Sampler: the single sample row is the outcome
    Case("fcc222-swap-sampler", _sampler_ensemble, (8,), host=False, r_cap=1 << 16),
]}

HOST_RUNS = [(c.name, n) for c in CASES.values() if c.host for n in c.ns]
DEVICE_RUNS = [(c.name, n) for c in CASES.values() if c.gpu for n in c.ns]
N_STATISTICS = sum(3 * len(c.ns) * c.groups * (int(c.host) + int(c.gpu)) for c in CASES.values())
ALPHA = FAMILY_ALPHA / N_STATISTICS


@functools.lru_cache(maxsize=None)
def power_of(case, R):
    """{defect: best detection probability over the case's laws} at R walkers per state point."""
    law, out = case.law, {}
    for g, n in case.laws():
        exp = law.expected(g, n)
        for d in law.applicable(n):
            out[d] = max(out.get(d, 0.0), detection(exp, law.expected(g, n, d), R, ALPHA))
    return out


@functools.lru_cache(maxsize=None)
def choose_R(case):
    """(R, {defect: detection probability at R}, defects the case cannot detect at the cap)."""
    cap = power_of(case, R_CAP)
    drive = [d for d, p in cap.items() if p >= 0.99]
    R = R_MIN
    while R < R_CAP:
        p = power_of(case, R)
        if all(p[d] >= 0.99 for d in drive):
            break
        R *= 2
    return R, power_of(case, R), sorted(set(cap) - set(drive))


@functools.lru_cache(maxsize=None)
def pooled_mass(case, R):
    return max(case.law.expected(g, n).cells(R)[2] for g, n in case.laws())


def assert_pooling_cap(case, R):
    """At most 5 % of the mass in the pooled cell, on the law alone."""
    assert pooled_mass(case, R) <= 0.05, (case.name, R, pooled_mass(case, R))


def cap_respecting_R(case, R):
    """R doubled until the pooled cell of every law of the case holds at most 5 % of the mass."""
    while R < R_CAP and pooled_mass(case, R) > 0.05:
        R *= 2
    return R


# ---- running a case on an engine or the oracle ---------------------------------------------------------------------
def seeds_for(case, R, rerun=False):
    G = case.law.G
    return np.arange(G * R, dtype=np.uint64) + np.uint64(case.seed_base + (500_000_000 if rerun else 0))


def run_handle(case, handle, R, n, rerun=False):
    """One launch of ``n`` steps on a handle of G * R walkers (state point g owns walkers g R .. (g + 1) R - 1):
    returns (state dict, [Sample per state point])."""
    law = case.law
    occ = np.tile(law.start.astype(np.int32), (law.G * R, 1))
    handle.set_state(occ, seeds_for(case, R, rerun) + np.uint64(7919 * n), np.repeat(law.temperatures, R))
    if case.built["mu_rows"] is not None and hasattr(handle, "set_walker_mu"):
        handle.set_walker_mu(np.repeat(case.built["mu_rows"], R, axis=0))
    handle.run(n)
    st = handle.get_state()
    assert np.all(st["n_steps"] == n)
    return st, [Sample(st["occupancy"][g * R:(g + 1) * R], st["n_accepted"][g * R:(g + 1) * R], st["enthalpy"][g * R:(g + 1) * R])
                for g in range(law.G)]


FULL_R = ("fcc222-swap", 3)  # the (case, n) the CPU tier runs at the device's R: the device test compares histograms with it
_ORACLE_SAMPLES = {}


def host_R(case, n=None):
    """Walkers per state point of the CPU tier: 2^16, doubled until the pooled cell holds at most 5 % of the mass (never
    beyond the device's R); the device's R for FULL_R."""
    if (case.name, n) == FULL_R:
        return case.R
    return min(case.R, cap_respecting_R(case, HOST_R))


def oracle_samples(name, n, R=None, rerun=False):
    """[Sample per state point] of the CPU oracle's chains of the case after n steps (computed once per (case, n, R))."""
    from oracle import oracle as orc

    case = CASES[name]
    R = host_R(case, n) if R is None else R
    key = (name, n, R, rerun)
    if key not in _ORACLE_SAMPLES:
        law = case.law
        if case.built["mu_rows"] is None:
            ora = orc.OracleMC(case.built["tab"], capi.make_config(law.G * R, capi.KERNEL_METROPOLIS, law.step))
            _ORACLE_SAMPLES[key] = run_handle(case, ora, R, n, rerun)[1]
        else:  # per-walker chemical potentials: one oracle per state point, built with that point's table
            out = []
            seeds = seeds_for(case, R, rerun) + np.uint64(7919 * n)
            for g in range(law.G):
                ora = orc.OracleMC(law.tabs[g], capi.make_config(R, capi.KERNEL_METROPOLIS, law.step))
                ora.set_state(np.tile(law.start.astype(np.int32), (R, 1)), seeds[g * R:(g + 1) * R], law.temperatures[g])
                ora.run(n)
                st = ora.get_state()
                assert np.all(st["n_steps"] == n)
                out.append(Sample(st["occupancy"], st["n_accepted"], st["enthalpy"]))
            _ORACLE_SAMPLES[key] = out
    return _ORACLE_SAMPLES[key]


def report(case, g, n, res, where):
    line = (f"[chain law] {case.name} g={g} T={case.law.temperatures[g]:.0f}K n={n} on {where}: R={res['R']} df={res['df']} "
            f"p_chi2={res['p_chi2']:.3g}" + (f" z_acc={res['z_acc']:+.2f}" if "z_acc" in res else "")
            + f" z_H={res['z_H']:+.2f} zero={res['zero']} trace_err={res.get('trace_err', 0.0):.1e} alpha={ALPHA:.2e}")
    print(line)
    return line
