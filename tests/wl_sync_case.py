"""Shared helpers of the tests of the merge of a window's copies (parallel.WLWindows.synchronise on the host,
smolmc_wl_synchronise on the device): the 16-site case, windows and start states of tests/wl_windows_case.py, a config
with check period 0, hand-made arrays that take every branch of the definition, and a replica-exchange Wang-Landau
chain in plain Python (numpy_rewl) that runs the scheme without the engine and without the oracle."""

import functools

import numpy as np

from smol_amd import capi, parallel
from tests import wl_windows_case as wc

FLATNESS, DIVISOR = 0.8, 2.0


def windows(seed, copies=wc.COPIES):
    c = wc.case()
    wx = parallel.WLWindows(c["lo"], c["hi"], c["bin"], wc.N_WINDOWS, overlap=0.5, copies=copies, seed=seed)
    assert (wx.L, wx.Lw, wx.Ls) == (wc.N_BINS, 12, 6)
    return wx


def config(R, vmin, vmax, check_period=0, **kw):
    """The config of tests/wl_windows_case.py with check period 0: no estimator leaves its stage inside a launch."""
    return capi.make_config(R, capi.KERNEL_WANGLANDAU, capi.STEP_SWAP, min_enthalpy=float(vmin), max_enthalpy=float(vmax),
                            bin_size=wc.case()["bin"], check_period=check_period, flatness=FLATNESS, mod_update=DIVISOR, **kw)


# ---- hand-made arrays ------------------------------------------------------------------------------------------------
# Entropies whose sum depends on the order: 1 + 2^-53 + 2^-53 is 1 from the left (each addend is half an ulp of 1: ties
# to even) and 1 + 2^-52 from the right; with five values likewise.
_E = 2.0 ** -53
ORDER_3 = np.array([1.0, _E, _E])
ORDER_5 = np.array([1.0, _E, _E, _E, _E])


def ascending_mean(values):
    a = np.float64(values[0])
    for v in values[1:]:
        a = a + np.float64(v)
    return a / np.float64(len(values))


def planted(R, copies, L=12, at_threshold=True, third="single"):
    """(entropy (R, L), histogram (R, L) int64, mod_factor (R,), expected status (R / copies,)) with these groups, in
    turn: 0 merges, its bin 3 visited by copy 0 only and its bin 5 holding the order-dependent entropies; 1 has in
    its last copy one visited bin exactly at flatness * mean (`at_threshold`: not flat under the strict >; else that count
    is one higher and the group merges); 2 has a copy with one visited bin (`third` = "single", n < 2: not flat) or
    flat copies with unequal factors (`third` = "factors": status 2); from group 3 on alternately unequal factors and
    merging groups with random entropies."""
    G = R // copies
    assert G * copies == R and G >= 3 and L >= 8
    rng = np.random.default_rng(1000 * R + copies)
    S = np.zeros((R, L))
    hist = np.zeros((R, L), dtype=np.int64)
    m = np.full(R, 2.0 ** -3)
    want = np.zeros(G, dtype=np.int32)
    order = {3: ORDER_3, 5: ORDER_5}.get(copies)
    for g in range(G):
        e = np.arange(g * copies, (g + 1) * copies)
        # every copy visited the bins 0, 1, 2, 4, 5, 6 with a flat histogram around 1000 (all > 0.8 x mean)
        vis = np.array([0, 1, 2, 4, 5, 6])
        S[np.ix_(e, vis)] = rng.uniform(0.5, 40.0, size=(copies, len(vis)))
        hist[np.ix_(e, vis)] = rng.integers(950, 1050, size=(copies, len(vis)))
        hist[np.ix_(e, [3, 7])] = rng.integers(0, 5, size=(copies, 2))  # (counts in unvisited bins: not part of V)
        want[g] = 1
        if g == 0:
            S[e[0], 3], hist[e[0], 3] = 7.25, 1000  # visited by copy 0 only: the merged value is 7.25 / copies
            if order is not None:
                S[e, 5] = order
        elif g == 1:
            # last copy: two visited bins with the counts (1500, x).  0.8 * (1500 + x) / 2 == x at x = 1000: the mean is
            # 1250.0 and 0.8 * 1250.0 rounds to 1000.0 exactly (0.8 itself is not exact in binary: asserted below)
            S[e[-1]], hist[e[-1]] = 0.0, 0
            S[e[-1], [1, 6]] = [3.5, 4.5]
            hist[e[-1], [1, 6]] = [1500, 1000 if at_threshold else 1001]
            want[g] = 0 if at_threshold else 1
        elif g == 2 and third == "single":
            S[e[copies // 2]] = 0.0
            S[e[copies // 2], 4] = 2.0  # one visited bin
            want[g] = 0
        elif g == 2 or g % 2 == 1:
            m[e[-1]] = np.nextafter(m[e[-1]], 1.0)  # one ulp apart: not bitwise equal
            want[g] = 2
    assert np.float64(FLATNESS) * (np.float64(2500) / np.float64(2)) == 1000.0
    return S, hist, m, want


# ---- the scheme in plain Python --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tables():
    """(index of every bit mask, per window: in-window flags and bins of the 12870 states as lists)."""
    c = wc.case()
    wx = windows(0)
    masks = (c["states"].astype(np.int64) << np.arange(c["N"])).sum(axis=1)
    index = {int(mk): i for i, mk in enumerate(masks)}
    inside, bins = [], []
    for k in range(wx.n_windows):
        inside.append(((c["E"] >= wx.window_min[k]) & (c["E"] < wx.window_max[k])).tolist())
        bins.append(wx.bins(c["E"], wx.window_min[k]).tolist())
    return index, inside, bins


def numpy_rewl(seed, copies, synchronise, rounds=wc.ROUNDS, steps=wc.STEPS):
    """Replica-exchange Wang-Landau on the enumerated 16-site case without engine or oracle: every state a bit mask, the
    energies a table over the 12870 states, proposals swaps of one occupied and one empty site, a proposal that leaves
    the window rejected and counted in the current bin; `rounds` rounds of `steps` steps per walker, after each round
    one exchange decided by wx.decide with the identity map (accepted pairs swap their configurations) and then
    either one wx.synchronise (`synchronise`) or every estimator's own flatness check (the scheme of the sampling
    kernels at check period `steps`).  Returns dict(wx, entropy, mod_factor, merges, visited, rms (per copy), joined)."""
    c = wc.case()
    N = c["N"]
    wx = windows(seed, copies)
    index, inside, bins = _tables()
    E = c["E"]
    rng = np.random.default_rng(seed)
    occ0 = wc.start_occupancies(wx, seed)
    state = [int((occ0[e].astype(np.int64) << np.arange(N)).sum()) for e in range(wx.R)]
    S = np.zeros((wx.R, wx.Lw))
    hist = np.zeros((wx.R, wx.Lw), dtype=np.int64)
    m = np.ones(wx.R)
    merges = np.zeros(wx.n_windows, dtype=np.int64)
    identity = np.arange(wx.R)
    half = N // 2
    for rnd in range(rounds):
        for e in range(wx.R):
            k = int(wx.window_of[e])
            ins, bn = inside[k], bins[k]
            s_row, h_row, mf = S[e].tolist(), hist[e].tolist(), float(m[e])
            mask = state[e]
            cur = index[mask]
            jb = bn[cur]
            io, ie = rng.integers(0, half, steps).tolist(), rng.integers(0, half, steps).tolist()
            lu = np.log(rng.random(steps)).tolist()
            on = [i for i in range(N) if mask >> i & 1]
            off = [i for i in range(N) if not mask >> i & 1]
            for t in range(steps):
                a, b = on[io[t]], off[ie[t]]
                new = index[mask ^ (1 << a) ^ (1 << b)]
                if ins[new]:
                    jn = bn[new]
                    d = s_row[jb] - s_row[jn]
                    if d >= 0.0 or lu[t] < d:
                        mask ^= (1 << a) ^ (1 << b)
                        on[io[t]], off[ie[t]] = b, a
                        cur, jb = new, jn
                s_row[jb] += mf
                h_row[jb] += 1
            S[e], hist[e], state[e] = s_row, h_row, mask
        H = np.array([E[index[mk]] for mk in state])
        res = wx.decide(H, S, identity, wx.move_of(wx.calls), wx.calls)
        wx.calls += 1
        for (s, t), acc in zip(res["pairs"], res["accept"]):
            if acc:
                state[s], state[t] = state[t], state[s]
        if synchronise:
            out = wx.synchronise(S, hist, m, flatness=FLATNESS, divisor=DIVISOR)
            S, hist, m = out["entropy"], out["histogram"], out["mod_factor"]
            merges += out["status"] == 1
        else:
            for e in range(wx.R):
                if wx.flat(S[e], hist[e], FLATNESS):
                    hist[e] = 0
                    m[e] = m[e] / DIVISOR
    ln_g, per_copy, visited = wx.join(S)
    rms = [wc.rms_vs_exact(per_copy[i], per_copy[i] != 0) for i in range(copies)]
    return dict(wx=wx, entropy=S, mod_factor=m, merges=merges, visited=visited, rms=rms, joined=wc.rms_vs_exact(ln_g, visited))


if __name__ == "__main__":  # the table in tests/test_wl_sync_host.py
    import sys

    for copies in (2, 4):
        for seed in (5, 6, 7):
            for sync in (False, True):
                r = numpy_rewl(seed, copies, sync)
                mf = r["mod_factor"]
                print(f"copies {copies} seed {seed} {'merged     ' if sync else 'independent'}: rms per copy "
                      f"{min(r['rms']):.3f} - {max(r['rms']):.3f}, joined {r['joined']:.3f}, factors {mf.min():.1e} .. {mf.max():.1e}, "
                      f"merges {r['merges'].tolist()}, acceptance {r['wx'].acceptance:.2f}, all visited "
                      f"{bool((r['visited'] >= wc.case()['occupied']).all())}", flush=True)
    sys.exit(0)
