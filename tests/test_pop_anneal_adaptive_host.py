"""The adaptive schedule of population annealing on the host: the integer overlap rule and the search of the next
temperature (parallel.PopulationAnnealing.overlap_ok, next_temperature), and the whole scheme on the CPU oracle against
exact enumeration.  The device side is tests/test_gpu_pop_anneal_adaptive.py."""

import numpy as np
import pytest

from smol_amd import parallel
from tests import pop_anneal_adaptive_case as ac
from tests import pop_anneal_case as pc

PA = parallel.PopulationAnnealing
kB = parallel.kB
T85 = PA.target_word(0.85)


def enthalpies(seed, n, scale=0.05):
    return np.random.default_rng(seed).normal(scale=scale, size=n)


def float_overlap(H, db):
    """sum_j min(1 / n, w_j / W) in float64 from the untruncated weights."""
    H = np.asarray(H, dtype=np.float64)
    w = np.exp(-(db * (H - (H.min() if db > 0 else H.max()))))
    return float(np.minimum(1.0 / len(H), w / w.sum()).sum())


# ---- the rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 256, 1000])
def test_overlap_ok_against_a_float_evaluation(n):
    """Away from the threshold (the truncation of q_j moves the overlap by at most n 2^-40 / min weight, far below
    the 1e-6 kept clear here) the integer rule decides as the float overlap does; both signs of db."""
    decided = [0, 0]
    for seed in range(12):
        H = enthalpies(seed, n)
        for db in (3.0, -3.0, 20.0, -20.0, 80.0, 0.4):
            f = float_overlap(H, db)
            q, _, _ = PA.weights_of_step(H, db)
            assert abs(PA.overlap(q) - f) < 1e-9
            for target in (0.3, 0.5, 0.7, 0.85, 0.95, 0.999):
                if abs(f - target) < 1e-6:
                    continue
                ok = PA.overlap_ok(H, db, PA.target_word(target))
                assert ok == (f > target), (seed, db, target, f)
                decided[int(ok)] += 1
    if n > 1:
        assert min(decided) >= 20  # (both answers occur)


def test_s_is_cq_plus_nu_and_the_margin():
    for seed, n in enumerate((1, 3, 64, 300)):
        H = enthalpies(seed, n)
        for db in (5.0, -12.0, 40.0):
            q, Q, _ = PA.weights_of_step(H, db)
            qs = [int(x) for x in q]
            n_, Q_, c, U = PA.overlap_terms(q)
            assert (n_, Q_) == (n, Q) and Q == sum(qs)
            assert c == sum(1 for x in qs if n * x >= Q) and U == sum(x for x in qs if n * x < Q)
            s = sum(min(Q, n * x) for x in qs)
            assert s == c * Q + n * U
            assert PA.overlap(q) == s / (n * Q)
            ok, margin = PA.overlap_ok(H, db, T85, margin=True)
            assert ok == (s * 2 ** 32 >= T85 * n * Q) and margin == abs(s * 2 ** 32 - T85 * n * Q) >> 32


def test_no_step_is_overlap_one():
    H = enthalpies(3, 37)
    q, Q, href = PA.weights_of_step(H, 0.0)
    assert np.all(q == 2 ** 40) and href == H.max() and PA.overlap(q) == 1.0
    assert PA.overlap_ok(H, 0.0, 2 ** 32 - 1) and PA.overlap_ok(H, -0.0, 1)
    assert PA.overlap_ok([0.25], 1e6, 2 ** 32 - 1)  # one walker: every step is ok
    for bad in (0, 2 ** 32, -1):
        with pytest.raises(ValueError, match="0 < t < 2\\^32"):
            PA.overlap_ok(H, 1.0, bad)
    for bad in (0.0, 1.0, 1e-12):
        with pytest.raises(ValueError, match="target overlap"):
            PA.target_word(bad)
    assert PA.target_word(0.5) == 2 ** 31


# ---- the search -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [400.0, -400.0, 25.0])
@pytest.mark.parametrize("n_iter", [1, 5, 16, 60])
def test_bisection_keeps_ok_lo_and_not_ok_hi(D, n_iter):
    H = enthalpies(8, 200)
    db, reached, forced, margin, lo, hi = PA.search_step(H, D, T85, n_iter)
    assert not reached and not PA.overlap_ok(H, D, T85)
    assert PA.overlap_ok(H, lo, T85) and not PA.overlap_ok(H, hi, T85)
    assert 0.0 <= abs(lo) < abs(hi) <= abs(D) and lo * D >= 0.0 and hi * D > 0.0
    assert forced == (lo == 0.0) and db == (hi if forced else lo)
    if n_iter >= 16:
        assert not forced and abs(hi - lo) <= abs(D) * 2.0 ** -min(n_iter, 50)
    if n_iter == 60:  # the search ran out of doubles before it ran out of halvings: lo and hi are neighbours
        assert lo / D > 2.0 ** -7 and np.nextafter(lo, hi) == hi
    # the steps are the midpoints, each rounded once: replay them
    a, b, margins = np.float64(0.0), np.float64(D), [PA.overlap_ok(H, D, T85, margin=True)[1]]
    for _ in range(n_iter):
        mid = np.float64(0.5) * (a + b)
        if mid == a or mid == b:
            break
        ok, m = PA.overlap_ok(H, mid, T85, margin=True)
        margins.append(m)
        a, b = (mid, b) if ok else (a, mid)
    assert (a, b) == (lo, hi) and margin == min(margins)


def test_reached_forced_and_heating():
    H = enthalpies(4, 2 * 128).reshape(2, 128)
    T = 1000.0
    beta = 1.0 / (kB * T)
    # a limit 1 % away: the whole step is ok, the temperature is the limit itself
    t_new, reached, forced, _ = PA.next_temperature(H, beta, 990.0, T85, 16)
    assert (t_new, reached, forced) == (990.0, True, False)
    # the limit itself: db = 0
    assert PA.next_temperature(H, beta, T, T85, 16)[:3] == (T, True, False)
    # far away, one halving: the midpoint is still too far, lo stays 0 and the step is hi
    D = 1.0 / (kB * 1.0) - beta
    t_new, reached, forced, _ = PA.next_temperature(H, beta, 1.0, T85, 1)
    assert not reached and forced
    assert t_new == 1.0 / (kB * (beta + 0.5 * D)) and 1.0 < t_new < 2.1
    # the same search with 16 halvings is not forced and keeps the target
    t16, reached, forced, _ = PA.next_temperature(H, beta, 1.0, T85, 16)
    assert not reached and not forced and t_new < t16 < T
    db16 = 1.0 / (kB * t16) - beta
    for p in range(2):
        assert PA.overlap(PA.weights_of_step(H[p], db16)[0]) >= 0.85 - 1e-6
    # heating: T_limit > T, db < 0, H_ref is the largest enthalpy
    th, reached, forced, _ = PA.next_temperature(H, beta, 1e6, T85, 16)
    assert not reached and not forced and T < th < 1e6
    dbh = 1.0 / (kB * th) - beta
    assert dbh < 0 and PA.weights_of_step(H[0], dbh)[2] == H[0].max()
    assert PA.next_temperature(H, beta, 1010.0, T85, 16)[:3] == (1010.0, True, False)
    for bad in (0.0, -5.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="positive and finite"):
            PA.next_temperature(H, beta, bad, T85, 16)
    for bad in (0, 61):
        with pytest.raises(ValueError, match="n_iter"):
            PA.next_temperature(H, beta, 500.0, T85, bad)


def test_smallest_step_wins_across_populations():
    rng = np.random.default_rng(6)
    H = np.stack([rng.normal(scale=s, size=96) for s in (0.02, 0.08, 0.04)])  # the widest population moves least
    beta = 1.0 / (kB * 800.0)
    for T_limit in (80.0, 8000.0):
        D = np.float64(1.0) / (np.float64(kB) * np.float64(T_limit)) - np.float64(beta)
        steps = [PA.search_step(H[p], D, T85, 16) for p in range(3)]
        dbs = [abs(s[0]) for s in steps]
        assert dbs[1] < dbs[2] < dbs[0]
        t_new, reached, forced, margin = PA.next_temperature(H, beta, T_limit, T85, 16)
        assert t_new == 1.0 / (kB * (beta + steps[1][0])) and not reached and not forced
        assert margin == min(s[3] for s in steps)
        # ... whatever the order of the populations; alone, the narrow one goes further
        assert PA.next_temperature(H[::-1], beta, T_limit, T85, 16)[0] == t_new
        alone = PA.next_temperature(H[0], beta, T_limit, T85, 16)[0]
        assert abs(alone - 800.0) > abs(t_new - 800.0)
    # reached needs every population: one that cannot reach the limit keeps all from it
    D = np.float64(1.0) / (np.float64(kB) * np.float64(80.0)) - np.float64(beta)
    between = 0.5 * (PA.search_step(H[1], D, T85, 16)[0] + PA.search_step(H[0], D, T85, 16)[0])
    T_limit = 1.0 / (kB * (beta + between))
    D = np.float64(1.0) / (np.float64(kB) * np.float64(T_limit)) - np.float64(beta)
    assert PA.search_step(H[0], D, T85, 16)[1] and not PA.search_step(H[1], D, T85, 16)[1]
    t_new, reached, _, _ = PA.next_temperature(H, beta, T_limit, T85, 16)
    assert not reached and T_limit < t_new < 800.0
    assert PA.next_temperature(H[0], beta, T_limit, T85, 16)[:2] == (T_limit, True)
    # forced is the flag of the population whose step is taken
    t_new, reached, forced, _ = PA.next_temperature(H, beta, 1.0, T85, 2)
    steps = [PA.search_step(H[p], 1.0 / (kB * 1.0) - beta, T85, 2) for p in range(3)]
    k = int(np.argmin([abs(s[0]) for s in steps]))
    assert forced == steps[k][2] and all(s[2] for s in steps)


def test_temperature_and_beta_round_as_specified():
    H = enthalpies(9, 150).reshape(1, -1)
    T = np.float64(1234.5)
    beta = np.float64(1.0) / (np.float64(kB) * T)
    t_new, reached, _, _ = PA.next_temperature(H, beta, 77.0, T85, 16)
    D = np.float64(1.0) / (np.float64(kB) * np.float64(77.0)) - beta
    db = PA.search_step(H[0], D, T85, 16)[0]
    assert not reached
    prod = np.float64(kB) * (beta + db)  # the sum, the product, the quotient: three roundings
    assert t_new == float(np.float64(1.0) / prod)
    # db is a dyadic fraction of D: 16 halvings leave k / 2^16 of it
    k = db / D * 2 ** 16
    assert abs(k - round(k)) < 1e-6 and 0 < round(k) < 2 ** 16
    # the schedule keeps betas == 1 / (kB T) of the recorded temperatures
    pa = PA.adaptive(T, 77.0, 0.85, n_iter=16)
    assert pa.choose(H.reshape(-1)) == t_new and pa.temperatures[-1] == t_new
    assert pa.betas[-1] == 1.0 / (kB * t_new) and pa.betas[0] == beta
    res = pa.step(H.reshape(-1), 0)
    q, Q, href = PA.weights(H[0], beta, 1.0 / (kB * t_new))
    assert np.array_equal(res["q"], q) and res["log_q"][0] == np.log(Q / (150 * 2.0 ** 40)) - (pa.betas[1] - pa.betas[0]) * href


def test_adaptive_schedule_bookkeeping():
    pa = PA.adaptive(900.0, 300.0, 0.85, populations=2, seed=3, n_iter=8, max_steps=3)
    assert pa.adaptive_schedule and not pa.done and pa.n_steps == 0 and list(pa.temperatures) == [900.0]
    assert pa.overlap_target == T85 and pa.free_energy().shape == (0, 2)
    H = enthalpies(2, 64)
    for k in range(3):
        t_new = pa.choose(H)
        assert pa.n_steps == k + 1 and not pa.done and 300.0 < t_new < pa.temperatures[k]
        res = pa.step(H, k)
        assert pa.calls == k + 1 and pa.log_q.shape == (k + 1, 2) and pa.free_energy().shape == (k + 1, 2)
        np.testing.assert_array_equal(pa.betas, 1.0 / (kB * pa.temperatures))
        H = H[res["parent"]]
    with pytest.raises(RuntimeError, match="max_steps = 3"):
        pa.choose(H)
    pa = PA.adaptive(900.0, 895.0, 0.85, populations=2)
    assert pa.choose(H) == 895.0 and not pa.done  # chosen, not yet taken
    pa.step(H, 0)
    assert pa.done and list(pa.temperatures) == [900.0, 895.0] and pa.forced == [False]
    with pytest.raises(ValueError, match="reached its end"):
        pa.choose(H)
    # a fixed schedule is what it was
    fixed = PA([900.0, 600.0, 400.0], populations=2)
    assert not fixed.adaptive_schedule and fixed.n_steps == 2 and not fixed.done
    with pytest.raises(ValueError, match="fixed schedule"):
        fixed.append(300.0, True)
    fixed.step(H, 0)
    fixed.step(H, 1)
    assert fixed.done
    for kwargs in (dict(overlap=0.0), dict(overlap=1.0), dict(n_iter=0), dict(n_iter=61), dict(t_end=0.0)):
        args = dict(t_start=900.0, t_end=300.0, overlap=0.85)
        args.update(kwargs)
        with pytest.raises(ValueError):
            PA.adaptive(**args)


# ---- the scheme on the CPU oracle against exact enumeration ---------------------------------------------------------
@pytest.mark.parametrize("seed", pc.SEEDS)
def test_oracle_adaptive_annealing_against_enumeration(seed):
    pa, dl, de, history = ac.oracle_errors(seed)
    print(f"seed {seed}: {pa.n_steps} steps", np.round(pa.temperatures, 1))
    print("   sum ln Q - exact", np.round(dl, 4), " final mean enthalpy - exact", np.round(de, 5))
    print("   smallest overlap per step", np.round(pa.overlaps.min(axis=1), 4))
    assert pa.done and pa.temperatures[0] == ac.T_START and pa.temperatures[-1] == ac.T_END
    assert np.all(np.diff(pa.temperatures) < 0)
    assert pa.n_steps < ac.FIXED_STEPS  # the claim: fewer steps than the fixed ladder's 15
    assert len(history) == pa.n_steps == len(pa.log_q) == len(pa.overlaps) and not any(pa.forced)
    # every step but the last keeps the target, and wastes little of it (16 halvings)
    assert np.all(pa.overlaps >= ac.OVERLAP - 1e-6)
    assert np.all(pa.overlaps[:-1].min(axis=1) < ac.OVERLAP + 0.01)
    assert np.all(np.abs(dl) <= ac.LNZ_BOUND), dl
    assert np.all(np.abs(de) <= ac.EMEAN_BOUND), de
