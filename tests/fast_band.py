"""Adversarial constructions for the float32 accept pre-test of the lean kernels and the float32 bin pre-test of the
lean Wang-Landau kernel (tests/test_fast_band_host.py holds them against the CPU oracle alone,
tests/test_gpu_fast_band.py runs them on the device, tools/fast_band_margin.py measures the margin of the band).

The kernels decide a step on a float32 wave sum S of the energy change: accept on S < thr - eps, reject on
S > thr + eps, the float64 rule in between, with eps = fast_eps + 1e-6 |thr| (mc_lean.h, mc_lean_multi.h); mc_wl.h
takes the bin of the proposed enthalpy from a float32 position carried with the same bound per accepted step.  A
band that is too narrow turns a decision only when the threshold lands within the float32 error of the exact value,
which a random chain does about once in 1e7 steps.  Here the threshold is PLACED there on every tested step.

Common definitions
  * exact dH of a proposal: OracleEvaluator.feature_vector_change(occ, flips) @ natural_parameters() in float64
    (cross-checked on 16 walkers per construction against feature_vector(after) - feature_vector(before));
    A = |feature change| @ |natural parameters| + |dH| is the scale of the proposal;
  * the hair: delta = +- 2^-34 A, the sign alternating over walkers (random in construction C): 6e-11 relative, far
    above the 1e-15 by which two float64 summation orders differ, far below the 6e-8 of one float32 rounding.  The
    threshold is put at dH + delta, so the exact rule accepts when delta > 0 and rejects when delta < 0, and a
    float32 pre-test decides such a step wrongly exactly when its error exceeds its band;
  * a walker is adversarial when its tested proposal is uphill, dH > 2^-20 A (so a positive threshold exists), and A
    stands above the noise floor of its state (Pricer.floor: a mirror-symmetric swap has dH = 0 and A ~ 1e-16); the
    others are controls at an ordinary temperature.  Cap: at least half the walkers of every construction are
    adversarial (asserted on the oracle by the CPU tier);
  * the reference is always the CPU oracle (for bins: exact float64 floor division), never the device at another
    band scale.

Metropolis constructions
  A  one native step at every phase of the random batches: R = 4096 random starts at several compositions, walker r
     at n_steps = r mod 128 (set_counters), its temperature T = (dH + delta) / (-kB ln u) from the proposal and the
     uniform the oracle names for its next step.  All 64 lanes of the threshold batch occur among the adversarial
     walkers.
  B  one native step inside a launch: R = 2048 starts quenched on the oracle (1e-3 K, 50 sweeps); while the state
     stays in its minimum the proposals and uniforms of the next 96 steps are known; tau_j = dH_j / (-ln u_j) over
     the uphill prefix, the tested step k = argmin tau_j, kB T = tau_k with the hair on dH_k; every earlier step is
     rejected (tau_j > 1.001 tau_k asserted, else the walker is a control).  >= 48 of the 64 lanes are covered.
  C  replay, every step adversarial: R = 1024, n = 64, one temperature per walker; the host walks the chain in
     float64 with its own generator, u = exp(-beta (dH + delta)) for an uphill proposal, 0.5 otherwise.  (A step
     whose exponent leaves [1e-3, 600] is a control too: there exp and log do not round-trip to 2^-34.)

Teeth: every case repeats A (and the one-step probes of C: walker r replays step r mod n of its chain alone, from the
state the host's chain had before it) at SMOLMC_FAST_EPS_SCALE = 1, 1/2, ... 2^-20 with a fresh handle per scale; no
decision may be wrong at 1, some scale must show one (else the construction never reaches the float32 error), and the
largest such scale is the measured margin of the case (tools/fast_band_margin.py, profiles/fast_band_margin.jsonl).

Wang-Landau: the window constructions are described above WL_KS below; their scale sweep is a measurement, since the
tolerance of that pre-test does not scale with the band.

Not covered: the Ewald, biased and Wang-Landau-multi variants never take the pre-test; the TableFlip kernels are
exact; the 1e-6 |thr| term of the band is exercised only as far as the temperatures of the cases reach (thr = dH +
delta here, so the term is 1e-6 of the tested dH)."""

import functools

import numpy as np

from smol_amd import capi, moca, synth
from tests import chain_law as cl
from tests.cases import load_case, tables_for

KB = moca.kB
HAIR = 2.0 ** -34
UPHILL = 2.0 ** -20
NOISE_FLOOR = 2.0 ** -16
CONTROL_T = 1000.0
RTOL, ATOL = 1e-10, 1e-9  # the parity suite's tolerance on the enthalpy
SCALES = tuple(2.0 ** -k for k in range(21))  # the band-scale sweep: 1, 1/2, ... 2^-20
SWAP, FLIP = capi.STEP_SWAP, capi.STEP_FLIP
INT, CORR = capi.FEATURES_INTERACTIONS, capi.FEATURES_CORRELATIONS
R_A, R_B, N_B, R_C, N_C = 4096, 2048, 96, 1024, 64


def _nspecies(sc):
    return np.array([sc.model.prim.nspecies[b] for b in sc.site_b])


def _fcc(dims, step, nspecies=2, mu=None, mode=INT):
    """The small fcc cells of tests/chain_law.py (same cutoffs, coefficients and chemical potentials)."""
    def build():
        model = synth.build_cluster_model(synth.fcc_prim(nspecies=nspecies), cl.CUTOFFS)
        sc = synth.build_supercell(model, dims)
        coefs = synth.random_coefs(model, seed=11, scale=0.03)
        tab = capi.TableSet.from_synth(sc, coefs, feature_mode=mode, mu_table=None if mu is None else cl._mu_table(sc, mu))
        return dict(tab=tab, nsp=_nspecies(sc))
    return build


def _triplets(step):
    """fcc_prim666_triplets of the parity suite, with its chemical potentials for the flip."""
    def build():
        c = load_case("fcc_prim666_triplets")
        mu = None
        if step == FLIP:
            mu = np.zeros((c["sc"].num_sites, 2))
            mu[:] = np.linspace(-0.3, 0.4, 2)[None, :]
        return dict(tab=tables_for("fcc_prim666_triplets", INT, mu_table=mu), nsp=_nspecies(c["sc"]))
    return build


def _two_sublattices(mode):
    def build():
        model = synth.build_cluster_model(synth.rocksalt_prim(anion_charges=(-2.0, -1.0)), {2: 6.0, 3: 4.5})
        sc = synth.build_supercell(model, [3, 2, 2])
        tab = capi.TableSet.from_synth(sc, synth.random_coefs(model, seed=11, scale=0.03), feature_mode=mode,
                                       sublattice_probabilities=[0.3, 0.7])
        return dict(tab=tab, nsp=_nspecies(sc))
    return build


WALKER_MU_SMALL, WALKER_MU_FACTOR = np.array([0.0, 0.002]), 100.0


def _walker_mu():
    """fcc 2x2x2 semigrand flips: the handle is created with small chemical potentials, one walker in eight then gets
    rows 100 times as large through set_walker_mu (the stale-bound case engine.hip names)."""
    model = synth.build_cluster_model(synth.fcc_prim(), cl.CUTOFFS)
    sc = synth.build_supercell(model, [2, 2, 2])
    coefs = synth.random_coefs(model, seed=11, scale=0.03)
    tab = capi.TableSet.from_synth(sc, coefs, mu_table=cl._mu_table(sc, WALKER_MU_SMALL))
    big = capi.TableSet.from_synth(sc, coefs, mu_table=cl._mu_table(sc, WALKER_MU_SMALL * WALKER_MU_FACTOR))
    return dict(tab=tab, big=big, nsp=_nspecies(sc))


class Case:
    """name; build() -> dict(tab, nsp[, big]); step; the kernel family the device handle must report under ``env``
    (substrings of kernel_info that must / must not be there, '^' = at the start); the constructions it runs."""

    def __init__(self, name, build, step, want, wont=(), env=None, constructions="A", twin=None):
        self.name, self._build, self.step, self.want, self.wont = name, build, step, tuple(want), tuple(wont)
        self.env, self.constructions, self.twin = dict(env or {}), constructions, twin

    @functools.cached_property
    def built(self):
        return CASES[self.twin].built if self.twin else self._build()

    @property
    def tab(self):
        return self.built["tab"]

    @property
    def seed_base(self):
        return 7_000_003 * (1 + list(CASES).index(self.twin or self.name))

    def family_ok(self, info):
        head = info.split(" env=")[0]
        return all((head.startswith(w[1:]) if w.startswith("^") else w in head) for w in self.want) and not any(
            w in head for w in self.wont)


ROWS = ("^lean ", "solo=1", " rows=")
NO_ROWS, NO_SOLO = {"SMOLMC_NO_SOLO_ROWS": "1"}, {"SMOLMC_NO_SOLO": "1"}
CASES = {c.name: c for c in [
    Case("fcc444-swap", _fcc([4, 4, 4], SWAP), SWAP, ROWS, constructions="AB"),
    Case("fcc444-flip", _fcc([4, 4, 4], FLIP, mu=cl.MU2), FLIP, ROWS, constructions="AB"),
    Case("fcc444-swap-plain-solo", None, SWAP, ("^lean ", "solo=1"), wont=(" rows=",), env=NO_ROWS, twin="fcc444-swap"),
    Case("fcc444-flip-plain-solo", None, FLIP, ("^lean ", "solo=1"), wont=(" rows=",), env=NO_ROWS, twin="fcc444-flip"),
    # (the binary 6x6x6 cell fits the solo kernels too: the plain lean kernel is reached with SMOLMC_NO_SOLO)
    Case("triplets-swap", _triplets(SWAP), SWAP, ("^lean ",), wont=("solo=1",), env=NO_SOLO, constructions="ABC"),
    Case("triplets-flip", _triplets(FLIP), FLIP, ("^lean ",), wont=("solo=1",), env=NO_SOLO, constructions="ABC"),
    Case("fcc223-ternary-corr-kf", _fcc([2, 2, 3], SWAP, nspecies=3, mode=CORR), SWAP, ("^lean ", "kf=1")),
    Case("rocksalt322-two-sublattices", _two_sublattices(INT), SWAP, ("^lean-multi",), constructions="AC"),
    Case("rocksalt322-corr-lazy", _two_sublattices(CORR), SWAP, ("^lean-multi", "lazy-features")),
    Case("fcc222-walker-mu", _walker_mu, FLIP, ("^lean", "walker_mu=1")),
]}
RUNS = {k: [c.name for c in CASES.values() if k in c.constructions] for k in "ABC"}


def clean_env(monkeypatch, case, scale=None):
    """The environment of a case: the dispatch switches cleared, then the case's own variables and the band scale
    (before the handle is created)."""
    for v in cl.DISPATCH_SWITCHES + ("SMOLMC_FAST_EPS_SCALE",):
        monkeypatch.delenv(v, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if scale is not None:
        monkeypatch.setenv("SMOLMC_FAST_EPS_SCALE", repr(float(scale)))


# ---- the oracle's view of a step ----------------------------------------------------------------------------------
def uniform_of(seed, step):
    """The acceptance uniform of step ``step`` of the walker with seed ``seed``: words 2 and 3 of Philox block 0."""
    from oracle import oracle as orc

    seed, step = int(seed), int(step)
    w = orc.philox([step & 0xffffffff, step >> 32, 0, 0], [seed & 0xffffffff, seed >> 32])
    return float(((w[2] >> 5) << 26) | (w[3] >> 6)) / 9007199254740992.0


def uniforms_of(seeds, steps):
    """``uniform_of`` for arrays: Philox4x32-10 (Salmon et al., SC'11) in NumPy, counter (step lo, step hi, 0, 0), key the
    seed (tests/test_fast_band_host.py::test_numpy_philox_is_the_oracles holds it against the oracle's own Philox)."""
    seeds, steps = np.broadcast_arrays(np.asarray(seeds, dtype=np.uint64), np.asarray(steps, dtype=np.uint64))
    m32 = np.uint64(0xffffffff)
    c = [steps & m32, steps >> np.uint64(32), np.zeros_like(steps), np.zeros_like(steps)]
    k0, k1 = seeds & m32, seeds >> np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return (((c[2] >> np.uint64(5)) << np.uint64(26)) | (c[3] >> np.uint64(6))).astype(np.float64) / 9007199254740992.0


def flips_of(nf, fl):
    return [(int(fl[2 * j]), int(fl[2 * j + 1])) for j in range(nf)]


class Pricer:
    """Exact dH and scale A of a proposal on one TableSet, in float64 on the oracle's evaluator."""

    def __init__(self, tab):
        from oracle import oracle as orc

        self.ev = orc.OracleEvaluator(tab)
        self.nat = self.ev.natural_parameters()
        self.absnat = np.abs(self.nat)

    def __call__(self, occ, flips):
        if not flips:
            return 0.0, 0.0
        d = self.ev.feature_vector_change(occ, flips)
        dH = float(d @ self.nat)
        return dH, float(np.abs(d) @ self.absnat) + abs(dH)

    def bound(self, occ):
        """``price(nf, rec)`` of many proposals from ONE state ((nf, rec): what OracleMC.propose returns), on
        OracleEvaluator.bind: ``price.move(nf, rec)`` makes the state take the step, ``price.occ`` is the state."""
        change = self.ev.bind(occ)

        def price(nf, rec):
            if nf == 0:
                return 0.0, 0.0
            d = change(nf, rec)
            dH = float(d @ self.nat)
            return dH, float(np.abs(d) @ self.absnat) + abs(dH)
        price.move, price.occ = change.move, change.occ
        return price

    def floor(self, occ):
        """The noise floor of A at a state: 2^-16 of |features| @ |natural parameters|.  A swap of two sites in mirror
        environments has dH = 0 exactly; float64 leaves |dH| ~ A ~ 1e-16 there (five of the 4096 walkers of the fcc 4x4x4
        swap), which passes dH > 2^-20 A although nothing is uphill, and the sign of such a dH is that of one summation
        order.  The next smallest A of these models is 14 orders of magnitude above, so the floor excludes nothing else."""
        return NOISE_FLOOR * float(np.abs(self.ev.feature_vector(np.ascontiguousarray(occ, dtype=np.int32))) @ self.absnat)

    def from_scratch(self, occ, flips):
        after = occ.copy()
        for s, c in flips:
            after[s] = c
        return float((self.ev.feature_vector(after) - self.ev.feature_vector(occ)) @ self.nat)


def random_starts(case, R, rng):
    """Random occupancies at several compositions: walker r draws its codes as floor(u^g n_species), g cycling."""
    nsp = case.built["nsp"]
    g = np.array([0.4, 0.7, 1.0, 1.5, 2.5])[np.arange(R) % 5]
    return np.minimum((rng.random((R, len(nsp))) ** g[:, None] * nsp).astype(np.int32), nsp - 1).astype(np.int32)


def _oracles(case, R):
    """[(tables, pricer, walkers it speaks for (R,) bool)]: one per chemical-potential table of the case."""
    tab = case.tab
    if "big" not in case.built:
        return [(tab, Pricer(tab), np.ones(R, dtype=bool))]
    big = np.arange(R) % 8 == 3
    return [(tab, Pricer(tab), ~big), (case.built["big"], Pricer(case.built["big"]), big)]


def walker_mu_rows(case, R):
    """The rows of set_walker_mu of a case with per-walker chemical potentials (None for the others)."""
    if "big" not in case.built:
        return None
    rows = np.tile(WALKER_MU_SMALL[None, None, :], (R, 1, 1))
    rows[np.arange(R) % 8 == 3] *= WALKER_MU_FACTOR
    return rows


class Construction:
    """What a handle is set to and what it must then do: occ (R, N), seeds, n_steps, temperature (R,), steps of the
    launch, adversarial (R,) bool, sign (R,) (+1: the exact rule accepts the tested step), tested (R,) the index of
    the tested step within the launch, dH, A (R,), checked (the 16 walkers cross-checked from scratch)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def flipped(self):
        """The same construction with every hair's sign reversed."""
        c = Construction(**self.__dict__)
        c.sign = -self.sign
        c.temperature = np.where(self.adversarial, self.tau(c.sign) / KB, self.temperature)
        return c

    def tau(self, sign):
        return (self.dH + sign * HAIR * self.A) / self.neg_log_u


def set_up(handle, con, mu_rows=None):
    handle.set_state(con.occ, con.seeds, con.temperature)
    handle.set_counters(n_steps=con.n_steps)
    if mu_rows is not None and hasattr(handle, "set_walker_mu"):
        handle.set_walker_mu(mu_rows)


def oracle_run(case, con):
    """The oracle's state after the construction's launch (dict of get_state, walkers of every chemical-potential
    table from the oracle of that table)."""
    from oracle import oracle as orc

    R = len(con.occ)
    out = None
    for tab, _, mask in _oracles(case, R):
        ora = orc.OracleMC(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, case.step))
        set_up(ora, con)
        ora.run(con.steps)
        st = ora.get_state()
        if out is None:
            out = st
        else:
            for k in out:
                out[k][mask] = st[k][mask]
    return out


def oracle_rows(case, con, chunks):
    """The oracle's state after every one of the ``chunks`` run() calls of the construction's launch."""
    from oracle import oracle as orc

    (tab, _, _), = _oracles(case, len(con.occ))
    ora = orc.OracleMC(tab, capi.make_config(len(con.occ), capi.KERNEL_METROPOLIS, case.step))
    set_up(ora, con)
    out = []
    for n in chunks:
        ora.run(n)
        out.append(ora.get_state())
    return out


def oracle_decisions(case, con):
    """accepted (R,) bool of the TESTED step of every walker on the oracle, and n_accepted (R,) before it."""
    from oracle import oracle as orc

    R = len(con.occ)
    acc, before = np.zeros(R, dtype=bool), np.zeros(R, dtype=np.int64)
    for tab, _, mask in _oracles(case, R):
        ora = orc.OracleMC(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, case.step))
        set_up(ora, con)
        nacc = ora.get_state()["n_accepted"].astype(np.int64)
        for j in range(int(con.tested.max()) + 1):
            hit = mask & (con.tested == j)
            ora.run(1)
            st = ora.get_state()
            before[hit], acc[hit] = nacc[hit], st["accepted"][hit]
            nacc = st["n_accepted"].astype(np.int64)
    return acc, before


def _price_next(case, occ, seeds, n_steps, R, todo=None, out=None):
    """Proposal, uniform, dH and A of the step the walkers ``todo`` take next from (occ, seeds, n_steps)."""
    from oracle import oracle as orc

    flips, dH, A, nlu = out or ([None] * R, np.zeros(R), np.zeros(R), np.ones(R))
    todo = np.ones(R, dtype=bool) if todo is None else todo
    for tab, price, mask in _oracles(case, R):
        ora = orc.OracleMC(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, case.step))
        ora.set_state(occ, seeds, CONTROL_T)
        for r in np.flatnonzero(mask & todo):
            flips[r] = flips_of(*ora.propose(r, int(n_steps[r])))
            dH[r], A[r] = price(occ[r], flips[r])
            u = uniform_of(seeds[r], n_steps[r])
            nlu[r] = -np.log(u) if u > 0.0 else np.inf
    return flips, dH, A, nlu


def _cross_check(case, occ, flips, dH, pick):
    R = len(occ)
    for tab, price, mask in _oracles(case, R):
        for r in pick:
            if mask[r]:
                np.testing.assert_allclose(price.from_scratch(occ[r], flips[r]), dH[r], rtol=0, atol=1e-9)
    return np.asarray(pick)


@functools.lru_cache(maxsize=None)
def construction_a(name, R=R_A):
    case = CASES[CASES[name].twin or name]
    rng = np.random.default_rng(case.seed_base)
    occ = random_starts(case, R, rng)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(case.seed_base)
    n_steps = (np.arange(R) % 128).astype(np.uint64)
    flips, dH, A, nlu = _price_next(case, occ, seeds, n_steps, R)
    floor = np.zeros(R)
    for _, price, mask in _oracles(case, R):
        floor[mask] = [price.floor(occ[r]) for r in np.flatnonzero(mask)]
    for redraw in range(1, 4):  # a walker whose next proposal is not uphill gets another seed (three redraws at most)
        adv = (dH > UPHILL * A) & (A > floor) & np.isfinite(nlu) & (nlu > 0)
        seeds[~adv] += np.uint64(R)
        _price_next(case, occ, seeds, n_steps, R, ~adv, (flips, dH, A, nlu))
    adv = (dH > UPHILL * A) & (A > floor) & np.isfinite(nlu) & (nlu > 0)
    sign = np.where(np.arange(R) % 2 == 0, 1.0, -1.0)
    con = Construction(occ=occ, seeds=seeds, n_steps=n_steps, steps=1, adversarial=adv, sign=sign, dH=dH, A=A,
                       neg_log_u=nlu, tested=np.zeros(R, dtype=np.int64), temperature=None)
    con.temperature = np.where(adv, con.tau(sign) / KB, CONTROL_T)
    con.checked = _cross_check(case, occ, flips, dH, np.flatnonzero(adv)[:: max(1, int(adv.sum()) // 16)][:16])
    return con


@functools.lru_cache(maxsize=None)
def construction_b(name, R=R_B, n=N_B):
    from oracle import oracle as orc

    case = CASES[CASES[name].twin or name]
    assert "big" not in case.built
    tab, N = case.tab, case.tab.num_sites
    rng = np.random.default_rng(case.seed_base + 1)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(case.seed_base + 100_000)
    ora = orc.OracleMC(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, case.step))
    ora.set_state(random_starts(case, R, rng), seeds, 1e-3)
    ora.run(50 * N)  # the quench: 50 sweeps at 1e-3 K
    st = ora.get_state()
    occ, n0 = st["occupancy"], st["n_steps"].astype(np.uint64)
    price = Pricer(tab)
    dH, A, nlu = np.zeros(R), np.zeros(R), np.ones(R)
    tested, adv = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=bool)
    flips_k = [[] for _ in range(R)]
    U = uniforms_of(seeds[:, None], n0[:, None] + np.arange(n, dtype=np.uint64)[None, :])
    propose = ora.proposer()
    for r in range(R):
        tau, rec, price_r, s0, floor = [], [], price.bound(occ[r]), int(n0[r]), price.floor(occ[r])
        for j in range(n):  # the uphill prefix: the state stays while every step is rejected
            nf, raw = propose(r, s0 + j)
            d, a = price_r(nf, raw)
            fl = flips_of(nf, raw)
            u = U[r, j]
            if not (d > UPHILL * a and a > floor and u > 0.0):
                break
            tau.append(d / -np.log(u))
            rec.append((fl, d, a, -np.log(u)))
        if not tau:
            continue
        k = int(np.argmin(tau))
        tested[r], flips_k[r] = k, rec[k][0]
        dH[r], A[r], nlu[r] = rec[k][1:]
        adv[r] = all(t > 1.001 * tau[k] for t in tau[:k])  # every earlier step is rejected, far from its threshold
    sign = np.where(np.arange(R) % 2 == 0, 1.0, -1.0)
    con = Construction(occ=occ, seeds=seeds, n_steps=n0, steps=n, adversarial=adv, sign=sign, dH=dH, A=A, neg_log_u=nlu,
                       tested=tested, temperature=None)
    con.temperature = np.where(adv, con.tau(sign) / KB, CONTROL_T)
    con.checked = _cross_check(case, occ, flips_k, dH, np.flatnonzero(adv)[:: max(1, int(adv.sum()) // 16)][:16])
    return con


def residues(con):
    """The lanes of the 64-step threshold batch on which the tested steps of the adversarial walkers sit."""
    return np.unique((con.n_steps[con.adversarial].astype(np.int64) + con.tested[con.adversarial]) % 64)


# ---- construction C: replay --------------------------------------------------------------------------------------
def _host_proposal(subs, cum, step, occ, rng, rec):
    """One proposal of the reference's ushers from the host's own generator, written into ``rec``: the flips."""
    sites, codes = subs[int(np.searchsorted(cum, rng.random(), side="right"))] if len(subs) > 1 else subs[0]
    s1 = int(sites[rng.integers(len(sites))])
    if step == FLIP:
        other = [c for c in codes if c != occ[s1]]
        rec[0], rec[1] = s1, other[rng.integers(len(other))]
        return 1
    other = sites[occ[sites] != occ[s1]]
    if len(other) == 0:
        return 0
    s2 = int(other[rng.integers(len(other))])
    rec[0], rec[1], rec[2], rec[3] = s1, occ[s2], s2, occ[s1]
    return 2


@functools.lru_cache(maxsize=None)
def construction_c(name, R=R_C, n=N_C, flip=False):
    """dict(occ, seeds, temperature (R,), steps (R, n, 4) int32, uniforms (R, n), accepted (R, n) bool the host's
    decisions, adversarial (R, n) bool, H (R, n) the host's enthalpy after every step, checked); ``flip`` reverses every
    sign (the chains then part at the first adversarial step of every walker)."""
    case = CASES[CASES[name].twin or name]
    tab = case.tab
    occ0 = random_starts(case, R, np.random.default_rng(case.seed_base + 2))
    T = np.geomspace(300.0, 3000.0, R)
    price = Pricer(tab)
    subs = [(np.asarray(sl["active_sites"]), [int(c) for c in sl["codes"]]) for sl in tab.sublattices]
    cum = np.cumsum(np.asarray(tab._keep["sub_probs"], dtype=np.float64))[:-1]
    steps = np.full((R, n, 4), -1, dtype=np.int32)
    u, acc, adv, H = np.full((R, n), 0.5), np.zeros((R, n), dtype=bool), np.zeros((R, n), dtype=bool), np.zeros((R, n))
    checked, log_half = 0, np.log(0.5)
    probe_occ = np.zeros_like(occ0)  # the state of walker r before its step r mod n: the one-step probes of the sweep
    for r in range(R):
        rng = np.random.default_rng([case.seed_base + 2, r])  # (one generator per walker: the chains are independent)
        to_check = r % 64 == 0  # the first adversarial step of 16 walkers is cross-checked from scratch
        walk, beta, floor = price.bound(occ0[r]), 1.0 / (KB * T[r]), price.floor(occ0[r])
        occ = walk.occ
        h = float(price.ev.feature_vector(occ) @ price.nat)
        for j in range(n):
            rec = steps[r, j]
            if j == r % n:
                probe_occ[r] = occ
            nf = _host_proposal(subs, cum, case.step, occ, rng, rec)
            dH, A = walk(nf, rec)
            if dH > UPHILL * A and A > floor and 1e-3 <= beta * dH <= 600.0:
                sign = (1.0 if rng.random() < 0.5 else -1.0) * (-1.0 if flip else 1.0)
                u[r, j] = np.exp(-beta * (dH + sign * HAIR * A))
                adv[r, j], a = True, sign > 0
                if to_check:
                    np.testing.assert_allclose(price.from_scratch(occ, flips_of(nf, rec)), dH, rtol=0, atol=1e-9)
                    checked, to_check = checked + 1, False
            else:  # the plain rule at u = 0.5
                a = -beta * dH >= 0 or -beta * dH > log_half
            if a:
                walk.move(nf, rec)
                h += dH
            acc[r, j], H[r, j] = a, h
    jr = np.arange(R) % n
    pick = (np.arange(R), jr)
    probe = dict(occ=probe_occ, seeds=np.arange(R, dtype=np.uint64), temperature=T, steps=steps[pick][:, None, :],
                 uniforms=u[pick][:, None], accepted=acc[pick][:, None], adversarial=adv[pick][:, None])
    return dict(occ=occ0, seeds=np.arange(R, dtype=np.uint64), temperature=T, steps=steps, uniforms=u, accepted=acc,
                adversarial=adv, H=H, checked=checked, probe=probe)


def replay(case, handle, con):
    handle.set_state(con["occ"], con["seeds"], con["temperature"])
    return handle.replay(con["steps"], con["uniforms"])


# ---- judging a handle ----------------------------------------------------------------------------------------------
def wrong_decisions(con, st):
    """Adversarial walkers of a one-step construction whose decision is not the one the hair's sign implies."""
    return int(np.sum(con.adversarial & (st["accepted"] != (con.sign > 0))))


def assert_parity(a, b):
    assert np.array_equal(a["accepted"], b["accepted"])
    assert np.array_equal(a["n_accepted"], b["n_accepted"])
    assert np.array_equal(a["n_steps"], b["n_steps"])
    assert np.array_equal(a["occupancy"], b["occupancy"])
    np.testing.assert_allclose(a["enthalpy"], b["enthalpy"], rtol=RTOL, atol=ATOL)


def margin(counts):
    """The largest scale of a sweep {scale: (wrong, total)} with a wrong decision (None: none)."""
    bad = [s for s, (w, _) in counts.items() if w > 0]
    return max(bad) if bad else None


# ---- on the device -------------------------------------------------------------------------------------------------
def _engine(case, R):
    from smol_amd.engine import Engine

    return Engine(case.tab, capi.make_config(R, capi.KERNEL_METROPOLIS, case.step))


def launch(case, con, after=None):
    """One fresh handle through the construction's launch: (state, kernel_info[, what ``after(handle)`` returns]); the
    kernel family of the case is asserted."""
    eng = _engine(case, len(con.occ))
    try:
        set_up(eng, con, walker_mu_rows(case, len(con.occ)))
        eng.run(con.steps)
        st = eng.get_state()
        info = eng.kernel_info()  # (after the launch: the per-walker rows are part of the dispatch)
        extra = after(eng) if after else None
    finally:
        eng.close()
    assert case.family_ok(info), (case.want, case.wont, info)
    return (st, info, extra) if after else (st, info)


def launch_replay(case, con):
    """(accepted, H, kernel_info) of construction C on a fresh handle."""
    eng = _engine(case, len(con["occ"]))
    try:
        acc, H = replay(case, eng, con)
        info = eng.kernel_info()
    finally:
        eng.close()
    assert case.family_ok(info), (case.want, case.wont, info)
    return acc, H, info


INFO = {}  # (case, construction) -> the kernel_info string the handles of its last sweep reported


def sweep_a(name, set_env, scales=SCALES):
    """{scale: (wrong, total)} of construction A; ``set_env(scale)`` prepares the environment of the next handle."""
    case, con = CASES[name], construction_a(name)
    out = {}
    for s in scales:
        set_env(s)
        st, info = launch(case, con)
        out[s] = (wrong_decisions(con, st), int(con.adversarial.sum()))
        INFO[(name, "A")] = info
    return out


def sweep_c(name, set_env, scales=SCALES):
    """{scale: (wrong, total)} of construction C's one-step probes: walker r replays step r mod n of its chain alone,
    from the state the host's chain had before it (a wrong decision inside a chain would make the later records of
    that walker improper swaps of the state it is then in, which a swap handle refuses)."""
    case, con = CASES[name], construction_c(name)["probe"]
    out = {}
    for s in scales:
        set_env(s)
        acc, _, info = launch_replay(case, con)
        out[s] = (int(np.sum((acc != con["accepted"]) & con["adversarial"])), int(con["adversarial"].sum()))
        INFO[(name, "C")] = info
    return out


def sweep_line(name, kind, counts):
    m = margin(counts)
    return (f"[fast band] {name} {kind}: wrong/total per scale " + " ".join(f"2^{int(np.log2(s))}:{w}/{t}" for s, (w, t) in counts.items())
            + f"; largest scale with a wrong decision: {'none' if m is None else f'2^{int(np.log2(m))}'}")


# ---- Wang-Landau: the bin pre-test of mc_wl.h ------------------------------------------------------------------------
# All entropies zero and a modification factor of 1e-30: no entropy difference ever reaches log u, so every in-window
# step is accepted and the trajectory does not depend on the windows.  ONE oracle with a window never hit walks a pool
# of chains a step at a time and yields H after every step; per-walker windows (or the handle's window) then put the
# proposed enthalpy of the LAST step of a k-step launch 1e-8 bin from an interior bin edge (half the walkers), from
# the window's upper end (a quarter) or from its lower end (a quarter; beyond an end the step is rejected, which is
# why it is the last).  Expected bins: floor((H - vmin) / bin) by float64 floor division, wanglandau.py's rule.
# A walker whose earlier steps come within 0.01 bin of a window end -- for the end types: whose H_k is not the running
# extreme of its path -- is a control with its path in the middle of its window; at most half may be.
# Teeth: the band-scale sweep of the Metropolis cases has nothing to find here -- the tolerance of the pre-test in bins
# is tol0 + resync_after * e1b = WL_RESYNC_FRAC (0.005 bin) at EVERY scale of the band (mc_wl.h:193-197), so an enthalpy
# 1e-8 bin from an edge always takes the exact path.  What these runs hold is therefore everything around the float32
# sum: tol0 / tolb and the float32 roundings of the thresholds (a pre-test that trusted a position 1e-8 bin from an
# edge would put half of these walkers into the neighbouring bin or on the wrong side of a window end), the forced
# resync after many accepted steps, and the exact path's floor division and window test.  Both signs of the hair are
# among the walkers of every run and their expected histograms differ (asserted on the host).
WL_KS, WL_BINS, WL_HAIR, WL_R, WL_POOL = (1, 2, 17, 64, 200), (0.11, 0.011), 1e-8, 1024, 4096
WL_L = {0.11: 128, 0.011: 1024}  # bins per window: at least 40, and wide enough for the 200-step paths of the pool
WL_MOD = 1e-30


def wl_tab():
    return CASES["triplets-swap"].tab


def wl_config(R, vmin, vmax, bin_size):
    return capi.make_config(R, capi.KERNEL_WANGLANDAU, SWAP, min_enthalpy=float(vmin), max_enthalpy=float(vmax),
                            bin_size=float(bin_size), check_period=0, mod_factor=WL_MOD)


@functools.lru_cache(maxsize=None)
def wl_pool(P=WL_POOL):
    """dict(occ0 (P, N), seeds (P,), H (P, 201) the enthalpy after every step, occ {j: (P, N)} the occupancies after the
    steps k - 1 and k of every launch length): the all-accepting chains, walked once on one wide-window oracle."""
    from oracle import oracle as orc

    tab = wl_tab()
    rng = np.random.default_rng(20261019)
    occ0 = (rng.random((P, tab.num_sites)) < 0.5).astype(np.int32)
    seeds = np.arange(P, dtype=np.uint64) + np.uint64(31_000_003)
    ora = orc.OracleMC(tab, wl_config(P, -1e4, 1e4, 100.0))
    ora.set_state(occ0, seeds, 0.0)
    n, keep = max(WL_KS), {k - 1 for k in WL_KS} | set(WL_KS)
    H, occ = np.zeros((P, n + 1)), {}
    for j in range(n + 1):
        st = ora.get_state()
        H[:, j] = st["enthalpy"]
        if j in keep:
            occ[j] = st["occupancy"]
        assert np.all(st["n_accepted"] == j)  # the oracle accepts every in-window step
        if j < n:
            ora.run(1)
    return dict(occ0=occ0, seeds=seeds, H=H, occ=occ)


def _top(vmin, L, b):
    """vmin + L bins, an ulp lower where rounding would make the ceil rule count L + 1."""
    vmax = vmin + L * b
    while int(np.ceil((vmax - vmin) / b)) > L:
        vmax = np.nextafter(vmax, -np.inf)
    return vmax


def _bottom(vmax, L, b):
    vmin = vmax - L * b
    while int(np.ceil((vmax - vmin) / b)) > L:
        vmin = np.nextafter(vmin, np.inf)
    return vmin


def wl_window(path, kind, sign, L, b):
    """(vmin, vmax, adversarial) for a chain with enthalpies ``path`` (H_0 .. H_k): kind 0 an interior edge, 1 the upper
    end, 2 the lower end, ``sign`` +1 the proposed enthalpy H_k on the upper side of the edge (inside the window for the
    lower end, outside for the upper one); not adversarial: the path in the middle of the window, no hair."""
    Hp, lo, hi = path[-1], path.min(), path.max()
    mid = 0.5 * (lo + hi) - 0.5 * L * b
    if kind == 0:
        m = int(np.clip(np.round((Hp - mid) / b), 1, L - 1))
        vmin = Hp - (m + sign * WL_HAIR) * b
        vmax = _top(vmin, L, b)
    elif kind == 1:
        vmax = Hp - sign * WL_HAIR * b
        vmin = _bottom(vmax, L, b)
    else:
        vmin = Hp - sign * WL_HAIR * b
        vmax = _top(vmin, L, b)
    before = path[:-1]
    ok = bool(np.all(before > vmin + 0.01 * b) and np.all(before < vmax - 0.01 * b))
    if kind == 0:  # the hair as it came out in float64: on the side asked for, 1e-8 bin to a factor of two
        off = (Hp - vmin) / b - m
        ok = ok and 0.5 * WL_HAIR < sign * off < 2.0 * WL_HAIR
    elif kind == 1:
        ok = ok and 0.5 * WL_HAIR * b < sign * (Hp - vmax) < 2.0 * WL_HAIR * b and (Hp < vmax) == (sign < 0)
    else:
        ok = ok and 0.5 * WL_HAIR * b < sign * (Hp - vmin) < 2.0 * WL_HAIR * b and (Hp >= vmin) == (sign > 0)
    if not ok:
        vmin = mid
        vmax = _top(vmin, L, b)
        assert np.all(path > vmin + 0.01 * b) and np.all(path < vmax - 0.01 * b)
    return vmin, vmax, ok


def wl_expected(pool, chain, vmin, vmax, k, L, b):
    """dict(histogram (R, L), n_accepted (R,), occupancy (R, N), accepted_last (R,)) after a k-step launch of the chains
    ``chain`` in the windows [vmin, vmax): every step but the last is accepted, the last one when H_k is in the window;
    the bin of the state after every step by exact float64 floor division."""
    H = pool["H"][chain, : k + 1]
    last = (H[:, k] >= vmin) & (H[:, k] < vmax)
    after = H[:, 1:].copy()
    if k >= 1:
        after[:, -1] = np.where(last, H[:, k], H[:, k - 1])
    bins = np.floor_divide(after - vmin[:, None], b).astype(np.int64)
    assert bins.min() >= 0 and bins.max() < L
    hist = np.zeros((len(chain), L), dtype=np.int64)
    np.add.at(hist, (np.arange(len(chain))[:, None], bins), 1)
    occ = np.where(last[:, None], pool["occ"][k][chain], pool["occ"][k - 1][chain])
    return dict(histogram=hist, n_accepted=(k - 1 + last).astype(np.int64), occupancy=occ, accepted_last=last)


@functools.lru_cache(maxsize=None)
def wl_construction(k, b, R=WL_R):
    """Per-walker windows: walker r is of kind (0, 0, 1, 2)[r mod 4] with the sign alternating every four walkers.  The
    end kinds take the chains of the pool whose H_k is the running extreme of their path, the interior kind the others."""
    pool, L = wl_pool(), WL_L[b]
    H = pool["H"][:, : k + 1]
    fits = np.ptp(pool["H"], axis=1) < (L - 4) * b  # (the whole 200-step path fits a window: also as a control)
    top = fits & (H[:, k] > H[:, :k].max(axis=1) + 0.02 * b)
    bot = fits & (H[:, k] < H[:, :k].min(axis=1) - 0.02 * b)
    kind = np.array([0, 0, 1, 2])[np.arange(R) % 4]
    sign = np.where((np.arange(R) // 4) % 2 == 0, 1.0, -1.0)
    chain, vmin, vmax, adv = np.full(R, -1, dtype=np.int64), np.zeros(R), np.zeros(R), np.zeros(R, dtype=bool)
    for q, cand in ((1, top), (2, bot)):  # the end kinds first: they need their chains
        rows, take = np.flatnonzero(kind == q), np.flatnonzero(cand)
        chain[rows[: len(take)]] = take[: len(rows)]
    free = np.flatnonzero(fits & ~np.isin(np.arange(len(fits)), chain))
    rows = np.flatnonzero(chain < 0)  # the interior kind, and end walkers without a chain of their kind (controls)
    chain[rows] = free[: len(rows)]
    for r in range(R):
        vmin[r], vmax[r], adv[r] = wl_window(H[chain[r]], int(kind[r]), sign[r], L, b)
    exp = wl_expected(pool, chain, vmin, vmax, k, L, b)
    return dict(k=k, bin=b, L=L, chain=chain, kind=kind, sign=sign, vmin=vmin, vmax=vmax, adversarial=adv,
                occ0=pool["occ0"][chain], seeds=pool["seeds"][chain], expected=exp)


WL_WIDE = [(WL_BINS[i % 2], (i // 2) % 3, 1.0 if (i // 6) % 2 == 0 else -1.0, WL_KS[i % 5]) for i in range(24)]


@functools.lru_cache(maxsize=None)
def wl_wide_construction(i, R=64):
    """Handle i of the 24 with ONE window for the handle (the instantiation without per-walker windows): all walkers
    copies of one chain of the pool, the config's window tuned to that chain's step k."""
    b, kind, sign, k = WL_WIDE[i]
    pool, L = wl_pool(), WL_L[b]
    H = pool["H"][:, : k + 1]
    for c in range(i, len(H)):  # the first chain from i on that takes the window
        if np.ptp(pool["H"][c]) < (L - 4) * b:
            vmin, vmax, ok = wl_window(H[c], kind, sign, L, b)
            if ok:
                break
    else:
        raise AssertionError(("no chain of the pool takes the window", WL_WIDE[i]))
    chain = np.full(R, c)
    exp = wl_expected(pool, chain, np.full(R, vmin), np.full(R, vmax), k, L, b)
    return dict(k=k, bin=b, L=L, chain=chain, kind=np.full(R, kind), sign=np.full(R, sign), vmin=vmin, vmax=vmax,
                adversarial=np.ones(R, dtype=bool), occ0=pool["occ0"][chain], seeds=pool["seeds"][chain], expected=exp)


def wl_assert(con, st, wl):
    """histogram, occurrences, n_accepted and the occupancy of a handle after the launch, entry for entry."""
    exp = con["expected"]
    bad = np.flatnonzero(np.any(wl["histogram"] != exp["histogram"], axis=1))
    assert len(bad) == 0, (len(bad), [(int(r), int(con["kind"][r]), float(con["sign"][r]), bool(con["adversarial"][r])) for r in bad[:8]])
    assert np.array_equal(wl["occurrences"], exp["histogram"])
    assert np.array_equal(st["n_accepted"].astype(np.int64), exp["n_accepted"])
    assert np.array_equal(st["occupancy"], exp["occupancy"])


def wl_launch(con, per_walker):
    """(state, get_wl, kernel_info) of a fresh device handle after the construction's k-step launch."""
    from smol_amd.engine import Engine

    R = len(con["chain"])
    v0, v1 = (con["vmin"][0], con["vmax"][0]) if per_walker else (con["vmin"], con["vmax"])
    eng = Engine(wl_tab(), wl_config(R, v0, v1, con["bin"]))
    try:
        assert eng.L == con["L"]
        if per_walker:
            eng.set_wl_windows(con["vmin"], con["vmax"])
        eng.set_state(con["occ0"], con["seeds"])
        eng.set_wl(mod_factor=np.full(R, WL_MOD))
        eng.run(con["k"])
        st, wl, info = eng.get_state(), eng.get_wl(), eng.kernel_info()
    finally:
        eng.close()
    return st, wl, info


def wl_wrong_rows(con, st, wl):
    """Adversarial walkers whose histogram row, occurrences, accept counter or occupancy differs from the reference."""
    exp = con["expected"]
    bad = (np.any(wl["histogram"] != exp["histogram"], axis=1) | np.any(wl["occurrences"] != exp["histogram"], axis=1)
           | (st["n_accepted"].astype(np.int64) != exp["n_accepted"]) | np.any(st["occupancy"] != exp["occupancy"], axis=1))
    return int(np.sum(bad & con["adversarial"]))


WL_SWEEPS = {"wang-landau-walker-windows": (lambda: wl_construction(200, 0.011), True),
             "wang-landau-handle-window": (lambda: wl_wide_construction(9), False)}  # (k = 200, 0.011 eV bins, upper end)


def sweep_wl(name, set_env, scales=SCALES):
    """{scale: (wrong rows, adversarial walkers)} of a Wang-Landau construction, a fresh handle per scale.  A
    measurement: the tolerance of the pre-test is WL_RESYNC_FRAC of a bin at every scale, so no scale is expected to
    show a wrong row (see the comment above WL_KS)."""
    build, per_walker = WL_SWEEPS[name]
    con, out = build(), {}
    for s in scales:
        set_env(s)
        st, wl, info = wl_launch(con, per_walker)
        out[s] = (wl_wrong_rows(con, st, wl), int(con["adversarial"].sum()))
        INFO[(name, "WL")] = info
    return out
