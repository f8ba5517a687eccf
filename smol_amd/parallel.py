"""Multi-GPU layer: one process per GPU, replicas sharded across ranks.

The path shards into independent units: walkers never interact while sampling (the
reference's ``nwalkers`` are independent kernels, smol/moca/sampler/sampler.py:111-116,
:436-440), so there is NO data-path collective.  RCCL (torch.distributed backend "nccl"
on ROCm; "gloo" in the CPU tests) is used only for

  * ``global_sums``  -- all-reduce of O(F) float64 running sums at reporting time;
  * ``ReplicaExchange`` -- the temperature-ladder swap step of BASELINE config 5, which
    has no counterpart in the reference (NEW functionality; validated by invariants,
    not parity): all-gather of one float64 enthalpy per walker, then every rank takes
    the same swap decisions from a shared counter-based random stream and only the
    *temperature assignment* moves -- occupancies never leave their GPU.
"""

from __future__ import annotations

import math

import numpy as np

kB = 8.617333262145e-5  # smol/constants.py:4


def shard(total, rank, world):
    """Contiguous block of walkers owned by ``rank``: (first, count)."""
    base, rem = divmod(int(total), int(world))
    first = rank * base + min(rank, rem)
    return first, base + (1 if rank < rem else 0)


class _NoDist:
    """torch is optional for single-GPU use (engine.load_library treats it the same way)."""

    @staticmethod
    def is_available():
        return False

    @staticmethod
    def is_initialized():
        return False


def _dist():
    try:
        import torch.distributed as dist
    except ImportError:
        return _NoDist
    return dist


def rank_and_world():
    """(rank, world) of the initialised torch.distributed group, else (0, 1)."""
    dist = _dist()
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def collective_device():
    """Where tensors handed to a collective must live: "cuda" under RCCL ("nccl"), else "cpu"."""
    dist = _dist()
    if dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
        return "cuda"
    return "cpu"


def local_device(rank):
    """HIP device ordinal of a rank: LOCAL_RANK when the launcher exports it (one process per
    GPU; with per-rank device masking only device 0 is visible), else rank modulo the visible
    devices, else 0."""
    import os

    try:
        import torch

        n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    except Exception:
        n = 0
    lr = int(os.environ.get("LOCAL_RANK", rank))
    return lr % n if n else 0


def global_sums(local, group=None):
    """Sum a float64 tensor over all ranks (RCCL all-reduce); identity for one rank."""
    dist = _dist()
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(local, op=dist.ReduceOp.SUM, group=group)
    return local


def _philox_uniforms(seed, counter, n):
    """n uniforms in [0,1) from NumPy's counter-based Philox (Philox4x64, NOT the engine's
    Philox4x32-10) keyed by ``seed`` at ``counter``: a pure function of (seed, counter), so
    every rank draws the identical numbers without communicating."""
    bitgen = np.random.Philox(key=np.uint64(seed), counter=[0, 0, 0, np.uint64(counter)])
    return np.random.Generator(bitgen).random(n)


class ReplicaExchange:
    """Parallel-tempering bookkeeping over a global ladder of walkers.

    Global walker g lives on rank ``g // per_rank`` at local slot ``g % per_rank`` (equal
    shards).  ``ladder`` holds the temperatures of the rungs; ``rung_of[g]`` is the rung
    walker g currently samples at.  One ``exchange`` attempts swaps between walkers on
    neighbouring rungs (even pairs on even calls, odd pairs on odd calls), accepting
    with min(1, exp((beta_a - beta_b) (H_a - H_b))) -- the standard detailed-balance rule
    for exchanging temperatures between two canonical (or semigrand, H = E - mu N) chains.
    """

    def __init__(self, ladder, per_rank, rank=0, world=1, seed=0, group=None):
        self.ladder = np.asarray(ladder, dtype=np.float64)
        self.n = len(self.ladder)
        self.per_rank, self.rank, self.world, self.group = int(per_rank), int(rank), int(world), group
        if self.per_rank * self.world != self.n:
            raise ValueError("ladder length must equal per_rank * world")
        self.seed = int(seed)
        self.rung_of = np.arange(self.n)  # walker -> rung
        self.calls = 0
        self.exchange_seconds = 0.0  # host wall time spent in exchange steps (run_replica_exchange), walkers idle
        self.exchange_timed = 0
        self.attempted = np.zeros(self.n - 1, dtype=np.int64)
        self.accepted = np.zeros(self.n - 1, dtype=np.int64)

    # rung_of / attempted / accepted: host arrays; after `decide_on_device` attempts the current values live on the
    # GPU and every read brings them back first (sync_from_device), so no reader ever sees a stale ladder
    def _synced(name):
        def get(self):
            self.sync_from_device()
            return getattr(self, "_" + name)

        def put(self, value):
            setattr(self, "_" + name, value)

        return property(get, put)

    rung_of, attempted, accepted = _synced("rung_of"), _synced("attempted"), _synced("accepted")
    del _synced

    # ------------------------------------------------------------------------------
    @property
    def temperatures(self):
        """Temperature of every global walker."""
        self.sync_from_device()
        return self.ladder[self.rung_of]

    def local_temperatures(self):
        a = self.rank * self.per_rank
        return self.temperatures[a:a + self.per_rank].copy()

    def gather(self, local_enthalpy, force_collective=False):
        """All-gather the per-walker enthalpies (torch tensor, float64, len per_rank) into a
        NumPy array of all walkers.  8 bytes per walker: latency-bound over xGMI.
        ``force_collective`` runs the all-gather even for a single rank (a world-size-1 process
        group), so that the multi-GPU code path can be exercised on one GPU."""
        import torch

        dist = _dist()
        ready = dist.is_available() and dist.is_initialized()
        if not ready or (self.world == 1 and not force_collective):
            return local_enthalpy.detach().cpu().numpy().astype(np.float64)
        out = torch.empty(self.n, dtype=torch.float64, device=local_enthalpy.device)
        dist.all_gather_into_tensor(out, local_enthalpy.contiguous(), group=self.group)
        return out.cpu().numpy()

    def decide(self, enthalpy):
        """Swap decisions from the gathered enthalpies: pure function of (state, enthalpy),
        identical on every rank.  Returns the list of accepted rung pairs (k, k+1)."""
        self.sync_from_device()
        if getattr(self, "_dev", None) is not None:
            self._dev = None  # (host decisions from here on: the device copies would go stale)
        parity = self.calls & 1
        walker_at = np.empty(self.n, dtype=np.int64)  # rung -> walker
        walker_at[self.rung_of] = np.arange(self.n)
        pairs = np.arange(parity, self.n - 1, 2)
        u = _philox_uniforms(self.seed, self.calls, max(len(pairs), 1))
        beta = 1.0 / (kB * self.ladder)
        # the pairs of one parity are disjoint: all decisions of an attempt at once
        enthalpy = np.asarray(enthalpy, dtype=np.float64)
        a, b = walker_at[pairs], walker_at[pairs + 1]
        expo = (beta[pairs] - beta[pairs + 1]) * (enthalpy[a] - enthalpy[b])
        with np.errstate(divide="ignore"):
            acc = (expo >= 0) | (np.log(u[: len(pairs)]) < expo)
        self.attempted[pairs] += 1
        won = pairs[acc]
        self.rung_of[a[acc]] = won + 1
        self.rung_of[b[acc]] = won
        self.accepted[won] += 1
        self.calls += 1
        return [(int(k), int(k + 1)) for k in won]

    # ---- decisions on the device (smolmc_exchange_dev) ---------------------------------------------
    # The same attempt without the host in the loop: the all-gathered enthalpies stay on the GPU, one small kernel
    # takes the decisions of `decide` -- same arithmetic, same counter-based uniforms (their logs are made on the
    # host, a block of attempts ahead of time, and uploaded once per block) -- moves the rung assignment and sets the
    # engine's temperatures.  rung_of / attempted / accepted live in device tensors meanwhile; `sync_from_device`
    # (called by every reader below) brings them back.
    LOG_U_BLOCK = 64  # attempts whose log-uniforms are uploaded together

    def _device_state(self, device):
        import torch

        if getattr(self, "_dev", None) is None or self._dev["device"] != device:
            self._dev = dict(
                device=device,
                ladder=torch.from_numpy(self.ladder).to(device),
                rung_of=torch.from_numpy(self.rung_of.astype(np.int32)).to(device),
                stats=torch.from_numpy(np.concatenate([self.attempted, self.accepted]).astype(np.int64)).to(device),
                log_u=None, log_u_first=-1,
            )
            # (the uploads ran on torch's stream, the decision kernel runs on the engine's: they must have landed)
            torch.cuda.synchronize(device)
            self._dev_dirty = False
        return self._dev

    def _log_u_row(self, st):
        """Device row of log(u) for attempt `self.calls` (uploaded LOG_U_BLOCK attempts at a time)."""
        import torch

        if st["log_u"] is None or not (st["log_u_first"] <= self.calls < st["log_u_first"] + self.LOG_U_BLOCK):
            half = max(self.n // 2, 1)
            rows = np.zeros((self.LOG_U_BLOCK, half))
            for i in range(self.LOG_U_BLOCK):
                c = self.calls + i
                npairs = len(range(c & 1, self.n - 1, 2))
                with np.errstate(divide="ignore"):  # (the draws `decide` makes for attempt c, in its order)
                    rows[i, :npairs] = np.log(_philox_uniforms(self.seed, c, max(npairs, 1))[:npairs])
            st["log_u"] = torch.from_numpy(rows).to(st["device"])
            torch.cuda.synchronize(st["device"])  # (as above: another stream reads it)
            st["log_u_first"] = self.calls
        return st["log_u"][self.calls - st["log_u_first"]]

    def decide_on_device(self, engine, enthalpy_all_dev):
        """One attempt decided by `engine`'s GPU from the device tensor of ALL walkers' enthalpies (float64, global
        order); the engine's temperatures are set by the same kernel.  Identical decisions to `decide`."""
        st = self._device_state(enthalpy_all_dev.device)
        lu = self._log_u_row(st)
        engine.exchange_dev(self.n, self.rank * self.per_rank, self.calls & 1, enthalpy_all_dev.data_ptr(),
                            st["ladder"].data_ptr(), lu.data_ptr(), st["rung_of"].data_ptr(), st["stats"].data_ptr())
        self.calls += 1
        self._dev_dirty = True

    def sync_from_device(self):
        """Bring rung_of / attempted / accepted back from the device after `decide_on_device` attempts."""
        if getattr(self, "_dev_dirty", False):
            import torch

            self._dev_dirty = False  # (first: the assignments below go through the syncing properties)
            torch.cuda.synchronize(self._dev["device"])
            self.rung_of = self._dev["rung_of"].cpu().numpy().astype(np.int64)
            stats = self._dev["stats"].cpu().numpy()
            self.attempted, self.accepted = stats[: self.n - 1].copy(), stats[self.n - 1:].copy()
        return self

    def exchange(self, local_enthalpy, force_collective=False):
        """gather + decide; returns this rank's new temperatures (NumPy, len per_rank)."""
        self.decide(self.gather(local_enthalpy, force_collective))
        return self.local_temperatures()

    @property
    def acceptance(self):
        self.sync_from_device()
        return self.accepted / np.maximum(self.attempted, 1)


def geometric_ladder(t_min, t_max, n):
    """Geometric temperature ladder (400-2000 K)."""
    return np.geomspace(t_min, t_max, n)


def _refuse_walker_mu(target):
    """An exchange that permutes temperatures only is no valid move between walkers of different Hamiltonians: engines
    and samplers with per-walker chemical potentials are refused."""
    eng = getattr(target, "_engine", target)  # (a moca.Sampler, or an Engine)
    if getattr(target, "walker_chemical_potentials", None) is not None or getattr(eng, "walker_mu_set", False):
        raise ValueError("replica exchange with per-walker chemical potentials: an exchange of temperatures alone is "
                         "no valid move between walkers of different Hamiltonians")


def run_replica_exchange(engine, rex, n_exchanges, steps_between, device=None, collective=None, device_decide=None):
    """Alternate ``steps_between`` MC steps on every walker with one exchange attempt.

    ``engine`` is a smol_amd.engine.Engine holding this rank's ``rex.per_rank`` walkers.
    Collective path (several ranks, or ``collective=True``) on RCCL: the enthalpies are exported
    device-to-device into a torch tensor (smolmc_export_enthalpy_dev), all-gathered
    without staging through the host, and the new temperatures go back through a device
    tensor (smolmc_import_temperature_dev); initialise torch.cuda / the process group BEFORE
    creating the engine, as bench.py does.  Collective path on a CPU backend (gloo: the CPU
    tests, ``bench.py --oversubscribe`` / ``--dry-run``): the same all-gather over host tensors.
    Single rank (default): no collective is needed, the enthalpies are read back directly and
    the temperatures uploaded with set_temperature.  All paths take the same decisions
    (tests/test_gpu_device_plumbing.py, tests/test_parallel_gloo.py).
    ``device_decide`` (default: SMOLMC_REX_DEVICE_DECIDE=1 in the environment; collective device path only): the swap
    decisions are taken by a kernel on the all-gathered device tensor (smolmc_exchange_dev) instead of NumPy on a
    host copy -- no device-to-host copy, no host arithmetic and no temperature upload per attempt; `rex.rung_of` /
    `attempted` / `accepted` are brought back when read (`rex.sync_from_device()`)."""
    import os

    _refuse_walker_mu(engine)
    if device_decide is None:
        device_decide = os.environ.get("SMOLMC_REX_DEVICE_DECIDE") == "1"
    dist = _dist()
    ready = dist.is_available() and dist.is_initialized()
    multi = ready and (rex.world > 1 if collective is None else bool(collective))
    if collective and not ready:
        raise RuntimeError("collective=True needs an initialised torch.distributed process group")
    on_device = multi and (device is not None or collective_device() == "cuda")
    buf = tbuf = allbuf = None
    if multi:
        import torch
    if on_device:
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        buf = torch.empty(rex.per_rank, dtype=torch.float64, device=dev)
        tbuf = torch.empty(rex.per_rank, dtype=torch.float64, device=dev)
    import time

    engine.set_temperature(rex.local_temperatures())
    for _ in range(n_exchanges):
        engine.run(steps_between)
        if hasattr(engine, "sync"):
            engine.sync()  # (the exchange needs the launch's enthalpies anyway; timed from here: its own latency)
        t_ex = time.perf_counter()
        if on_device and device_decide:
            engine.export_enthalpy(buf.data_ptr())
            if allbuf is None:
                allbuf = torch.empty(rex.n, dtype=torch.float64, device=dev)
            if rex.world > 1 or collective:
                dist.all_gather_into_tensor(allbuf, buf, group=rex.group)
            else:
                allbuf.copy_(buf)
            torch.cuda.current_stream().synchronize()  # (the kernel runs on the engine's stream)
            rex.decide_on_device(engine, allbuf)
        elif on_device:
            engine.export_enthalpy(buf.data_ptr())
            new_t = rex.exchange(buf, force_collective=True)
            tbuf.copy_(torch.from_numpy(new_t))
            torch.cuda.current_stream().synchronize()
            engine.import_temperature(tbuf.data_ptr())
        elif multi:
            mine = torch.from_numpy(np.ascontiguousarray(engine.get_enthalpy(), dtype=np.float64))
            engine.set_temperature(rex.exchange(mine, force_collective=True))
        else:
            rex.decide(engine.get_enthalpy())
            engine.set_temperature(rex.local_temperatures())
        rex.exchange_seconds += time.perf_counter() - t_ex
        rex.exchange_timed += 1
    if on_device and device_decide and hasattr(engine, "sync"):
        engine.sync()  # (the last attempt's temperatures are in place when this returns)
    return rex


# ---- exchanges between disjoint pairs, decided on the device: what the mu-T grid and the Wang-Landau windows share ------
class PairExchange:
    """Bookkeeping of an exchange whose attempt is one device call on disjoint pairs with one host-made ``log u`` per
    pair (``Engine.exchange_grid``, ``Engine.exchange_wl``): the Philox seed, the attempt counter ``calls``, the pair
    table of every move of ``MOVES`` and the ``attempted`` / ``accepted`` counts per move and pair.  A subclass names its
    moves (``MOVES``), what makes a move the key of the tables (``_key``) and the engine's call (``ENGINE_CALL``), and
    defines ``decide``."""

    def _init_exchange(self, seed, pairs):
        self.philox_seed, self.calls, self._pairs = int(seed), 0, pairs
        self.attempted = {move: np.zeros(len(p), dtype=np.int64) for move, p in pairs.items()}
        self.accepted = {move: np.zeros(len(p), dtype=np.int64) for move, p in pairs.items()}

    def pairs(self, move):
        """(npairs, 2) entries of one move: disjoint, so that an attempt decides them at once."""
        return self._pairs[self._key(move)]

    def move_of(self, attempt):
        return self.MOVES[int(attempt) % len(self.MOVES)]

    def log_u(self, attempt, npairs):
        """log of the ``npairs`` uniforms of attempt ``attempt`` (a pure function of the seed and the attempt)."""
        with np.errstate(divide="ignore"):
            return np.log(_philox_uniforms(self.philox_seed, attempt, max(int(npairs), 1))[:npairs])

    def record(self, move, accept):
        self.attempted[self._key(move)] += 1
        self.accepted[self._key(move)] += np.asarray(accept, dtype=np.int64)

    @property
    def acceptance(self):
        """Accepted / attempted over all pairs of all moves."""
        att = sum(int(a.sum()) for a in self.attempted.values())
        return sum(int(a.sum()) for a in self.accepted.values()) / max(att, 1)

    @staticmethod
    def _holders(entry_of, pairs):
        """(s, t, a, b) of ``decide``: the two entries of every pair and the walkers that hold them under the walker ->
        entry map ``entry_of``."""
        walker_at = np.empty(len(entry_of), dtype=np.int64)
        walker_at[entry_of] = np.arange(len(entry_of))
        s, t = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
        return s, t, walker_at[s], walker_at[t]

    @staticmethod
    def _swapped(entry_of, s, t, a, b, accept):
        """The map after the accepted pairs swapped their entries."""
        new = entry_of.copy()
        new[a[accept]] = t[accept]
        new[b[accept]] = s[accept]
        return new

    def attempt(self, engine, engine_entry=None):
        """One attempt on the device: the move whose turn it is goes to ``engine`` with this attempt's ``log_u``, the
        accept flags come back into ``record`` and ``calls`` moves on.  ``engine_entry``: the engine's number of every
        entry, where it numbers them differently (``GridExchange.bind``)."""
        move = self.move_of(self.calls)
        pairs = self.pairs(move)
        stats = np.zeros((len(pairs), 2), dtype=np.int64)
        getattr(engine, self.ENGINE_CALL)(pairs if engine_entry is None else engine_entry[pairs],
                                          self.log_u(self.calls, len(pairs)), stats)
        self.record(move, stats[:, 1])
        self.calls += 1


# ---- exchange across a mu-T grid (hyper-parallel tempering, smolmc_exchange_grid) -------------------------------------
class GridExchange(PairExchange):
    """Bookkeeping of replica exchange across a grid of temperatures x rows of chemical potentials, in one handle.

    State point ``p = (rep * nT + i) * nMu + j`` is (``temperatures[i]``, ``rows[j]``) of replica set ``rep``;
    ``rows`` is (nMu, n_sublattices, mu_width) in the layout of ``Engine.set_walker_mu``.  ``point_of[w]`` is the point
    walker w samples at.  The four moves -- ``("T", 0)``, ``("T", 1)``, ``("mu", 0)``, ``("mu", 1)`` -- pair the
    neighbours along one axis at even or odd offsets, inside one replica set, so the pairs of a move are disjoint.

    Walker a at s = (beta_s, row_s), walker b at t, H_s(x) = E0(x) - n(x) . row_s, d = row_t - row_s:

        Delta = (beta_s - beta_t) (Hb - Ha) + beta_s (n_b . d) - beta_t (n_a . d);   accept iff -Delta >= 0 or log u < -Delta

    which is (beta_k - beta_k+1) (H_a - H_b) of ``ReplicaExchange`` when d = 0.  On acceptance the walkers swap their
    points; the chemical work of a gains n_a . d and its enthalpy loses it, b the other way round with n_b . d.
    ``decide`` is this move in NumPy, in the operation order of the device kernel (grid_exchange.hip)."""

    MOVES = (("T", 0), ("T", 1), ("mu", 0), ("mu", 1))
    ENGINE_CALL = "exchange_grid"
    _key = staticmethod(tuple)
    seed = property(lambda self: self.philox_seed)  # (under the constructor's name; WLWindows.seed is a method)

    def __init__(self, temperatures, rows, replicas=1, seed=0):
        self.temperatures = np.asarray(temperatures, dtype=np.float64).reshape(-1)
        rows = np.asarray(rows, dtype=np.float64)
        if rows.ndim != 3:
            raise ValueError(f"expected rows of shape (points along mu, active sublattices, mu_width), got {rows.shape}")
        self.rows = np.ascontiguousarray(rows)
        self.nT, self.nMu, self.replicas = len(self.temperatures), len(self.rows), int(replicas)
        self.npoints = self.replicas * self.nT * self.nMu
        _, i, j = np.unravel_index(np.arange(self.npoints), (self.replicas, self.nT, self.nMu))
        self.point_temperatures = self.temperatures[i]  # (npoints,)
        self.point_rows = self.rows[j]                  # (npoints, n_sublattices, mu_width)
        self.point_of = np.arange(self.npoints)         # walker -> point
        self._init_exchange(seed, {move: self._make_pairs(*move) for move in self.MOVES})

    def _make_pairs(self, axis, offset):
        grid = np.arange(self.npoints).reshape(self.replicas, self.nT, self.nMu)
        if axis == "T":
            lo, hi = grid[:, offset:self.nT - 1:2, :], grid[:, offset + 1:self.nT:2, :]
        elif axis == "mu":
            lo, hi = grid[:, :, offset:self.nMu - 1:2], grid[:, :, offset + 1:self.nMu:2]
        else:
            raise ValueError(f"unknown exchange axis {axis!r}")
        return np.stack([lo.reshape(-1), hi.reshape(-1)], axis=1).astype(np.int32).reshape(-1, 2)

    def bind(self):
        """For an engine whose walker q holds the point ``point_of[q]`` now, so that the engine's state point q is the
        grid's point base[q]: (engine_point, the engine's number of every point, for ``attempt``; read_back(engine),
        which sets ``point_of`` from the engine's walker -> point map)."""
        base = np.asarray(self.point_of, dtype=np.int64).copy()
        engine_point = np.empty(self.npoints, dtype=np.int64)
        engine_point[base] = np.arange(self.npoints)

        def read_back(engine):
            self.point_of = base[engine.state_points()[0]]

        return engine_point, read_back

    def decide(self, enthalpy, counts, point_of, move, attempt, log_u=None, record=True):
        """One attempt of ``move`` on the host: enthalpy (R,), species counts (R, n_sublattices, mu_width) and the
        walker -> point map in; returns dict(pairs, exponent (-Delta per pair), accept, point_of (new), work_delta
        (what each walker's chemical work gains; its enthalpy loses it), enthalpy (re-priced)).  The definition the
        device kernel is tested against: beta = 1 / (kB T), every product and sum rounded on its own, n . d summed
        over the cells sublattice by sublattice, code by code."""
        enthalpy = np.asarray(enthalpy, dtype=np.float64)
        point_of = np.asarray(point_of, dtype=np.int64)
        counts = np.asarray(counts).reshape(self.npoints, -1).astype(np.float64)
        cells = self.point_rows.reshape(self.npoints, -1)
        pairs = self.pairs(move)
        s, t, a, b = self._holders(point_of, pairs)
        beta = 1.0 / (kB * self.point_temperatures)
        wa, wb = np.zeros(len(pairs)), np.zeros(len(pairs))
        for c in range(cells.shape[1]):  # (written out: np.dot sums in another order)
            d = cells[t, c] - cells[s, c]
            wa = wa + counts[a, c] * d
            wb = wb + counts[b, c] * d
        delta = ((beta[s] - beta[t]) * (enthalpy[b] - enthalpy[a]) + beta[s] * wb) - beta[t] * wa
        if log_u is None:
            log_u = self.log_u(attempt, len(pairs))
        log_u = np.asarray(log_u, dtype=np.float64)
        accept = (-delta >= 0) | (log_u < -delta)
        new_point_of = self._swapped(point_of, s, t, a, b, accept)
        work = np.zeros(self.npoints)
        work[a[accept]] = wa[accept]
        work[b[accept]] = -wb[accept]
        if record:
            self.record(move, accept)
        return dict(pairs=pairs, exponent=-delta, accept=accept, point_of=new_point_of, work_delta=work,
                    enthalpy=enthalpy - work)


def run_grid_exchange(engine, gx, n_exchanges, steps_between, host_decide=False, history=None):
    """Alternate ``steps_between`` MC steps on every walker with one exchange attempt across the mu-T grid ``gx``,
    cycling its four moves.  ``engine`` holds ``gx.npoints`` walkers with their state loaded; walker w starts at point
    ``gx.point_of[w]``.  Default: the attempt is decided and applied on the device (``Engine.exchange_grid``), nothing
    but the accept flags comes back.  ``host_decide=True``: the state is read back, ``gx.decide`` takes the decisions
    and ``set_temperature`` + ``set_walker_mu`` apply them -- the cross-check of the device path, and what it is timed
    against.  ``history``: a list that receives ``gx.point_of`` after every attempt."""
    if engine.R != gx.npoints:
        raise ValueError(f"the grid has {gx.npoints} state points, the engine {engine.R} walkers")
    engine_point, read_back = gx.bind()
    engine.set_walker_mu(gx.point_rows[gx.point_of])
    engine.set_temperature(gx.point_temperatures[gx.point_of])
    for _ in range(int(n_exchanges)):
        engine.run(steps_between)
        if host_decide:
            move = gx.move_of(gx.calls)
            st = engine.get_state()
            res = gx.decide(st["enthalpy"], engine.species_counts(st["occupancy"]), gx.point_of, move, gx.calls)
            gx.point_of = res["point_of"]
            engine.set_temperature(gx.point_temperatures[gx.point_of])
            engine.set_walker_mu(gx.point_rows[gx.point_of])
            gx.calls += 1
        else:
            gx.attempt(engine, engine_point)
            if history is not None:
                read_back(engine)
        if history is not None:
            history.append(np.array(gx.point_of))
    if not host_decide:
        read_back(engine)
    return gx


# ---- replica-exchange Wang-Landau: overlapping energy windows in one handle (smolmc_exchange_wl) ----------------------
def wl_num_levels(vmin, vmax, bin_size):
    """Number of Wang-Landau levels of a window by the engine's rule (smolmc_create): ceil((vmax - vmin) / bin_size)."""
    return int(math.ceil((float(vmax) - float(vmin)) / float(bin_size)))


class WLWindows(PairExchange):
    """Bookkeeping of replica-exchange Wang-Landau (Vogel, Li, Wuest, Landau, PRL 110, 210603) in one handle.

    The global range ``[min_enthalpy, max_enthalpy)`` has ``L = ceil((max - min) / bin_size)`` bins.  It is cut into
    ``n_windows`` aligned windows of ``Lw`` bins at a stride of ``Ls`` bins, ``(n_windows - 1) Ls + Lw == L``:
    ``vmin_k = min + k Ls bin``, ``vmax_k = min + (k Ls + Lw) bin``.  ``overlap`` is the requested ``1 - Ls / Lw``
    (``window_bins`` / ``stride_bins`` name Lw / Ls outright).  Every window exists ``copies`` times; estimator
    ``e = k * copies + i`` is copy i of window k, in the order of ``Engine.set_wl_windows(wx.vmin, wx.vmax)``.
    ``estimator_of[w]`` is the estimator walker w holds.  Move 0 pairs the windows (0, 1), (2, 3), ..., move 1 the
    windows (1, 2), (3, 4), ..., copy i with copy i, so the pairs of a move are disjoint.

    Walker a holds estimator s, walker b estimator t; the pair is rejected unless Ea lies in t's window and Eb in s's.
    With ia(E) = (E - vmin_s) // bin, ib(E) = (E - vmin_t) // bin:

        ex = ((S_s[ia(Ea)] - S_s[ia(Eb)]) + S_t[ib(Eb)]) - S_t[ib(Ea)];   accept iff ex >= 0 or log u < ex

    and the walkers swap estimators.  ``decide`` is this move in NumPy, in the operation order of the device kernel
    (wl_exchange.hip); ``join`` makes one ln g of the pieces.  ``synchronise`` is the second half of the method -- the
    copies of a window pass the flatness check together and take the mean of their entropies -- ``sync_attempt`` runs it
    on the device, ``merges`` and ``mod_factor`` keep its count and the factor per window."""

    MOVES = (0, 1)
    ENGINE_CALL = "exchange_wl"
    _key = staticmethod(int)

    def __init__(self, min_enthalpy, max_enthalpy, bin_size, n_windows, overlap=0.5, copies=1, seed=0,
                 window_bins=None, stride_bins=None):
        self.min_enthalpy, self.max_enthalpy, self.bin_size = float(min_enthalpy), float(max_enthalpy), float(bin_size)
        self.n_windows, self.copies = int(n_windows), int(copies)
        if self.n_windows < 1 or self.copies < 1 or not (0.0 <= overlap < 1.0) or not self.bin_size > 0:
            raise ValueError("WLWindows needs n_windows >= 1, copies >= 1, 0 <= overlap < 1 and bin_size > 0")
        self.L = wl_num_levels(self.min_enthalpy, self.max_enthalpy, self.bin_size)
        n = self.n_windows
        if window_bins is None or stride_bins is None:
            lw0 = self.L / (1.0 + (n - 1) * (1.0 - overlap))
            stride_bins = max(1, int(math.floor(lw0 * (1.0 - overlap) + 1e-9))) if n > 1 else 0
            window_bins = self.L - (n - 1) * stride_bins
        self.Lw, self.Ls = int(window_bins), int(stride_bins)
        if self.Lw < 1 or (n - 1) * self.Ls + self.Lw != self.L or (n > 1 and not 1 <= self.Ls <= self.Lw):
            raise ValueError(f"{n} windows of {self.Lw} bins at a stride of {self.Ls} do not tile the {self.L} global bins")
        k = np.arange(n, dtype=np.float64)
        wmin = self.min_enthalpy + k * self.Ls * self.bin_size
        wmax = self.min_enthalpy + (k * self.Ls + self.Lw) * self.bin_size
        for j in range(n):
            # the engine sizes a window by ceil((vmax - vmin) / bin): a top edge that rounding put an ulp too high
            # would count one bin more, so it is stepped down until the rule gives Lw (a sliver of < 1e-15 relative)
            for _ in range(64):
                if wl_num_levels(wmin[j], wmax[j], self.bin_size) <= self.Lw:
                    break
                wmax[j] = np.nextafter(wmax[j], -np.inf)
            if wl_num_levels(wmin[j], wmax[j], self.bin_size) != self.Lw:
                raise ValueError(f"window {j} = [{wmin[j]!r}, {wmax[j]!r}) does not give {self.Lw} levels at bin size "
                                 f"{self.bin_size!r} by the engine's rule ceil((vmax - vmin) / bin)")
        self.window_min, self.window_max = wmin, wmax
        self.window_of = np.repeat(np.arange(n), self.copies)          # estimator -> window
        self.copy_of = np.tile(np.arange(self.copies), n)              # estimator -> copy
        self.vmin, self.vmax = wmin[self.window_of], wmax[self.window_of]  # (R,) in estimator order
        self.R = n * self.copies
        self.estimator_of = np.arange(self.R)
        self._init_exchange(seed, {m: self._make_pairs(m) for m in self.MOVES})  # (philox_seed: `seed` is the method below)
        self.merges = np.zeros(n, dtype=np.int64)   # merges of every window's copies so far (sync_attempt)
        self.mod_factor = np.full(n, np.nan)        # every window's modification factor at the latest sync_attempt

    # ---- the second half of the method: the copies of a window go through the Wang-Landau stages together --------------
    @staticmethod
    def flat(entropy_row, histogram_row, flatness):
        """The flatness criterion of one estimator, as the sampling kernels apply it (wl_multi_flatness_check): over the
        visited bins V = {i: S[i] > 0}, n = |V| >= 2, every float(hist[i]) > flatness * (float(sum of hist over V) /
        float(n)); the mean and the threshold are one rounding each."""
        S, hist = np.asarray(entropy_row, dtype=np.float64), np.asarray(histogram_row, dtype=np.int64)
        V = S > 0
        n = int(V.sum())
        if n < 2:
            return False
        mean = np.float64(int(hist[V].sum(dtype=np.int64))) / np.float64(n)
        thr = np.float64(flatness) * mean
        return bool(np.all(hist[V].astype(np.float64) > thr))

    def synchronise(self, entropy, histogram, mod_factor, copies=None, flatness=0.8, divisor=2.0):
        """The merge of the copies of every window (Vogel, Li, Wuest, Landau, PRL 110, 210603), on the host: entropy
        (R, L) float64, histogram (R, L) int64, mod_factor (R,), all in ESTIMATOR order as ``Engine.get_wl`` returns
        them; group g is the estimators g * copies .. g * copies + copies - 1 (``copies`` defaults to ``self.copies``:
        group g is window g).  Per group, in this order:

          status 2  the copies' factors are not all bitwise equal: the group is left alone;
          status 0  some copy is not ``flat``: the group is left alone;
          status 1  every bin i, visited or not: a = S_e0[i], a = a + S_e0+c[i] for c = 1 .. copies - 1 in that order,
                    S_e[i] = a / float(copies) for every copy; every copy's histogram becomes 0, its factor m / divisor.

        Returns dict(status (G,) int32, entropy, histogram, mod_factor): new arrays, the inputs are not written.  The
        definition the merge mode of wl_exchange_kernel (``Engine.wl_synchronise``) is tested against, bit for bit."""
        S = np.array(entropy, dtype=np.float64, ndmin=2)
        hist = np.array(histogram, dtype=np.int64, ndmin=2)
        m = np.array(mod_factor, dtype=np.float64).reshape(-1)
        copies = self.copies if copies is None else int(copies)
        R = len(m)
        if S.shape != hist.shape or S.shape[0] != R:
            raise ValueError(f"entropy {S.shape}, histogram {hist.shape} and mod_factor {m.shape} do not belong together")
        if copies < 1 or R % copies:
            raise ValueError(f"copies = {copies} does not divide the {R} estimators")
        status = np.zeros(R // copies, dtype=np.int32)
        for g in range(R // copies):
            e0 = g * copies
            if len(set(m[e0:e0 + copies].view(np.uint64).tolist())) != 1:
                status[g] = 2
                continue
            if not all(self.flat(S[e], hist[e], flatness) for e in range(e0, e0 + copies)):
                continue
            a = S[e0].copy()
            for c in range(1, copies):  # (written out: NumPy's pairwise reduction sums in another order)
                a = a + S[e0 + c]
            S[e0:e0 + copies] = a / np.float64(copies)
            hist[e0:e0 + copies] = 0
            m[e0:e0 + copies] = m[e0] / np.float64(divisor)
            status[g] = 1
        return dict(status=status, entropy=S, histogram=hist, mod_factor=m)

    def sync_attempt(self, engine, host=False):
        """One merge attempt of every window's copies on the device (``Engine.wl_synchronise``); ``merges`` counts the
        windows that merged, ``mod_factor`` holds every window's factor after the call.  ``host=True``: the same through
        the host -- ``get_wl``, ``synchronise``, ``set_wl`` -- the cross-check of the device path, and what it is timed
        against.  Returns the status (n_windows,)."""
        if host:
            wl = engine.get_wl()
            res = self.synchronise(wl["entropy"], wl["histogram"], wl["mod_factor"], flatness=engine.config.wl_flatness,
                                   divisor=engine.config.wl_mod_divisor)
            if (res["status"] == 1).any():
                engine.set_wl(entropy=res["entropy"], histogram=res["histogram"], mod_factor=res["mod_factor"])
            status, factor = res["status"], res["mod_factor"][::self.copies]
        else:
            res = engine.wl_synchronise(self.copies)
            status, factor = res["status"], res["mod_factor"]
        self.merges += status == 1
        self.mod_factor = np.array(factor, dtype=np.float64)
        return status

    def converged(self, final_mod_factor):
        """Whether every window's factor (at the latest ``sync_attempt``) is at or below ``final_mod_factor``."""
        return bool(np.all(self.mod_factor <= float(final_mod_factor)))

    def _make_pairs(self, move):
        lo = np.arange(int(move), self.n_windows - 1, 2)
        i = np.arange(self.copies)
        s = (lo[:, None] * self.copies + i[None, :]).reshape(-1)
        return np.stack([s, s + self.copies], axis=1).astype(np.int32).reshape(-1, 2)

    def bins(self, enthalpy, vmin):
        """Bin of ``enthalpy`` in the window that starts at ``vmin``: the exact floor division of the sampling step,
        held inside 0 .. Lw - 1 (the clamp changes no index of an in-window enthalpy)."""
        q = np.floor_divide(np.asarray(enthalpy, dtype=np.float64) - vmin, self.bin_size)
        return np.clip(q, 0, self.Lw - 1).astype(np.int64)

    def decide(self, enthalpy, entropy, estimator_of, move, attempt, log_u=None, record=True, pairs=None):
        """One attempt of ``move`` (or of the disjoint ``pairs`` given outright, not recorded) on the host: enthalpy (R,)
        by walker, entropy (R, Lw) by ESTIMATOR and the walker -> estimator map in; returns dict(pairs, in_window,
        exponent, accept, estimator_of (new)).  The definition the
        device kernel is tested against: three roundings of the exponent in the order written in the class docstring."""
        enthalpy = np.asarray(enthalpy, dtype=np.float64)
        S = np.asarray(entropy, dtype=np.float64).reshape(self.R, self.Lw)
        estimator_of = np.asarray(estimator_of, dtype=np.int64)
        record = record and pairs is None
        pairs = self.pairs(move) if pairs is None else np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        s, t, a, b = self._holders(estimator_of, pairs)
        Ea, Eb = enthalpy[a], enthalpy[b]
        in_window = (Ea >= self.vmin[t]) & (Ea < self.vmax[t]) & (Eb >= self.vmin[s]) & (Eb < self.vmax[s])
        iaa, iab = self.bins(Ea, self.vmin[s]), self.bins(Eb, self.vmin[s])
        iba, ibb = self.bins(Ea, self.vmin[t]), self.bins(Eb, self.vmin[t])
        ex = ((S[s, iaa] - S[s, iab]) + S[t, ibb]) - S[t, iba]
        if log_u is None:
            log_u = self.log_u(attempt, len(pairs))
        log_u = np.asarray(log_u, dtype=np.float64)
        accept = in_window & ((ex >= 0) | (log_u < ex))
        if record:
            self.record(move, accept)
        return dict(pairs=pairs, in_window=in_window, exponent=ex, accept=accept,
                    estimator_of=self._swapped(estimator_of, s, t, a, b, accept))

    def levels(self):
        """Lower edges of the L global bins."""
        return self.min_enthalpy + np.arange(self.L) * self.bin_size

    def join(self, entropy):
        """One ln g over the global bin grid from the estimators' entropies (R, Lw), estimator order.  Per copy index:
        window after window is shifted by the mean difference over the bins that it and the part already joined have
        both visited (S > 0), and bins covered by several windows take the mean of the shifted values of the windows
        that visited them.  The copies are brought to copy 0's constant the same way and averaged.  Returns
        (ln g (L,), per-copy ln g (copies, L), visited (L,) bool); unvisited bins hold 0."""
        S = np.asarray(entropy, dtype=np.float64).reshape(self.n_windows, self.copies, self.Lw)
        per_copy = np.zeros((self.copies, self.L))
        seen = np.zeros((self.copies, self.L), dtype=bool)
        for i in range(self.copies):
            total, count = np.zeros(self.L), np.zeros(self.L)
            for k in range(self.n_windows):
                piece, sl = S[k, i], slice(k * self.Ls, k * self.Ls + self.Lw)
                vis = piece > 0
                if not vis.any():
                    continue
                have = count[sl] > 0
                shift = 0.0
                if have.any():
                    common = have & vis
                    if not common.any():
                        raise ValueError(f"copy {i}: window {k} shares no visited bin with the windows below it")
                    shift = float(np.mean((total[sl][common] / count[sl][common]) - piece[common]))
                total[sl] += np.where(vis, piece + shift, 0.0)
                count[sl] += vis
            seen[i] = count > 0
            per_copy[i, seen[i]] = total[seen[i]] / count[seen[i]]
        total, count = np.zeros(self.L), np.zeros(self.L)
        for i in range(self.copies):
            if not seen[i].any():
                continue
            have = count > 0
            shift = 0.0
            if have.any():
                common = have & seen[i]
                if not common.any():
                    raise ValueError(f"copy {i} shares no visited bin with the copies before it")
                shift = float(np.mean(total[common] / count[common] - per_copy[i, common]))
            per_copy[i, seen[i]] += shift
            total += np.where(seen[i], per_copy[i], 0.0)
            count += seen[i]
        visited = count > 0
        ln_g = np.zeros(self.L)
        ln_g[visited] = total[visited] / count[visited]
        return ln_g, per_copy, visited

    def seed(self, engine, occ0, chunk, max_chunks, temperature=None):
        """Start occupancies (R, N), one inside every estimator's window.  ``engine`` is a Wang-Landau handle of R
        walkers that still has the GLOBAL window it was created with (a second, short-lived handle: plain Wang-Landau
        walks the whole range); it is started from ``occ0`` ((N,) or (R, N)) and run in chunks of ``chunk`` steps.
        After every chunk each estimator that has none yet takes the occupancy of a walker whose enthalpy lies in its
        window (walkers not used before first).  Raises, naming the windows never reached, after ``max_chunks``."""
        if engine.R != self.R:
            raise ValueError(f"the windows have {self.R} estimators, the engine {engine.R} walkers")
        occ0 = np.asarray(occ0)
        occ0 = np.broadcast_to(occ0, (self.R, occ0.shape[-1]))
        engine.set_state(occ0, np.arange(self.R, dtype=np.uint64) + np.uint64(self.philox_seed * self.R + 1), temperature)
        out = np.zeros((self.R, occ0.shape[-1]), dtype=np.int32)
        missing = np.ones(self.R, dtype=bool)
        used = np.zeros(self.R, dtype=bool)
        for c in range(int(max_chunks) + 1):
            if c:
                engine.run(int(chunk), sync=True)
            st = engine.get_state()
            H = st["enthalpy"]
            for e in np.flatnonzero(missing):
                inside = (H >= self.vmin[e]) & (H < self.vmax[e])
                cand = np.flatnonzero(inside & ~used)
                if not len(cand):
                    cand = np.flatnonzero(inside)
                if len(cand):
                    out[e] = st["occupancy"][cand[0]]
                    used[cand[0]] = True
                    missing[e] = False
            if not missing.any():
                return out
        never = sorted(set(int(k) for k in self.window_of[missing]))
        raise RuntimeError(f"no walker reached window(s) {never} in {int(max_chunks)} chunks of {int(chunk)} steps: "
                           + ", ".join(f"[{self.window_min[k]:.6g}, {self.window_max[k]:.6g})" for k in never))


def run_wl_exchange(engine, wx, n_exchanges, steps_between, host_decide=False, history=None, sync_every=None,
                    final_mod_factor=None):
    """Alternate ``steps_between`` Wang-Landau steps on every walker with one exchange attempt between the windows of
    ``wx``, alternating its even and odd move.  ``engine`` holds ``wx.R`` walkers with ``set_wl_windows(wx.vmin,
    wx.vmax)`` in force and their state loaded.  Default: the attempt is decided and applied on the device
    (``Engine.exchange_wl``: the walkers swap estimators), nothing but the accept flags comes back.
    ``host_decide=True``: state and entropies are read back, ``wx.decide`` takes the decisions, and an accepted pair
    swaps its two CONFIGURATIONS through ``set_state(..., reset_aux=False)`` -- the estimators stay with their walkers;
    the cross-check of the device path, and what it is timed against.  ``history``: a list that receives the walker
    (host: configuration) -> estimator map after every attempt.
    ``sync_every=k``: after every k-th attempt the copies of every window are merged when all of them are flat
    (``wx.sync_attempt``: on the device, with ``host_decide=True`` through ``get_wl`` / ``wx.synchronise`` / ``set_wl``);
    the handle must have been created with check period 0, so that no copy leaves its stage alone.
    ``final_mod_factor``: the loop ends after the merge attempt at which every window's factor is at or below it."""
    if engine.R != wx.R:
        raise ValueError(f"the windows have {wx.R} estimators, the engine {engine.R} walkers")
    if final_mod_factor is not None and sync_every is None:
        raise ValueError("final_mod_factor needs sync_every: the windows' factors are those of the merge attempts")
    if sync_every is not None and int(sync_every) < 1:
        raise ValueError("sync_every must be at least 1")
    identity = np.arange(wx.R)
    if host_decide:
        wx.estimator_of = np.asarray(wx.estimator_of).copy()  # configuration -> estimator (= the walker it sits on)
    for i in range(int(n_exchanges)):
        engine.run(steps_between)
        if host_decide:
            move = wx.move_of(wx.calls)
            pairs = wx.pairs(move)
            st = engine.get_state()
            res = wx.decide(st["enthalpy"], engine.get_wl()["entropy"], identity, move, wx.calls)
            if res["accept"].any():
                occ = st["occupancy"].copy()
                s, t = pairs[res["accept"], 0], pairs[res["accept"], 1]
                occ[s], occ[t] = st["occupancy"][t], st["occupancy"][s]
                engine.set_state(occ, None, None, reset_aux=False)
                conf_at = np.empty(wx.R, dtype=np.int64)
                conf_at[wx.estimator_of] = identity
                wx.estimator_of[conf_at[s]], wx.estimator_of[conf_at[t]] = t, s
            wx.calls += 1
        else:
            wx.attempt(engine)
            if history is not None:
                wx.estimator_of = engine.wl_windows()[2].astype(np.int64)
        if history is not None:
            history.append(np.array(wx.estimator_of))
        if sync_every is not None and (i + 1) % int(sync_every) == 0:
            wx.sync_attempt(engine, host=host_decide)
            if final_mod_factor is not None and wx.converged(final_mod_factor):
                break
    if not host_decide:
        wx.estimator_of = engine.wl_windows()[2].astype(np.int64)
    return wx


# ---- population annealing: reweight, resample and clone a population of walkers (smolmc_anneal_resample) ------------
class PopulationAnnealing:
    """Bookkeeping and definition of population annealing (Hukushima & Iba 2003; Machta, PRE 82, 026704) in one handle.

    ``temperatures`` (K + 1,) is the schedule T_0 .. T_K; the R walkers of a handle are ``populations`` contiguous
    blocks of n = R / populations walkers that are annealed independently.  Step k takes every population from
    beta = 1 / (kB T_k) to beta' = 1 / (kB T_{k+1}), db = beta' - beta of either sign, by a move defined in integers:

        H_ref = min H (db > 0) or max H;   w_j = exp(-(db * (H_j - H_ref)));   q_j = floor(w_j 2^40);   Q = sum q_j
        off = (word * Q) >> 64,  word = uint64(u 2^53) << 11 with u one Philox uniform per population and step
        C_j = q_0 + ... + q_j;   child m (0 <= m < n) descends from the smallest j with n C_j > m Q + off
        every survivor keeps its slot; the k-th slot without a child takes the k-th surplus copy, of the donors
        repeat(arange(n), max(cnt - 1, 0)):  parent[m], and parent[parent[m]] == parent[m]
        ln Q_p = log(Q / (n 2^40)) - db * H_ref

    The sum of ln Q_p over the steps estimates ln Z(beta_K) - ln Z(beta_0).  ``weights`` and ``parent_map`` are the
    definition the device kernels (pop_anneal.hip) are tested against: q up to the last bit of exp, the map exactly.
    ``family[w]`` is the walker of the start population that walker w descends from.

    An adaptive schedule (``PopulationAnnealing.adaptive``) chooses every step from the population itself: the largest
    step towards ``t_end`` whose energy histograms at beta and beta' overlap by a target (Barash et al. 2017), also in
    integers.  For one population, a step db and a target t / 2^32 (0 < t < 2^32):

        s = sum_j min(Q, n q_j) = c Q + n U:  c walkers have n q_j >= Q, U is the sum of the other q_j
        (s / (n Q) = sum_j min(1 / n, q_j / Q): the expected share of distinct survivors of the resampling)
        the step is ok iff s 2^32 >= t n Q

    ``next_temperature`` bisects db between 0 and 1 / (kB T_limit) - beta per population and takes the db of smallest
    magnitude; the step itself is the move above from beta to the beta' of the chosen temperature."""

    SCALE_BITS = 40
    MAX_POPULATION = 1 << 22  # Q < 2^62
    MAX_ITER = 60

    def __init__(self, temperatures, populations=1, seed=0):
        self.temperatures = np.ascontiguousarray(temperatures, dtype=np.float64).reshape(-1)
        self.populations, self.philox_seed = int(populations), int(seed)
        if len(self.temperatures) < 1 or not np.all(self.temperatures > 0) or not np.all(np.isfinite(self.temperatures)):
            raise ValueError("PopulationAnnealing needs a schedule of positive, finite temperatures")
        if self.populations < 1:
            raise ValueError("PopulationAnnealing needs populations >= 1")
        self.betas = 1.0 / (kB * self.temperatures)
        self.calls = 0
        self.log_q = np.zeros((0, self.populations))  # (steps taken, P): ln Q_p of every step
        self.n_families = np.zeros((0, self.populations), dtype=np.int64)
        self.rho_t = np.zeros((0, self.populations))
        self.family = None  # (R,) set by the first step: the identity before it
        self.adaptive_schedule = False  # (PopulationAnnealing.adaptive: the schedule grows as the steps are chosen)
        self._reached = False

    @classmethod
    def adaptive(cls, t_start, t_end, overlap, populations=1, seed=0, n_iter=16, max_steps=1000):
        """A schedule that is chosen as it is taken: from ``t_start`` towards ``t_end`` (cooling or heating) in steps
        whose energy histograms overlap by ``overlap`` in (0, 1), each found with at most ``n_iter`` bisections
        (``next_temperature``).  ``temperatures`` starts as [t_start] and gains every chosen temperature (``append``);
        ``done`` turns true when ``t_end`` is reached, and a step beyond ``max_steps`` raises."""
        pa = cls([t_start], populations=populations, seed=seed)
        pa.t_end = float(t_end)
        if not (pa.t_end > 0.0 and np.isfinite(pa.t_end)):
            raise ValueError("PopulationAnnealing.adaptive needs a positive, finite end temperature")
        pa.overlap_value, pa.overlap_target = float(overlap), cls.target_word(overlap)
        pa.n_iter, pa.max_steps = int(n_iter), int(max_steps)
        if not 1 <= pa.n_iter <= cls.MAX_ITER:
            raise ValueError(f"PopulationAnnealing.adaptive needs n_iter in 1 .. {cls.MAX_ITER}")
        pa.adaptive_schedule = True
        pa.overlaps = np.zeros((0, pa.populations))  # (steps taken, P): the overlap achieved by every step
        pa.forced = []  # per step: the target could not be met at the resolution of the bisection
        return pa

    @staticmethod
    def target_word(overlap):
        """t = int(overlap 2^32) of an overlap in (0, 1); 0 < t < 2^32."""
        t = int(float(overlap) * 2 ** 32)
        if not 0 < t < 2 ** 32:
            raise ValueError(f"the target overlap must lie in (0, 1) and be at least 2^-32: {overlap}")
        return t

    def append(self, temperature, reached, forced=False, overlaps=None):
        """Record the temperature an adaptive schedule chose for its next step (before ``record`` of that step)."""
        self.check_room()
        self.temperatures = np.append(self.temperatures, np.float64(temperature))
        self.betas = 1.0 / (kB * self.temperatures)
        self._reached = bool(reached)
        self.forced.append(bool(forced))
        row = np.full(self.populations, np.nan) if overlaps is None else np.asarray(overlaps, dtype=np.float64).reshape(-1)
        self.overlaps = np.vstack([self.overlaps, row[None]])

    def check_room(self):
        """Raise unless an adaptive schedule may choose a further step."""
        if not self.adaptive_schedule:
            raise ValueError("a fixed schedule takes no further temperatures")
        if self._reached:
            raise ValueError("the adaptive schedule has reached its end temperature")
        if self.n_steps >= self.max_steps:
            raise RuntimeError(f"the adaptive schedule did not reach {self.t_end} K within max_steps = {self.max_steps} steps "
                               f"(now at {self.temperatures[-1]} K)")

    def choose(self, enthalpy):
        """The next temperature of an adaptive schedule from the enthalpies (R,) on the host: ``next_temperature``,
        recorded with ``append``.  Returns it."""
        H = np.asarray(enthalpy, dtype=np.float64).reshape(self.populations, -1)
        t_new, reached, forced, _ = self.next_temperature(H, self.betas[-1], self.t_end, self.overlap_target, self.n_iter)
        self.append(t_new, reached, forced)
        return t_new

    @property
    def n_steps(self):
        """Resampling steps of the schedule (of an adaptive one: those chosen so far)."""
        return len(self.temperatures) - 1

    @property
    def done(self):
        """Every step of the schedule is taken (an adaptive one: its end temperature is reached and that step taken)."""
        return self.calls >= self.n_steps and (self._reached or not self.adaptive_schedule)

    def offset_words(self, attempt):
        """The uint64 offset word of every population at step ``attempt`` (a pure function of the seed and the step)."""
        u = _philox_uniforms(self.philox_seed, attempt, self.populations)
        return (u * 2.0 ** 53).astype(np.uint64) << np.uint64(11)

    @classmethod
    def weights(cls, enthalpy, beta_old, beta_new):
        """(q (n,) uint64, Q int, H_ref) of one population."""
        return cls.weights_of_step(enthalpy, np.float64(beta_new) - np.float64(beta_old))

    @classmethod
    def weights_of_step(cls, enthalpy, db):
        """(q (n,) uint64, Q int, H_ref) of one population for a step ``db`` of beta."""
        H = np.asarray(enthalpy, dtype=np.float64).reshape(-1)
        db = np.float64(db)
        href = H.min() if db > 0 else H.max()
        w = np.exp(-(db * (H - href)))
        q = np.floor(w * 2.0 ** cls.SCALE_BITS).astype(np.uint64)
        return q, int(q.sum(dtype=np.uint64)), float(href)  # (Q < 2^62: the uint64 sum is exact)

    # ---- the adaptive step: the overlap of the energy histograms at beta and beta + db, in integers -----------------
    @staticmethod
    def overlap_terms(q):
        """(n, Q, c, U) of the weights of one population: c walkers with n q_j >= Q, U the sum of the other q_j, so that
        s = sum_j min(Q, n q_j) = c Q + n U.  (n q_j <= 2^62: uint64 holds it.)"""
        q = np.asarray(q, dtype=np.uint64).reshape(-1)
        n, Q = len(q), int(q.sum(dtype=np.uint64))
        big = q * np.uint64(n) >= np.uint64(Q)
        return n, Q, int(big.sum()), int(q[~big].sum(dtype=np.uint64))

    @classmethod
    def overlap(cls, q):
        """s / (n Q) = sum_j min(1 / n, q_j / Q) as a float, for reporting (the decisions are ``overlap_ok``'s)."""
        n, Q, c, U = cls.overlap_terms(q)
        return (c * Q + n * U) / (n * Q)

    @classmethod
    def overlap_ok(cls, enthalpy, db, target, margin=False):
        """Whether the step ``db`` keeps the overlap of one population at ``target`` / 2^32 or above: s 2^32 >= t n Q.
        ``margin=True``: (ok, |s 2^32 - t n Q| >> 32) -- how far the decision is from turning."""
        target = int(target)
        if not 0 < target < 2 ** 32:
            raise ValueError("the overlap target is a word t with 0 < t < 2^32 (the target is t / 2^32)")
        q, _, _ = cls.weights_of_step(enthalpy, db)
        n, Q, c, U = cls.overlap_terms(q)
        lhs, rhs = (c * Q + n * U) << 32, target * n * Q
        return (lhs >= rhs, abs(lhs - rhs) >> 32) if margin else lhs >= rhs

    @classmethod
    def search_step(cls, enthalpy, full_step, target, n_iter):
        """The step of one population towards ``full_step`` = beta_limit - beta: (db, reached, forced, smallest margin,
        lo, hi).  The whole step if it is ok; else the bisection of [0, full_step] that keeps ok(lo) and not ok(hi),
        at most ``n_iter`` halvings, db = lo -- or hi where lo is still 0 (forced: the schedule moves all the same)."""
        D = np.float64(full_step)
        ok, margin = cls.overlap_ok(enthalpy, D, target, margin=True)
        if ok:
            return D, True, False, margin, D, D
        lo, hi = np.float64(0.0), D
        for _ in range(int(n_iter)):
            mid = np.float64(0.5) * (lo + hi)
            if mid == lo or mid == hi:
                break
            ok, m = cls.overlap_ok(enthalpy, mid, target, margin=True)
            margin = min(margin, m)
            if ok:
                lo = mid
            else:
                hi = mid
        forced = lo == 0.0
        return (hi if forced else lo), False, bool(forced), margin, lo, hi

    @classmethod
    def next_temperature(cls, enthalpy, beta, temperature_limit, target, n_iter=16):
        """One choice for all populations, enthalpy (P, n): (T', reached, forced, smallest margin of all decisions).
        db is the population step (``search_step``) of smallest magnitude (the first of equals), ``reached`` holds iff
        every population reached the limit, ``forced`` iff the chosen one was forced.  T' = T_limit when reached, else
        1 / (kB (beta + db)), every operation rounded on its own; beta' is 1 / (kB T') as everywhere."""
        H = np.asarray(enthalpy, dtype=np.float64)
        H = H.reshape(1, -1) if H.ndim == 1 else H
        if not 1 <= int(n_iter) <= cls.MAX_ITER:
            raise ValueError(f"n_iter must lie in 1 .. {cls.MAX_ITER}")
        T_limit, beta = np.float64(temperature_limit), np.float64(beta)
        if not (T_limit > 0.0 and np.isfinite(T_limit)):
            raise ValueError("the temperature limit must be positive and finite")
        D = np.float64(1.0) / (np.float64(kB) * T_limit) - beta
        db, reached, forced, margin = None, True, False, None
        for p in range(len(H)):
            db_p, reached_p, forced_p, margin_p, _, _ = cls.search_step(H[p], D, target, n_iter)
            reached = reached and reached_p
            margin = margin_p if margin is None else min(margin, margin_p)
            if db is None or abs(db_p) < abs(db):
                db, forced = db_p, forced_p
        T_new = T_limit if reached else np.float64(1.0) / (np.float64(kB) * (beta + db))
        return float(T_new), bool(reached), bool(forced), int(margin)

    @staticmethod
    def children(q, word):
        """cnt (n,) int64: the children of every walker of one population under systematic resampling."""
        q = [int(x) for x in np.asarray(q).reshape(-1)]
        n, Q = len(q), sum(q)
        if Q <= 0:
            raise ValueError("the weights of a population sum to zero")
        off = (int(word) * Q) >> 64
        C = np.cumsum(np.asarray(q, dtype=np.uint64), dtype=np.uint64)  # (Q < 2^62: exact)
        # n C_j > m Q + off  <=>  C_j > (m Q + off) // n, both sides integers: the first j is a sorted search
        thr = np.array([(m * Q + off) // n for m in range(n)], dtype=np.uint64)
        anc = np.searchsorted(C, thr, side="right")
        return np.bincount(anc, minlength=n).astype(np.int64)

    @classmethod
    def parent_map(cls, q, word):
        """parent (n,) int64 of one population: slot m takes the state of slot parent[m]."""
        cnt = cls.children(q, word)
        n = len(cnt)
        parent = np.arange(n)
        parent[cnt == 0] = np.repeat(np.arange(n), np.maximum(cnt - 1, 0))
        return parent

    def log_q_of(self, qsum, href, beta_old, beta_new, n):
        """ln Q_p of a step from the sum of the weights and H_ref of every population."""
        db = np.float64(beta_new) - np.float64(beta_old)
        ratio = np.array([int(Q) / (n * 2.0 ** self.SCALE_BITS) for Q in np.asarray(qsum).reshape(-1)])
        return np.log(ratio) - db * np.asarray(href, dtype=np.float64).reshape(-1)

    def record(self, parent, qsum, href, attempt):
        """Take a step's outcome into the running sums and the lineage: ``parent`` (R,) slot numbers, ``qsum`` and
        ``href`` (P,).  Returns ln Q_p (P,)."""
        parent = np.asarray(parent, dtype=np.int64).reshape(-1)
        P, R = self.populations, len(parent)
        n = R // P
        lq = self.log_q_of(qsum, href, self.betas[attempt], self.betas[attempt + 1], n)
        if self.family is None:
            self.family = np.arange(R)
        self.family = self.family[parent]
        fam = self.family.reshape(P, n)
        nf, rho = np.zeros(P, dtype=np.int64), np.zeros(P)
        for p in range(P):
            _, sizes = np.unique(fam[p], return_counts=True)
            nf[p], rho[p] = len(sizes), float(np.sum(sizes.astype(np.float64) ** 2)) / n  # rho_t = n sum f_i^2
        self.log_q = np.vstack([self.log_q, lq[None]])
        self.n_families = np.vstack([self.n_families, nf[None]])
        self.rho_t = np.vstack([self.rho_t, rho[None]])
        self.calls = int(attempt) + 1
        return lq

    def step(self, enthalpy, attempt, record=True):
        """The whole move of step ``attempt`` over all populations on the host: enthalpy (R,) in; returns dict(parent
        (R,) slot numbers, q (R,) uint64, qsum (P,) uint64, href (P,), log_q (P,))."""
        H = np.asarray(enthalpy, dtype=np.float64).reshape(-1)
        P, R = self.populations, len(H)
        if R % P or R // P > self.MAX_POPULATION:
            raise ValueError(f"{P} populations do not divide the {R} walkers into blocks of at most 2^22")
        n = R // P
        b0, b1 = self.betas[attempt], self.betas[attempt + 1]
        words = self.offset_words(attempt)
        parent, q = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.uint64)
        qsum, href = np.zeros(P, dtype=np.uint64), np.zeros(P)
        for p in range(P):
            sl = slice(p * n, (p + 1) * n)
            q[sl], Q, href[p] = self.weights(H[sl], b0, b1)
            qsum[p] = Q
            parent[sl] = p * n + self.parent_map(q[sl], words[p])
        lq = self.record(parent, qsum, href, attempt) if record else self.log_q_of(qsum, href, b0, b1, n)
        return dict(parent=parent, q=q, qsum=qsum, href=href, log_q=lq)

    def log_partition_ratio(self):
        """(P,): the sum of ln Q_p over the steps taken, the estimate of ln Z(beta_now) - ln Z(beta_0)."""
        return self.log_q.sum(axis=0)

    def free_energy(self, log_z0=0.0):
        """(steps taken, P): -ln Z(beta_k) / beta_k along the schedule, k = 1 .., with ln Z(beta_0) = ``log_z0``."""
        k = len(self.log_q)
        return -(log_z0 + np.cumsum(self.log_q, axis=0)) / self.betas[1:k + 1, None]

    def population_weights(self):
        """(P,) normalised exp(sum ln Q_p): the weight of a population in an average over populations."""
        lpr = self.log_partition_ratio()
        w = np.exp(lpr - lpr.max())
        return w / w.sum()

    def combine(self, values):
        """The exp(sum ln Q)-weighted average across populations of per-population ``values`` (P, ...)."""
        v = np.asarray(values, dtype=np.float64)
        return np.tensordot(self.population_weights(), v, axes=(0, 0))

    def combined_log_partition_ratio(self):
        """ln of the mean over populations of exp(sum ln Q_p): the populations' joint estimate of ln Z / Z_0."""
        lpr = self.log_partition_ratio()
        return float(lpr.max() + np.log(np.mean(np.exp(lpr - lpr.max()))))


def run_population_annealing(engine, pa, steps_per_temperature, host_decide=False, history=None):
    """Anneal the walkers of ``engine`` along ``pa.temperatures``: at every step of the schedule the populations are
    reweighted, resampled and cloned, then every walker runs ``steps_per_temperature`` Metropolis steps at the new
    temperature.  ``engine`` holds R walkers (R a multiple of ``pa.populations``) with their state loaded at
    ``pa.temperatures[0]``.  Default: the move runs on the device (``Engine.anneal_resample``), only the map, the
    weights' sums and H_ref come back.  ``host_decide=True`` (also on ``oracle.OracleMC``): the state is read back,
    ``pa.step`` decides, and the clones go through ``set_state(occupancy[parent], reset_aux=False)`` -- enthalpies are
    then evaluated afresh, so the two paths agree statistically, not bit for bit.  ``history``: a list that receives
    the parent map of every step."""
    R, P = int(engine.R), pa.populations
    if R % P:
        raise ValueError(f"{P} populations do not divide the engine's {R} walkers")
    if pa.adaptive_schedule:
        return _run_adaptive_annealing(engine, pa, steps_per_temperature, host_decide, history)
    for k in range(pa.calls, pa.n_steps):
        t_new = pa.temperatures[k + 1]
        if host_decide:
            st = engine.get_state()
            res = pa.step(st["enthalpy"], k)
            parent = res["parent"]
            engine.set_state(st["occupancy"][parent], np.zeros(R, dtype=np.uint64), np.full(R, t_new), reset_aux=False)
            engine.set_counters(st["n_steps"], st["n_accepted"])
        else:
            res = engine.anneal_resample(np.full(P, t_new), pa.offset_words(k), npop=P)
            parent = res["parent"]
            pa.record(parent, res["qsum"], res["href"], k)
        if history is not None:
            history.append(np.array(parent))
        engine.run(int(steps_per_temperature))
    return pa


def _run_adaptive_annealing(engine, pa, steps_per_temperature, host_decide, history):
    """``run_population_annealing`` of an adaptive schedule: every step is chosen from the population (on the device by
    ``Engine.anneal_adaptive``, with ``host_decide`` by ``pa.choose`` on the enthalpies read back) until the end
    temperature is reached."""
    R, P = int(engine.R), pa.populations
    n = R // P
    while not pa.done:
        k = pa.calls
        if host_decide:
            st = engine.get_state()
            if pa.n_steps == k:  # (else: chosen already, the step itself is still to take)
                pa.choose(st["enthalpy"])
            t_new = pa.temperatures[k + 1]
            res = pa.step(st["enthalpy"], k)
            parent = res["parent"]
            engine.set_state(st["occupancy"][parent], np.zeros(R, dtype=np.uint64), np.full(R, t_new), reset_aux=False)
            engine.set_counters(st["n_steps"], st["n_accepted"])
        else:
            if pa.n_steps != k:
                raise ValueError("the device chooses and takes a step in one call: this schedule has a chosen step that was not taken")
            pa.check_room()
            res = engine.anneal_adaptive(pa.t_end, pa.overlap_value, pa.offset_words(k), npop=P, n_iter=pa.n_iter)
            parent = res["parent"]
            pa.append(res["temperature"], res["reached"], res["forced"])
            pa.record(parent, res["qsum"], res["href"], k)
        pa.overlaps[k] = [pa.overlap(res["q"][p * n:(p + 1) * n]) for p in range(P)]
        if history is not None:
            history.append(np.array(parent))
        engine.run(int(steps_per_temperature))
    return pa
