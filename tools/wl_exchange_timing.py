#!/usr/bin/env python3
"""Replica-exchange Wang-Landau on config 15 (config 4's Hamiltonian and global window as 16 windows x 64 copies, DESIGN
4.13), three measurements, one JSON line each into profiles/wl_windows_timing.jsonl:

  rate        steps/s (kernel time, HIP events) of config 15 against config 4 at the same walker count, launches
              alternating between the two handles; LDS bytes per workgroup from kernel_info.  (Config 4's kernels in
              this library are the parent commit's byte for byte, profiles/wl_windows_codeobj_diff.txt: no second
              library is needed for the comparison.)
  exchange    ms per exchange attempt decided and applied on the device (Engine.exchange_wl) against ms per attempt of
              run_wl_exchange(host_decide=True)'s body (state and entropies read back, WLWindows.decide, occupancies moved
              through set_state).  Wall clock from a synchronised stream to a synchronised stream.
  flatness    steps per walker until every estimator (config 15) / every walker (config 4) has passed --checks flatness
              checks (mod_factor <= 2^-checks), in rounds of --round steps with an exchange after each round.

python tools/wl_exchange_timing.py [--replicas 1024] [--what rate,exchange,flatness] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_configs import windowed_engine  # noqa: E402
from smol_amd import capi, parallel, workloads  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402


def stats_ms(samples):
    a = np.asarray(samples) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=len(a))


def build(config, replicas, mc):
    kw = dict(count=replicas, mc=mc)
    wl = workloads.BUILDERS[config](**kw)
    probe = Engine(wl.tables, capi.make_config(1))
    h0 = float(probe.natural_parameters @ probe.eval_full(wl.occupancy[:1])[0])
    probe.close()
    return workloads.BUILDERS[config](h0=h0, **kw)


def plain_engine(wl):
    eng = Engine(wl.tables, wl.make_config())
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    return eng


def lds_of(info):
    return int(next(tok.split("=")[1] for tok in info.split() if tok.startswith("lds=")))


def measure_rate(args, emit):
    w4, w15 = build(4, args.replicas, args.mc), build(15, args.replicas, args.mc)
    e4 = plain_engine(w4)
    e15, wx, seed_steps = windowed_engine(w15)
    for e in (e4, e15):
        e.run(args.mc, sync=True)
    ms = {4: [], 15: []}
    for _ in range(args.reps):  # launches alternating
        for key, e in ((4, e4), (15, e15)):
            e.run(args.mc, sync=True)
            ms[key].append(e.last_kernel_ms() * 1e-3)
    out = dict(what="rate", walkers=args.replicas, mc_steps_per_launch=args.mc, reps=args.reps, seed_steps_per_walker=seed_steps,
               window_bins=wx.Lw, stride_bins=wx.Ls)
    for key, e in ((4, e4), (15, e15)):
        t = float(np.median(ms[key]))
        info = e.kernel_info()
        out[f"config{key}"] = dict(kernel=info, lds_bytes_per_workgroup=lds_of(info), kernel_time=stats_ms(ms[key]),
                                   mc_steps_per_s=args.replicas * args.mc / t)
    out["config15_over_config4"] = out["config15"]["mc_steps_per_s"] / out["config4"]["mc_steps_per_s"]
    e4.close()
    e15.close()
    emit(out)


def measure_exchange(args, emit):
    w15 = build(15, args.replicas, args.mc)
    eng, wx, _ = windowed_engine(w15)
    eng.run(20000, sync=True)
    attempt, dev, dev_stats, host, acc, att = 0, [], [], [], 0, 0
    for i in range(args.warmup + args.reps):
        eng.run(1000, sync=True)
        pairs = wx.pairs(wx.move_of(attempt))
        log_u = wx.log_u(attempt, len(pairs))
        t0 = time.perf_counter()
        eng.exchange_wl(pairs, log_u)
        eng.sync()
        t1 = time.perf_counter()
        eng.run(1000, sync=True)
        stats = np.zeros((len(pairs), 2), dtype=np.int64)
        t2 = time.perf_counter()
        eng.exchange_wl(pairs, log_u, stats)
        t3 = time.perf_counter()
        attempt += 1
        if i >= args.warmup:
            dev.append(t1 - t0)
            dev_stats.append(t3 - t2)
            acc, att = acc + int(stats[:, 1].sum()), att + len(pairs)
    # the host path: what run_wl_exchange(host_decide=True) does per attempt (the estimators stay with their walkers, so
    # the windows are reset to the identity map first: every walker is re-seated in the window it holds)
    vmin, vmax, est = eng.wl_windows()
    st = eng.get_state()
    order = np.argsort(est)  # walker that holds estimator e
    eng.set_wl_windows(wx.vmin, wx.vmax)
    eng.set_state(st["occupancy"][order], w15.seeds, w15.temperature, reset_aux=False)
    identity = np.arange(wx.R)
    for i in range(max(2, args.warmup // 4) + max(5, args.reps // 4)):
        eng.run(1000, sync=True)
        move = wx.move_of(attempt)
        pairs = wx.pairs(move)
        t0 = time.perf_counter()
        st = eng.get_state()
        res = wx.decide(st["enthalpy"], eng.get_wl()["entropy"], identity, move, attempt, record=False)
        if res["accept"].any():
            occ = st["occupancy"].copy()
            s, t = pairs[res["accept"], 0], pairs[res["accept"], 1]
            occ[s], occ[t] = st["occupancy"][t], st["occupancy"][s]
            eng.set_state(occ, None, None, reset_aux=False)
        eng.sync()
        t1 = time.perf_counter()
        attempt += 1
        if i >= max(2, args.warmup // 4):
            host.append(t1 - t0)
    out = dict(what="exchange", walkers=args.replicas, kernel=eng.kernel_info(), pairs_per_attempt=int(len(wx.pairs(0))),
               device_attempt=stats_ms(dev), device_attempt_with_stats=stats_ms(dev_stats), acceptance=acc / max(att, 1),
               host_attempt=stats_ms(host))
    out["host_over_device"] = out["host_attempt"]["median_ms"] / out["device_attempt"]["median_ms"]
    eng.close()
    emit(out)


def measure_flatness(args, emit):
    target = 2.0 ** -args.checks
    out = dict(what="flatness", walkers=args.replicas, checks=args.checks, round_steps=args.round, max_rounds=args.max_rounds)
    w15 = build(15, args.replicas, args.mc)
    eng, wx, seed_steps = windowed_engine(w15)
    steps = None
    for k in range(args.max_rounds):
        parallel.run_wl_exchange(eng, wx, 1, args.round)
        if (eng.get_wl()["mod_factor"] <= target).all():
            steps = (k + 1) * args.round
            break
    out["config15"] = dict(steps_per_walker=steps, seed_steps_per_walker=seed_steps, exchange_acceptance=wx.acceptance,
                           slowest_mod_factor=float(eng.get_wl()["mod_factor"].max()))
    eng.close()
    e4 = plain_engine(build(4, args.replicas, args.mc))
    steps = None
    for k in range(args.max_rounds):
        e4.run(args.round, sync=True)
        if (e4.get_wl()["mod_factor"] <= target).all():
            steps = (k + 1) * args.round
            break
    out["config4"] = dict(steps_per_walker=steps, slowest_mod_factor=float(e4.get_wl()["mod_factor"].max()))
    e4.close()
    emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1024)
    ap.add_argument("--mc", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--checks", type=int, default=10)
    ap.add_argument("--round", type=int, default=20000)
    ap.add_argument("--max-rounds", type=int, default=200)
    ap.add_argument("--what", default="rate,exchange")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wl_windows_timing.jsonl"))
    args = ap.parse_args()

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")

    for what in args.what.split(","):
        dict(rate=measure_rate, exchange=measure_exchange, flatness=measure_flatness)[what](args, emit)


if __name__ == "__main__":
    main()
