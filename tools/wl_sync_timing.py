#!/usr/bin/env python3
"""The merge of a window's copies (smolmc_wl_synchronise) on config 15 -- 16 windows x 64 copies -- created
with check period 0; one JSON line per measurement into profiles/wl_sync_timing.jsonl:

  sync        ms per merge attempt on the device (Engine.wl_synchronise) without and with the status fetched, against ms
              per attempt of the host route (get_wl, WLWindows.synchronise, set_wl), and the bytes either moves.  Wall
              clock from a synchronised stream to a synchronised stream, device and host attempts alternating.
  converge    steps per walker until every window's factor is <= 2^-checks with merging (an exchange and a merge attempt
              after every round), and until every estimator has passed `checks` of its own flatness checks without
              (the handle of tools/wl_exchange_timing.py: check period 1000); at that point, for both, the RMS spread
              of ln g between the copies of a window (each copy minus its mean over the bins all copies visited).

python tools/wl_sync_timing.py [--replicas 1024] [--what sync,converge] [--out ...]"""
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
from smol_amd import parallel  # noqa: E402
from wl_exchange_timing import build, stats_ms  # noqa: E402


def engine(args, check_period):
    wl = build(15, args.replicas, args.mc)
    if check_period is not None:
        wl.config_kwargs = dict(wl.config_kwargs, check_period=check_period)
    return windowed_engine(wl)


def copy_spread(wx, entropy):
    """Per window: RMS over copies and bins of (S_copy - its mean over the common bins) - (the copies' mean of that)."""
    S = np.asarray(entropy).reshape(wx.n_windows, wx.copies, wx.Lw)
    out = []
    for k in range(wx.n_windows):
        common = (S[k] > 0).all(axis=0)
        if common.sum() < 2:
            out.append(float("nan"))
            continue
        d = S[k][:, common]
        d = d - d.mean(axis=1, keepdims=True)
        out.append(float(np.sqrt(np.mean((d - d.mean(axis=0, keepdims=True)) ** 2))))
    return out


def measure_sync(args, emit):
    eng, wx, _ = engine(args, 0)
    eng.run(20000, sync=True)
    dev, dev_fetch, host, merged = [], [], [], 0
    flat, div = eng.config.wl_flatness, eng.config.wl_mod_divisor
    for i in range(args.warmup + args.reps):
        eng.run(1000, sync=True)
        t0 = time.perf_counter()
        eng.wl_synchronise(wx.copies, fetch=False)
        eng.sync()
        t1 = time.perf_counter()
        eng.run(1000, sync=True)
        t2 = time.perf_counter()
        res = eng.wl_synchronise(wx.copies)
        t3 = time.perf_counter()
        eng.run(1000, sync=True)
        t4 = time.perf_counter()
        wl = eng.get_wl()
        ref = wx.synchronise(wl["entropy"], wl["histogram"], wl["mod_factor"], flatness=flat, divisor=div)
        eng.set_wl(entropy=ref["entropy"], histogram=ref["histogram"], mod_factor=ref["mod_factor"])
        eng.sync()
        t5 = time.perf_counter()
        if i >= args.warmup:
            dev.append(t1 - t0)
            dev_fetch.append(t3 - t2)
            host.append(t5 - t4)
            merged += int((res["status"] == 1).sum()) + int((ref["status"] == 1).sum())
    R, L, F = eng.R, eng.L, eng.F
    needed = R * L * 16 + R * 8
    out = dict(what="sync", walkers=R, copies=wx.copies, groups=wx.n_windows, bins=L, kernel=eng.kernel_info(),
               device_attempt=stats_ms(dev), device_attempt_with_status=stats_ms(dev_fetch), host_attempt=stats_ms(host),
               groups_merged_while_timing=merged,
               bytes_device_route=dict(without_status=0, with_status=wx.n_windows * 12),
               bytes_host_route=dict(needed_each_way=needed, moved_down_by_get_wl=needed + R * L * 8 * (1 + F), moved_up_by_set_wl=needed))
    out["host_over_device"] = out["host_attempt"]["median_ms"] / out["device_attempt"]["median_ms"]
    out["host_over_device_with_status"] = out["host_attempt"]["median_ms"] / out["device_attempt_with_status"]["median_ms"]
    eng.close()
    emit(out)


def measure_converge(args, emit):
    target = 2.0 ** -args.checks
    out = dict(what="converge", walkers=args.replicas, checks=args.checks, round_steps=args.round, max_rounds=args.max_rounds)
    eng, wx, seed_steps = engine(args, 0)
    parallel.run_wl_exchange(eng, wx, args.max_rounds, args.round, sync_every=1, final_mod_factor=target)
    spread = copy_spread(wx, eng.get_wl()["entropy"])
    out["merged"] = dict(steps_per_walker=wx.calls * args.round if wx.converged(target) else None, seed_steps_per_walker=seed_steps,
                         exchange_acceptance=wx.acceptance, merges_per_window=wx.merges.tolist(), slowest_mod_factor=float(np.max(wx.mod_factor)),
                         copy_spread_rms_max=float(np.nanmax(spread)), copy_spread_rms_median=float(np.nanmedian(spread)))
    eng.close()
    eng, wx, seed_steps = engine(args, None)
    steps = None
    for k in range(args.max_rounds):
        parallel.run_wl_exchange(eng, wx, 1, args.round)
        if (eng.get_wl()["mod_factor"] <= target).all():
            steps = (k + 1) * args.round
            break
    wl = eng.get_wl()
    spread = copy_spread(wx, wl["entropy"])
    m = wl["mod_factor"]
    out["independent"] = dict(steps_per_walker=steps, seed_steps_per_walker=seed_steps, exchange_acceptance=wx.acceptance,
                              slowest_mod_factor=float(m.max()), fastest_mod_factor=float(m.min()),
                              copy_spread_rms_max=float(np.nanmax(spread)), copy_spread_rms_median=float(np.nanmedian(spread)))
    eng.close()
    emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1024)
    ap.add_argument("--mc", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--checks", type=int, default=10)
    ap.add_argument("--round", type=int, default=20000)
    ap.add_argument("--max-rounds", type=int, default=1500)
    ap.add_argument("--what", default="sync,converge")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wl_sync_timing.jsonl"))
    args = ap.parse_args()

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")

    for what in args.what.split(","):
        dict(sync=measure_sync, converge=measure_converge)[what](args, emit)


if __name__ == "__main__":
    main()
