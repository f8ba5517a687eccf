#!/usr/bin/env python3
"""What labelling the components of every sample costs, on the device against on the host, one JSON line per
member fraction into profiles/connectivity_timing.jsonl:

  shape    config 2 (the headline: R = 4096 walkers of N = 4096 sites, two kinds, swap steps: the composition is kept)
  graph    one graph: the sites that hold species 1, bonded to their twelve nearest neighbours
  fraction the share of the sites that are members, set with the starting occupancies: 0.5, well above the fcc site
           threshold (0.199), and 0.2, at it, where the components are ramified and the passes many
  blocks   --samples samples per block, one sample per sweep (thin_by = N steps per walker); --reps blocks, --warmup first
  device   the block with SMOLMC_SAMPLE_CONNECTIVITY and without the occupancy column: wall time per sample from the
           queueing of the block to the column in hand, the kernel's own time (HIP events around its launch), its share of
           the block's MC kernel time (the events of smolmc_last_kernel_ms), and the passes its rows took
  host     one sample with the occupancy column, fetched packed, then Connectivity.evaluate on --host-rows of its rows (a
           breadth-first search in Python, one thread), scaled to all rows; likewise scipy.sparse.csgraph.connected_components
           where scipy is present (sizes only: no wrapping)

With --gated the graph's bonds carry their tetrahedral gates (a nearest-neighbour bond is open when the two
other corners of one of its two tetrahedra are members too, the 0-TM channel); the default fractions are then 0.45, 0.55
and 0.65, around the threshold near 0.55, and the host path opens the rows before it searches.

With --against LIB the tool measures instead whether the ungated graph pays for the gates: connectivity_kernel of this
build against that of another build of the library (the parent commit's), on the same R rows, launches alternating in one
process, and first the other build against a second handle of itself, which gives the spread of such a comparison.

python tools/connectivity_timing.py [--gated] [--against LIB] [--fractions 0.5,0.2] [--samples 16] [--reps 3] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import capi, workloads  # noqa: E402,F401
from smol_amd import connectivity as cn  # noqa: E402
from smol_amd.connectivity import Connectivity  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402


def stats_ms(samples):
    a = np.asarray(samples) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=len(a))


def scipy_sizes(spec, occ):
    """Largest component per row with scipy, or None without scipy."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return None
    g = spec.graphs[0]
    kinds = spec.kinds_of(occ)
    out = []
    for row, occ_row in zip(kinds, occ):
        member = np.isin(row, g.members)
        on = spec.open_rows(occ_row, 0)
        m = coo_matrix((np.ones(int(on.sum()), np.int8), (g.bonds[on, 0], g.bonds[on, 1])), shape=(len(row), len(row)))
        _, lab = connected_components(m, directed=False)
        out.append(int(np.bincount(lab[member]).max(initial=0)))
    return out


def workload(args):
    kw = dict(count=args.replicas) if args.replicas else {}
    if args.dim:
        kw["dim"] = args.dim
    return workloads.BUILDERS[2](**kw)


def start(wl, fraction):
    """Exactly round(fraction N) sites of species 1 in every row: swaps keep it so."""
    R, N = len(wl.seeds), wl.sc.num_sites
    rng = np.random.default_rng(7)
    n_members = int(round(fraction * N))
    occ = np.zeros((R, N), dtype=np.int32)
    for r in range(R):
        occ[r, rng.permutation(N)[:n_members]] = 1
    return occ


def graph_spec(wl, gated):
    a = float(np.linalg.norm(wl.sc.model.prim.lattice[0]))  # the fcc primitive vectors are nearest-neighbour vectors
    graph = dict(members=[1], cutoff=a * 1.01)
    if gated:
        graph["gate"] = dict(kinds=[1], corners=2, max_blocked=0)
    return Connectivity.from_supercell(wl.sc, [graph])


def other_engine(path, wl):
    """A handle served by another build of the library (one that may lack the newest entry points)."""
    import ctypes as C

    from smol_amd import engine

    lib = C.CDLL(path)
    for name, (res, argtypes) in engine.SYMBOLS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, argtypes
    ours, engine._LIB = engine.load_library(), lib
    try:
        return Engine(wl.tables, wl.make_config())
    finally:
        engine._LIB = ours


def measure_against(fraction, args):
    wl = workload(args)
    spec, occ = graph_spec(wl, False), start(wl, fraction)
    engines = dict(other=other_engine(args.against, wl), other_again=other_engine(args.against, wl), this=Engine(wl.tables, wl.make_config()))
    N = wl.sc.num_sites
    for eng in engines.values():  # the same chain in every handle: the same rows
        eng.set_state(occ, wl.seeds, wl.temperature)
        eng.set_connectivity(spec)
        eng.run(20 * N, sync=True)
    ms = {k: [] for k in engines}
    ref = None
    for rep in range(args.warmup + args.ab_reps):
        for k, eng in engines.items():  # alternating: one launch each, R rows
            stats = eng.connectivity()
            ref = stats if ref is None else ref
            assert np.array_equal(stats, ref), k
            if rep >= args.warmup:
                ms[k].append(eng.connectivity_kernel_ms())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    most, total = engines["this"].connectivity_passes()
    out = dict(what="connectivity_ungated_this_build_against_another", config=2, name=wl.name, against=os.path.basename(os.path.dirname(args.against)),
               walkers=len(wl.seeds), sites=N, member_fraction=fraction, rows_per_launch=len(wl.seeds), launches_each=args.ab_reps,
               kernel_ms=dict(this=med["this"], other=med["other"], other_again=med["other_again"],
                              min=dict((k, float(np.min(v))) for k, v in ms.items())),
               spread_other_against_itself=med["other_again"] / med["other"] - 1.0,
               this_against_other=med["this"] / med["other"] - 1.0, passes_most=int(most), passes_mean=total / len(wl.seeds),
               same_stats=True)
    for eng in engines.values():
        eng.close()
    return out


def measure(fraction, args):
    wl = workload(args)
    eng = Engine(wl.tables, wl.make_config())
    R, N, ns = eng.R, eng.N, args.samples
    thin = N  # one sweep
    eng.set_state(start(wl, fraction), wl.seeds, wl.temperature)
    spec = graph_spec(wl, args.gated)
    eng.set_connectivity(spec)
    eng.run(20 * N, sync=True)

    def device():
        t0 = time.perf_counter()
        eng.run_sampled_async(ns, thin, occupancy=False, connectivity=True)
        smp = eng.fetch_samples()
        t1 = time.perf_counter()
        most, total = eng.connectivity_passes()
        return dict(wall=t1 - t0, mc_ms=eng.last_kernel_ms(), cn_ms=eng.connectivity_kernel_ms(), most=most, mean=total / (ns * R),
                    stats=smp["connectivity"])

    D = [device() for _ in range(args.warmup + args.reps)][args.warmup:]
    # the host path, one sample: the occupancies come back, the definition runs on some of the rows
    t0 = time.perf_counter()
    eng.run_sampled_async(1, thin, occupancy=True, connectivity=True)
    smp = eng.fetch_samples(packed=True)
    t1 = time.perf_counter()
    rows = min(args.host_rows, R)
    sub = np.asarray(smp["occupancy"][0, :rows], dtype=np.int32)
    want = spec.evaluate(sub)[0]
    t2 = time.perf_counter()
    same = bool(np.array_equal(want, smp["connectivity"][0, :rows]))
    sizes = scipy_sizes(spec, sub)
    t3 = time.perf_counter()
    k = np.array([d["cn_ms"] for d in D])
    mc = np.array([d["mc_ms"] for d in D])
    dev = stats_ms([d["wall"] / ns for d in D])
    st = D[-1]["stats"][..., 0, :]
    fetch_ms, eval_ms = (t1 - t0) * 1e3, (t2 - t1) * 1e3 * R / rows
    host_ms = fetch_ms + eval_ms
    out = dict(what="connectivity_gated" if args.gated else "connectivity", config=2, name=wl.name, kernel=eng.kernel_info(), walkers=R, sites=N, member_fraction=fraction,
               n_bonds=int(len(spec.graphs[0].bonds)), channels=eng.connectivity_gates()[1], samples_per_block=ns, thin_by=thin, reps=args.reps,
               device_equals_definition=same, rows_wrapping=float((st[..., cn.WRAP_AXES] != 0).mean()),
               mean_components=float(st[..., cn.N_COMPONENTS].mean()), mean_largest=float(st[..., cn.LARGEST].mean()),
               device=dict(per_sample=dev, connectivity_kernel_ms_per_block=float(np.median(k)),
                           connectivity_kernel_us_per_sample=float(np.median(k)) * 1e3 / ns,
                           mc_kernel_ms_per_block=float(np.median(mc)), connectivity_share_of_mc_kernel=float(np.median(k / mc)),
                           passes_most=int(max(d["most"] for d in D)), passes_mean=float(np.mean([d["mean"] for d in D])),
                           bytes_per_sample=R * 8 * cn.N_STATS),
               host=dict(per_sample_ms=host_ms, ring_and_fetch_ms=fetch_ms, evaluate_ms=eval_ms, rows_evaluated=rows,
                         scaled_to_rows=R, bytes_per_sample=R * N, n=1,
                         scipy_components_ms=None if sizes is None else (t3 - t2) * 1e3 * R / rows,
                         scipy_largest_equal=None if sizes is None else bool(np.array_equal(sizes, want[:, 0, cn.LARGEST]))),
               host_over_device=host_ms / dev["median_ms"])
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fractions", default=None, help="member fractions (default 0.5,0.2; with --gated 0.45,0.55,0.65)")
    ap.add_argument("--gated", action="store_true", help="the bonds carry their tetrahedral gates")
    ap.add_argument("--against", default=None, help="another build of libsmolmc_hip.so: time the ungated kernel of this build against it")
    ap.add_argument("--ab-reps", type=int, default=15, help="launches of each handle with --against")
    ap.add_argument("--replicas", type=int, default=0, help="walkers (default: the configuration's)")
    ap.add_argument("--dim", type=int, default=0, help="supercell size (default: the configuration's)")
    ap.add_argument("--samples", type=int, default=16, help="samples per block")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-rows", type=int, default=32, help="rows of the one host sample the definition is run on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "connectivity_timing.jsonl"))
    args = ap.parse_args()
    fractions = args.fractions or ("0.45,0.55,0.65" if args.gated else "0.5,0.2")
    for f in fractions.split(","):
        line = json.dumps((measure_against if args.against else measure)(float(f), args))
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
