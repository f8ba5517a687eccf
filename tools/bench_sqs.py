"""Throughput of the distance-objective kernel (mc_dist_kernel): swap steps per second of a batched SQS search.

Two shapes, one JSON line each: the binary fcc model {2: 7.0, 3: 5.0} (9 features) and the ternary fcc model
{2: 7.0, 3: 5.0, 4: 4.2} (48 features), both in the 64-site diag(4,4,4) cell, random-alloy target.  Kernel time
from the engine's device events over several launches after a warm-up; the wall time of the full default anneal
(StochasticSQSGenerator.generate: linspace(5, 0.01, 20), --anneal-steps steps per temperature).

    python tools/bench_sqs.py [--walkers 4096] [--steps 2000] [--launches 5] [--anneal-steps 1000]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smol_amd import capi, synth  # noqa: E402
from smol_amd import sqs  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402

SHAPES = {
    "binary": (dict(), {2: 7.0, 3: 5.0}),
    "ternary": (dict(nspecies=3), {2: 7.0, 3: 5.0, 4: 4.2}),
}


def bench(shape, R, steps, launches, anneal_steps):
    kw, cut = SHAPES[shape]
    model = synth.build_cluster_model(synth.fcc_prim(**kw), cut)
    mat = np.diag([4, 4, 4])
    sc, tab = sqs.distance_tables(model, mat, capi.FEATURES_CORRELATIONS)
    spec = sqs.distance_spec(model, capi.FEATURES_CORRELATIONS)
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP), distance=spec)
    rng = np.random.default_rng(0)
    occ = np.stack([sqs.random_ordered_occupancy(sc, rng) for _ in range(R)])
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(1), 1.0)
    eng.run(steps, sync=True)  # warm-up
    ms = []
    for _ in range(launches):
        eng.run(steps, sync=True)
        ms.append(eng.last_kernel_ms())
    kms = float(np.median(ms))
    info = eng.kernel_info()
    eng.close()
    gen = sqs.StochasticSQSGenerator(model, 64, supercell_matrices=[mat], nwalkers=R, seeds=1)
    t0 = time.perf_counter()
    gen.generate(anneal_steps)
    best = gen.get_best_sqs(1)[0]
    wall = time.perf_counter() - t0
    return dict(tool="bench_sqs", shape=shape, features=int(spec.struct.n_features), sites=int(sc.num_sites),
                walkers=R, steps_per_launch=steps, kernel_ms=round(kms, 4),
                swap_steps_per_s=float(f"{R * steps / (kms * 1e-3):.4g}"), kernel_info=info,
                anneal=dict(temperatures=20, steps_per_temperature=anneal_steps, wall_s=round(wall, 3),
                            best_score=round(float(best.score), 6)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--anneal-steps", type=int, default=1000)
    ap.add_argument("--shapes", default="binary,ternary")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        print(json.dumps(bench(shape, a.walkers, a.steps, a.launches, a.anneal_steps)), flush=True)


if __name__ == "__main__":
    main()
