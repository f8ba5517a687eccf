#!/usr/bin/env python3
"""The measured margin of the float32 accept band, one JSON line per (case, construction, scale) into
profiles/fast_band_margin.jsonl: the sweeps of tests/test_gpu_fast_band.py outside pytest.

Every case of tests/fast_band.py runs its adversarial construction (A: one native step with the Metropolis threshold
2^-34 of the proposal's scale from the exact energy change; C: replay with every step adversarial) at
SMOLMC_FAST_EPS_SCALE = 1, 1/2, ... 2^-20, a fresh handle per scale; ``wrong`` counts the adversarial decisions that
differ from the float64 rule's, ``total`` the adversarial decisions.  The largest scale with a wrong decision is the
measured margin of the case (the band could be that much narrower before a decision turns); none at scale 1 is the
soundness check.  ``family`` is the kernel_info string the handles reported.  The two Wang-Landau lines (construction
"WL": rows of the histogram that differ from the floor-division reference, k = 200, 0.011 eV bins) are a measurement
of another kind: the tolerance of that pre-test does not scale with the band, so no scale is expected to show one.

python tools/fast_band_margin.py [--cases a,b] [--out ...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import chain_law as cl  # noqa: E402
from tests import fast_band as fb  # noqa: E402


def set_env(case, scale):
    for v in cl.DISPATCH_SWITCHES:
        os.environ.pop(v, None)
    os.environ.update(case.env)
    os.environ["SMOLMC_FAST_EPS_SCALE"] = repr(float(scale))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(fb.CASES))  # (the two Wang-Landau sweeps always run)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fast_band_margin.jsonl"))
    a = ap.parse_args()
    with open(a.out, "w") as f:
        for name in a.cases.split(","):
            case = fb.CASES[name]
            for kind in case.constructions:
                if kind == "B":  # (the sweep runs the one-step constructions)
                    continue
                sweep = fb.sweep_a if kind == "A" else fb.sweep_c
                counts = sweep(name, lambda s: set_env(case, s))
                for s, (wrong, total) in counts.items():
                    f.write(json.dumps(dict(case=name, construction=kind, family=fb.INFO[(name, kind)].split(" env=")[0],
                                            scale=s, wrong=wrong, total=total)) + "\n")
                f.flush()
                print(fb.sweep_line(name, kind, counts), flush=True)
        for name in fb.WL_SWEEPS:  # the Wang-Landau bin pre-test: a measurement, no scale is expected to show a wrong row
            def wl_env(scale):
                for v in cl.DISPATCH_SWITCHES:
                    os.environ.pop(v, None)
                os.environ["SMOLMC_FAST_EPS_SCALE"] = repr(float(scale))
            counts = fb.sweep_wl(name, wl_env)
            for s, (wrong, total) in counts.items():
                f.write(json.dumps(dict(case=name, construction="WL", family=fb.INFO[(name, "WL")].split(" env=")[0],
                                        scale=s, wrong=wrong, total=total)) + "\n")
            print(fb.sweep_line(name, "WL", counts), flush=True)


if __name__ == "__main__":
    main()
