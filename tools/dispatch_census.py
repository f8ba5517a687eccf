#!/usr/bin/env python
"""Census of the dispatched kernel instantiations (tests/dispatch_matrix.py).

  --list                 (no device) the four classes with counts per template, and the coordinates the reduced matrix leaves
                         to the full product or lists as unreached
  --search               (device, no launch) create a handle per candidate and print the greedy cover as a TARGETS table
  --run [--full] [--lib release|bounds] [--out FILE]
                         (device, one process) run the reduced matrix -- or, with --full, one candidate per cell that any
                         candidate reaches -- against the CPU oracle; one JSON line per case
  --check-trace DIR --out FILE
                         compare the predicted symbols of a --run (FILE) with the kernel names that
                         `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/dispatch_census.py --run --out FILE`
                         recorded: the one confirmation of predict() that does not rest on restating the launchers.
                         No counters go in the same run."""

import argparse
import collections
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import codeobj, engine  # noqa: E402
from tests import dispatch_matrix as dm  # noqa: E402


def lib_path(which):
    return engine.LIB_PATH if which == "release" else os.path.join(os.path.dirname(engine.LIB_PATH), "libsmolmc_hip_bounds.so")


def do_list(args):
    symbols = sorted(codeobj.kernel_digests(lib_path(args.lib)))
    cls = dm.classify(symbols)
    table = collections.Counter((dm.template_of(s) if dm.coords(s) else "(helpers)", c) for s, c in cls.items())
    classes = ["covered", "dispatchable, not in the reduced matrix", "never dispatched", "helper"]
    print(f"{len(symbols)} kernels")
    print(f"{'template':24s}" + "".join(f"{c[:22]:>24s}" for c in classes))
    for t in list(dm.MC_TEMPLATES) + ["(helpers)"]:
        print(f"{t:24s}" + "".join(f"{table[(t, c)]:24d}" for c in classes))
    need = dm.required(symbols)
    left = need - dm.covered_by(list(dm.TARGETS.values()) + list(dm.UNIV_TARGETS.values()), symbols)  # (+ the universal kernel's layout cases)
    print(f"\nrequired coordinates {len(need)}: covered {len(need) - len(left)}, unreached {len(left)}")
    for why, qs in sorted(collections.Counter(dm.unreached(q) or "NOT CLASSIFIED" for q in left).items(), key=lambda x: -x[1]):
        print(f"  {qs:4d}  {why[:150]}")
    full = collections.Counter(dm.coords(s).F for s, c in cls.items() if c == "dispatchable, not in the reduced matrix")
    print("\ncells left to the full product, per launcher:")
    print("  " + ", ".join(f"{f} {n}" for f, n in sorted(full.items())))
    print("\nnever dispatched:")
    for name, _, why, where in dm.NEVER_DISPATCHED:
        print(f"  {name}: {where}")
    return 0


def _cells(cases):
    """Create every candidate's handle (no launch): [(case, kernel_info, symbol)] of those with a prediction."""
    out, handles = [], {}
    for c in cases:
        key = (c.handle_id, c.drive if c.drive in ("wmu", "win") else "run")
        if key not in handles:
            try:
                with dm.dispatch_env(c):
                    eng = engine.Engine(dm.case_tables(c), dm.config(c))
                    ref = dm.reference(c) if c.drive in ("wmu", "win") else None
                    if c.drive == "wmu":
                        eng.set_walker_mu(ref["rows"])
                    if c.drive == "win":
                        eng.set_wl_windows(ref["windows"][0], ref["windows"][1])
                    handles[key] = eng.kernel_info()
                    eng.close()
            except (engine.EngineError, ValueError) as ex:  # a refusal of smolmc_create or smolmc_set_*: no such cell here
                if str(ex).startswith("hip"):  # (a HIP error is no refusal: nothing more is started on the device)
                    raise
                handles[key] = ex
        info = handles[key]
        if isinstance(info, Exception):
            continue
        try:
            out.append((c, info, dm.predict(info, c.facts)))
        except dm.NoLeanLauncher:
            pass
    return out


def _greedy(cells, symbols):
    need = {q for q in dm.required(symbols) if dm.unreached(q) is None}
    order = sorted(cells, key=lambda x: (x[0].R, len(x[0].env), x[0].id))
    chosen = []
    while need:
        best = max(order, key=lambda x: len(dm.coordinates_of(dm.coords(x[2])) & need))
        gain = dm.coordinates_of(dm.coords(best[2])) & need
        if not gain:
            break
        chosen.append(best)
        need -= gain
    return chosen, need


def do_search(args):
    engine.load_library(lib_path(args.lib))
    symbols = sorted(codeobj.kernel_digests(lib_path(args.lib)))
    chosen, left = _greedy(_cells(list(dm.candidates())), symbols)
    print("TARGETS = {")
    for c, _, s in sorted(chosen, key=lambda x: x[0].id):
        print(f'    "{c.id}": "{dm.show(dm.coords(s))}",')
    print("}")
    print(f"# {len(chosen)} cases; required coordinates without a candidate: {len(left)}", file=sys.stderr)
    for q in sorted(left, key=str):
        print("#  ", q, file=sys.stderr)
    return 0


def do_run(args):
    engine.LIB_PATH = lib_path(args.lib)
    engine._LIB = None
    t0 = time.time()
    if args.full:  # one candidate per cell that any candidate reaches
        seen, cases = set(), []
        for c, info, s in _cells(list(dm.candidates())):
            if s not in seen:
                seen.add(s)
                cases.append(c)
    else:
        cases = dm.CASES
    out = open(args.out, "w") if args.out else sys.stdout
    failed = 0
    for c in cases:
        rec = {"case": c.id, "lib": args.lib}
        t1 = time.time()
        try:
            rec["kernel_info"], rec["predicted"] = dm.run_case(c, engine.Engine)
            rec["result"] = "ok"
            if not args.full and dm.show(dm.coords(rec["predicted"])) != dm.TARGETS[c.id]:
                rec["result"] = f"moved off its cell {dm.TARGETS[c.id]}"
        except AssertionError as ex:
            rec["result"] = "FAILED: " + str(ex)[:300]
        except Exception as ex:  # a HIP error ends the run: nothing more is started on the device
            rec["result"] = f"ERROR: {type(ex).__name__}: {ex}"[:400]
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(f"stopped at {c.id}: {rec['result']}", file=sys.stderr)
            return 2
        rec["seconds"] = round(time.time() - t1, 3)
        failed += rec["result"] != "ok"
        out.write(json.dumps(rec) + "\n")
        out.flush()
    print(f"{len(cases)} cases on the {args.lib} library, {failed} not ok, {time.time() - t0:.1f} s", file=sys.stderr)
    return 1 if failed else 0


def do_check_trace(args):
    rows = []
    for f in glob.glob(os.path.join(args.check_trace, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r.get("Start_Timestamp") or 0), r.get("Kernel_Name") or r.get("Name") or ""))
    rows.sort()
    norm = codeobj._norm
    names = [n[:-3] if n.endswith(".kd") else n for _, n in rows]
    names = [n if n.startswith("void ") else "void " + n for n in names]
    launched = [norm(n) for n in names if dm.coords(n) is not None]
    runs = [json.loads(line) for line in open(args.out)]
    predicted = [norm(r["predicted"]) for r in runs if "predicted" in r]

    def collapse(seq):
        return [x for i, x in enumerate(seq) if i == 0 or seq[i - 1] != x]

    a, b = collapse(launched), collapse(predicted)
    mismatches = [{"position": i, "launched": x, "predicted": y} for i, (x, y) in enumerate(zip(a, b)) if x != y]
    report = {"cases": len(runs), "not_ok": [r for r in runs if r.get("result") != "ok"], "kernel_launches": len(launched),
              "distinct_launched": len(set(launched)), "distinct_predicted": len(set(predicted)),
              "launched_not_predicted": sorted(set(launched) - set(predicted)), "predicted_not_launched": sorted(set(predicted) - set(launched)),
              "sequence_lengths": [len(a), len(b)], "sequence_mismatches": mismatches[:50]}
    print(json.dumps(report, indent=1))
    ok = not report["launched_not_predicted"] and not report["predicted_not_launched"] and not mismatches and len(a) == len(b)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--check-trace", metavar="DIR")
    ap.add_argument("--lib", choices=["release", "bounds"], default="release")
    ap.add_argument("--out", metavar="FILE")
    args = ap.parse_args()
    if args.list:
        return do_list(args)
    if args.search:
        return do_search(args)
    if args.run:
        return do_run(args)
    if args.check_trace:
        if not args.out:
            ap.error("--check-trace needs --out FILE, the JSON lines of the traced --run")
        return do_check_trace(args)
    ap.error("one of --list, --search, --run, --check-trace")


if __name__ == "__main__":
    sys.exit(main())
