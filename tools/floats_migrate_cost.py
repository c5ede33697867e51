"""Cost of migrating float sets on a local group of processor-face ranks (hnumo_group_floats_*), DESIGN.md §6.1.3.

    python tools/floats_migrate_cost.py measure --config dg316L3 --ranks 2 --out mig_2.json
        the case split into `ranks` block ranks in a local group on one GPU; for 10^4 and 4 10^5 floats on a
        regular grid (medians of 5 after a warm-up, wall time with a device synchronise):
          the group step with the set migrating (every = 1);
          the same step with the same set not migrating, in the same run: the baseline;
          the group step without any set;
          the explicit group advance, with a dt that moves the fastest float half an element;
          the rounds and the floats in flight per advance, counted by carrying the records through
          hnumo_floats_outbox / _deliver on a second, identical set.
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \\
            python tools/floats_migrate_cost.py profile --config dg316L3 --ranks 2
        six explicit advances of the large set migrating, then six not migrating, under the profiler (a run
        of its own, no counters).
    python tools/floats_migrate_cost.py merge --out floats_migrate_cost.json mig_*.json --stats 2=DIR ...
        one file: the measurements plus the kernels' time per launch from the profiler runs.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "h-numo_amd"))

SIZES = {"1e4": (100, 100), "4e5": (632, 633)}


def group_for(config, ranks):
    from hnumo.case import build_case, make_config
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    from hnumo.facepart import face_partition
    case = build_case(make_config(config))
    parts = [face_partition(case, ranks, r, "block") for r in range(ranks)]
    engines = [Engine(p) for p in parts]
    local_group(engines)
    sts = [e.state() for e in engines]
    for e in engines:
        e.set_resident(True)
    for _ in range(2):
        group_ti_rk_bcl(engines, sts)
    return case, parts, engines, sts


def half_element_dt(case, engines, sts):
    c = np.asarray(case.arrays["coord"])
    h = np.sqrt((c[0].max() - c[0].min()) * (c[1].max() - c[1].min()) / case.scalars["nelem"])
    sp = 0.0
    for e, (q, qb, qp) in zip(engines, sts):
        e.sync(q, qb, qp)
        sp = max(sp, float(np.sqrt((q[1] / q[0]) ** 2 + (q[2] / q[0]) ** 2).max()))
    return float(0.5 * h / sp) if sp > 0 else float(case.scalars["dt"])


def med(f, n=5):
    f()                                   # warm-up
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": n}


def seeds(case, size):
    from hnumo import floats as FL
    xy = FL.seed_grid(case, *SIZES[size], margin=0.02)
    return xy, (np.arange(xy.shape[1]) % case.scalars["nlayers"] + 1).astype(np.int32)


def carried_advance(engines, fid, dt, max_rounds):
    """One advance with the records carried by the host: [floats in flight in round 1, 2, ...]."""
    for e in engines:
        e.floats_advance(fid, dt)
    flights = []
    for _ in range(max_rounds + 1):
        boxes = [e.floats_outbox(fid) for e in engines]
        n = sum(d.shape[1] for d, _ in boxes)
        if not n:
            break
        flights.append(n)
        for src, (d, i) in enumerate(boxes):
            for dst in np.unique(i[4]):
                sel = i[4] == dst
                engines[int(dst)].floats_deliver(fid, src, d[:, sel], i[:, sel])
    for e in engines:
        e.floats_settle(fid)
    return flights


def measure(a):
    import torch
    from hnumo import floats as FL
    from hnumo.engine import group_floats_migrate, group_ti_rk_bcl
    case, parts, engines, sts = group_for(a.config, a.ranks)
    Sc = case.scalars
    scale = float(np.abs(np.asarray(case.arrays["coord"])[0:2]).max())
    out = {"config": a.config, "ranks": a.ranks, "nelem": Sc["nelem"], "ngl": Sc["ngl"], "nlayers": Sc["nlayers"], "sets": {}}

    def step():
        group_ti_rk_bcl(engines, sts)
        torch.cuda.synchronize()

    out["group_step_no_set"] = med(step)
    for size in SIZES:
        xy, layer = seeds(case, size)
        r = out["sets"][size] = {"floats": int(xy.shape[1])}
        gf = FL.GroupFloats(engines, xy, layer, coord_scale=scale)
        gf.begin(every=1)
        r["group_step_migrating"] = med(step)
        group_floats_migrate(engines, gf.id, False, 0.0)
        r["group_step_same_set_not_migrating"] = med(step)
        group_floats_migrate(engines, gf.id, True, scale)
        gf.begin(every=0)
        dt = r["advance_dt"] = half_element_dt(case, engines, sts)      # (of the state now: the flow spins up from rest)

        def advance():
            gf.advance(dt=dt)
            torch.cuda.synchronize()

        r["group_advance"] = med(advance)
        r["active_after"] = int(sum((g["status"] == 0).sum() for g in gf.get()))
        r["lost_after"] = int(sum((g["status"] == 2).sum() for g in gf.get()))
        gf.destroy()
        twin = FL.GroupFloats(engines, xy, layer, coord_scale=scale)
        r["flights_per_round_of_6_advances"] = [carried_advance(engines, twin.id, dt, FL.MAXROUNDS) for _ in range(6)]
        r["rounds_per_advance"] = [len(f) for f in r["flights_per_round_of_6_advances"]]
        twin.destroy()
    for e in engines:
        e.close()
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def profile(a):
    import torch
    from hnumo import floats as FL
    from hnumo.engine import group_floats_migrate
    case, parts, engines, sts = group_for(a.config, a.ranks)
    scale = float(np.abs(np.asarray(case.arrays["coord"])[0:2]).max())
    dt = half_element_dt(case, engines, sts)
    xy, layer = seeds(case, "4e5")
    gf = FL.GroupFloats(engines, xy, layer, coord_scale=scale)
    for _ in range(6):
        gf.advance(dt=dt)
    torch.cuda.synchronize()
    group_floats_migrate(engines, gf.id, False, 0.0)
    for _ in range(6):
        for s in gf.sets:
            s.advance(dt=dt)
    torch.cuda.synchronize()
    for e in engines:
        e.close()


def merge(a):
    res = {"what": "cost of migrating float sets on a local group (tools/floats_migrate_cost.py)", "cases": {}}
    for p in a.files:
        d = json.load(open(p))
        res["cases"][str(d["ranks"])] = d
    for spec in a.stats or []:
        ranks, d = spec.split("=", 1)
        c = res["cases"].get(ranks)
        tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not tr or c is None:
            continue
        rows = list(csv.DictReader(open(tr[0])))
        k = c["kernel_us_4e5"] = {}
        for key, pat in (("float_advance_kernel<5,1,true>", "float_advance_kernelILi5ELi1ELb1"), ("float_advance_kernel<5,1,false>", "float_advance_kernelILi5ELi1ELb0"),
                         ("float_arrive_kernel<5>", "float_arrive_kernelILi5")):
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
                  if pat in r["Kernel_Name"] or key.replace(",", ", ") in r["Kernel_Name"]]
            if us:
                k[key] = {"calls": len(us), "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "total_us": sum(us)}
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("measure", "profile"):
        p = sub.add_parser(name)
        p.add_argument("--config", default="dg316L3")
        p.add_argument("--ranks", type=int, default=2)
        p.add_argument("--out", default="floats_migrate_cost.json")
    p = sub.add_parser("merge")
    p.add_argument("files", nargs="+")
    p.add_argument("--stats", action="append")
    p.add_argument("--out", required=True)
    a = ap.parse_args()
    {"measure": measure, "profile": profile, "merge": merge}[a.cmd](a)
