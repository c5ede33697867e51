"""Cost of advancing float sets on the resident state (kernels_float.hip, hnumo_floats_*), DESIGN.md §6.1.3.

    python tools/floats_cost.py measure --config dg25L3 --out cost_dg25L3.json
        resident engine, two sets seeded on a regular grid: the large one (dg25L3: 100 x 100 = 10^4
        floats; dg316L3: 632 x 633 = 4 10^5) and 16.  Per set and lane mapping (a row per lane, one lane
        per float) the wall time of one advance plus a device synchronise (median of 5 after one
        warm-up) with a dt that moves the fastest float half an element; hnumo_sync alone, the floor
        of any host pass; ms_per_step and the stream-copy bandwidth of the same run; the step loop
        with every = 1 on 10^4 floats beside the same loop without floats.
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \
            python tools/floats_cost.py profile --config dg25L3
        six advances of each set in each lane mapping under the profiler (a run of its own).
    python tools/floats_cost.py merge --out floats_cost.json cost_*.json --stats cfg=DIR ...
        one file: the measurements plus float_advance_kernel's time per launch from the profiler runs
        and its achieved bandwidth against the stream copy.
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

MAPPINGS = {"lane": "0", "rows": "1"}        # HNUMO_FLOAT_ROWS; the first is the engine's default


def algorithmic_bytes(elem_before, elem_after, ngl: int) -> dict:
    """float_advance_kernel per launch: a float's record read (6 doubles, 4 ints) and written (6
    doubles, 3 ints), and three evaluations of 24 P bytes per distinct element touched."""
    P, M = ngl * ngl, len(elem_before)
    touched = int(np.unique(np.concatenate([elem_before[elem_before > 0], elem_after[elem_after > 0]])).size)
    rec = M * (64 + 60)
    return {"records": rec, "elements_touched": touched, "fields": 3 * touched * 24 * P, "total": rec + 3 * touched * 24 * P}


def sets_for(case):
    from hnumo import floats as FL
    n = 100 if case.scalars["nelem"] < 10000 else 632
    return {"large": FL.seed_grid(case, n, n + (0 if n == 100 else 1), margin=0.02), "16": FL.seed_grid(case, 4, 4)}


def engine_for(config, rows):
    from hnumo.case import build_case, make_config
    from hnumo.engine import Engine
    os.environ["HNUMO_EXPERIMENTS"] = "1"
    os.environ["HNUMO_FLOAT_ROWS"] = rows
    case = build_case(make_config(config))
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    return case, e, st


def half_element_dt(case, q):
    c = np.asarray(case.arrays["coord"])
    h = np.sqrt((c[0].max() - c[0].min()) * (c[1].max() - c[1].min()) / case.scalars["nelem"])
    sp = np.sqrt((q[1] / q[0]) ** 2 + (q[2] / q[0]) ** 2).max()
    return float(0.5 * h / sp) if sp > 0 else float(case.scalars["dt"])


def med(f, n=5):
    f()                                   # warm-up
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": n}


def measure(a):
    import torch
    from hnumo import floats as FL
    from hnumo.engine import Engine
    out = {"config": a.config, "sets": {}}
    for mapping, rows in MAPPINGS.items():
        case, e, (q, qb, qp) = engine_for(a.config, rows)
        Sc = case.scalars
        nsteps = 20 if Sc["nelem"] < 10000 else 3
        out.update(nelem=Sc["nelem"], npoin=Sc["npoin"], nlayers=Sc["nlayers"], ngl=Sc["ngl"], stage_path=e.stage_path,
                   overrides=e.overrides if hasattr(e, "overrides") else None)
        if mapping == "lane":
            out["ms_per_step"] = e.bench_steps(nsteps)[0] / nsteps
            t = time.perf_counter()
            e.sync(q, qb, qp)
            out["sync_alone_ms"] = (time.perf_counter() - t) * 1e3
            out["sync_alone"] = med(lambda: e.sync(q, qb, qp))
        else:
            e.sync(q, qb, qp)
        dt = half_element_dt(case, q)
        out["advance_dt"] = dt
        for name, xy in sets_for(case).items():
            r = out["sets"].setdefault(name, {"floats": int(xy.shape[1])})
            layer = (np.arange(xy.shape[1]) % Sc["nlayers"] + 1).astype(np.int32)
            t = time.perf_counter()
            df = FL.DeviceFloats(e, xy, layer)
            r["create_ms"] = (time.perf_counter() - t) * 1e3
            before = df.get()
            torch.cuda.synchronize()

            def advance():
                df.advance(dt=dt)
                torch.cuda.synchronize()

            r[f"advance_and_synchronise_{mapping}"] = med(advance)
            after = df.get()
            r["active_after_6"] = int((after["status"] == 0).sum())
            r["changed_element"] = int(((after["elem"] != before["elem"]) & (after["elem"] > 0)).sum())
            r["algorithmic_bytes"] = algorithmic_bytes(before["elem"], after["elem"], Sc["ngl"])
            if name == "large" and mapping == "lane":
                # the step loop with the set advanced after every step, beside the loop without
                def loop():
                    for _ in range(nsteps):
                        e.ti_rk_bcl(q, qb, qp)
                    torch.cuda.synchronize()
                plain = med(loop, 3)
                d4 = FL.DeviceFloats(e, FL.seed_grid(case, 100, 100, margin=0.02), 1)
                d4.begin(every=1)
                with_floats = med(loop, 3)
                d4.destroy()
                out["step_loop_10k_floats"] = {"steps": nsteps, "without_ms_per_step": plain["median_ms"] / nsteps,
                                  "with_every_1_ms_per_step": with_floats["median_ms"] / nsteps}
            df.destroy()
        e.close()
    nbytes = 1 << 31
    bw, variant = Engine.stream_copy_bw(0, nbytes, 10)
    out["stream_copy_GBps"] = bw
    out["stream_copy_how"] = f"hnumo_stream_copy_bw, {nbytes} bytes, 10 launches, variant {int(variant)}"
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def profile(a):
    import torch
    from hnumo import floats as FL
    # in the trace: mapping by mapping, the large set's six launches, then the 16's
    for mapping, rows in MAPPINGS.items():
        case, e, (q, qb, qp) = engine_for(a.config, rows)
        e.sync(q, qb, qp)
        dt = half_element_dt(case, q)
        for name, xy in sets_for(case).items():
            layer = (np.arange(xy.shape[1]) % case.scalars["nlayers"] + 1).astype(np.int32)
            df = FL.DeviceFloats(e, xy, layer)
            for _ in range(6):
                e.ti_rk_bcl(q, qb, qp)
                df.advance(dt=dt)
            torch.cuda.synchronize()
            df.destroy()
        e.close()


def merge(a):
    res = {"what": "cost of advancing float sets on the resident state (tools/floats_cost.py)", "cases": {}}
    for p in a.files:
        d = json.load(open(p))
        res["cases"][d["config"]] = d
    for spec in a.stats or []:
        cfg, d = spec.split("=", 1)
        c = res["cases"].get(cfg)
        tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not tr or c is None:
            continue
        rows = [r for r in csv.DictReader(open(tr[0])) if "float_advance_kernel" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
        for i, (mapping, name) in enumerate((m, n) for m in MAPPINGS for n in ("large", "16")):
            part = us[6 * i:6 * i + 6]
            if len(part) < 6:
                continue
            s = c["sets"][name]
            k = s.setdefault("kernel_us", {})[mapping] = {"calls": len(part), "median_us": statistics.median(part), "min_us": min(part),
                                                          "max_us": max(part), "kernel": rows[6 * i]["Kernel_Name"]}
            nb = s["algorithmic_bytes"]["total"]
            k["achieved_GBps"] = nb / (k["median_us"] * 1e-6) / 1e9
            k["fraction_of_stream_copy"] = k["achieved_GBps"] / c["stream_copy_GBps"]
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("measure", "profile"):
        p = sub.add_parser(name)
        p.add_argument("--config", default="dg25L3")
        p.add_argument("--out", default="floats_cost.json")
    p = sub.add_parser("merge")
    p.add_argument("files", nargs="+")
    p.add_argument("--stats", action="append")
    p.add_argument("--out", required=True)
    a = ap.parse_args()
    {"measure": measure, "profile": profile, "merge": merge}[a.cmd](a)
