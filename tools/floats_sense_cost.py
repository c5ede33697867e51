"""Cost of the float sets' sensors (float_sense_kernel, hnumo_floats_sensors / _record), DESIGN.md §6.1.3.

    python tools/floats_sense_cost.py measure --config dg25L3 --out sense_dg25L3.json
        resident engine, one set seeded on a regular grid (dg25L3: 100 x 100 = 10^4 floats; dg316L3: 632 x 633 =
        4 10^5), after the six mixing advances of tools/floats_cost.py.  Medians of 5 after a warm-up, with min-max:
        (a) hnumo_floats_record plus a device synchronise for the masks 0, 1, 2 and 3;
        (b) the path the sensors replace, timed the same way: hnumo_floats_plan, hnumo_sample_create_ref (a STATE
            and a VORT set), hnumo_sample of both, hnumo_sample_destroy of both.
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \\
            python tools/floats_sense_cost.py profile --config dg25L3
        a run of its own, without counters: float_sense_kernel (mask 3) and sample_kernel (STATE, VORT) on the same
        points, five launches each, once right after creation (the floats sorted by element) and once after the
        six mixing advances.
    python tools/floats_sense_cost.py merge --out floats_sense_cost.json sense_*.json --stats cfg=DIR ...
        one file: the measurements plus the kernels' times per launch and the sorted-to-mixed ratio.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "h-numo_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from floats_cost import half_element_dt, med  # noqa: E402

NLAUNCH = 5


def setup(config):
    """(case, engine, its state arrays, xy, layer): resident, two steps taken, the vorticity products begun."""
    from hnumo import floats as FL
    from hnumo import vorticity as V
    from hnumo.case import build_case, make_config
    from hnumo.engine import Engine
    case = build_case(make_config(config))
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    e.vort_begin(V.coriolis_of(case))
    n = 100 if case.scalars["nelem"] < 10000 else 632
    xy = FL.seed_grid(case, n, n + (0 if n == 100 else 1), margin=0.02)
    layer = (np.arange(xy.shape[1]) % case.scalars["nlayers"] + 1).astype(np.int32)
    return case, e, st, xy, layer


def mix(e, st, df, case):
    e.sync(*st)
    dt = half_element_dt(case, st[0])
    for _ in range(6):
        df.advance(dt=dt)


def replaced_path(e, df, xgl):
    """What a caller did per record before the sensors: four calls and a host plan per source."""
    from hnumo import sample as S
    elem, xe = e.floats_plan(df.id)
    ids = [e.sample_create_ref(xgl, elem, xe, src) for src in (S.STATE, S.VORT)]
    out = [e.sample(i) for i in ids]
    for i in ids:
        e.sample_destroy(i)
    return out


def measure(a):
    import torch
    from hnumo import floats as FL
    from hnumo import sample as S
    case, e, st, xy, layer = setup(a.config)
    Sc = case.scalars
    out = {"config": a.config, "nelem": Sc["nelem"], "ngl": Sc["ngl"], "nlayers": Sc["nlayers"], "floats": int(xy.shape[1]),
           "record_and_synchronise": {}, "stage_path": e.stage_path}
    xgl = S.case_xgl(case)
    for mask in (0, 1, 2, 3):
        df = FL.DeviceFloats(e, xy, layer, sensors=mask)
        mix(e, st, df, case)
        df.begin(every=0, record_every=0, capacity=8)
        torch.cuda.synchronize()

        def record():
            df.record()
            torch.cuda.synchronize()

        r = med(record)
        r["K"] = df.sense_info()[1]
        out["record_and_synchronise"][str(mask)] = r
        if mask == 3:
            def old():
                replaced_path(e, df, xgl)
                torch.cuda.synchronize()
            out["replaced_path_plan_create_sample_destroy"] = med(old)
            g = df.get()
            out["active_after_mixing"] = int((g["status"] == 0).sum())
        df.destroy()
    e.close()
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def profile(a):
    import torch
    from hnumo import floats as FL
    from hnumo import sample as S
    case, e, st, xy, layer = setup(a.config)
    xgl = S.case_xgl(case)
    df = FL.DeviceFloats(e, xy, layer, sensors=3)
    # in the trace: NLAUNCH float_sense_kernel, NLAUNCH sample_kernel STATE, NLAUNCH sample_kernel VORT -- sorted, then mixed
    for phase in ("sorted", "mixed"):
        if phase == "mixed":
            mix(e, st, df, case)
        for _ in range(NLAUNCH):
            df.sense()
        elem, xe = e.floats_plan(df.id)
        for src in (S.STATE, S.VORT):
            sid = e.sample_create_ref(xgl, elem, xe, src)
            for _ in range(NLAUNCH):
                e.sample(sid)
            e.sample_destroy(sid)
        torch.cuda.synchronize()
    e.close()


def merge(a):
    res = {"what": "cost of the float sets' sensors (tools/floats_sense_cost.py)", "cases": {}}
    for p in a.files:
        d = json.load(open(p))
        res["cases"][d["config"]] = d
    for spec in a.stats or []:
        cfg, d = spec.split("=", 1)
        c = res["cases"].get(cfg)
        tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not tr or c is None:
            continue
        rows = [r for r in csv.DictReader(open(tr[0])) if "float_sense_kernel" in r["Kernel_Name"] or "sample_kernel" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
        if len(us) != 6 * NLAUNCH:
            c["kernel_us"] = {"error": f"{len(us)} launches in the trace, expected {6 * NLAUNCH}"}
            continue
        k = c["kernel_us"] = {}
        for i, (phase, which) in enumerate((p, w) for p in ("sorted", "mixed") for w in ("float_sense", "sample_state", "sample_vort")):
            part = us[NLAUNCH * i:NLAUNCH * (i + 1)]
            k.setdefault(phase, {})[which] = {"median_us": statistics.median(part), "min_us": min(part), "max_us": max(part),
                                              "calls": len(part), "kernel": rows[NLAUNCH * i]["Kernel_Name"]}
        for phase in k:
            k[phase]["sense_over_sample_state_plus_vort"] = k[phase]["float_sense"]["median_us"] / (
                k[phase]["sample_state"]["median_us"] + k[phase]["sample_vort"]["median_us"])
        k["float_sense_mixed_over_sorted"] = k["mixed"]["float_sense"]["median_us"] / k["sorted"]["float_sense"]["median_us"]
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("measure", "profile"):
        p = sub.add_parser(name)
        p.add_argument("--config", default="dg25L3")
        p.add_argument("--out", default="floats_sense_cost.json")
    p = sub.add_parser("merge")
    p.add_argument("files", nargs="+")
    p.add_argument("--stats", action="append")
    p.add_argument("--out", required=True)
    a = ap.parse_args()
    {"measure": measure, "profile": profile, "merge": merge}[a.cmd](a)
