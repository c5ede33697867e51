"""Cost of the wind blend (kernels_wind.hip, hnumo_wind_*), DESIGN.md §6.1.6.

    python tools/wind_cost.py measure --config dg316L3 --out cost_dg316L3.json
        resident engine: wall time of hnumo_wind_set followed by a device synchronise (median of 9 after one
        warm-up) for M = 1..4, beside ms_per_step, and the stream-copy bandwidth of the same run.
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \
            python tools/wind_cost.py profile --config dg316L3
        six blends per M under the profiler (a run of its own, no counters), the table-row kernel through a
        schedule and the argument kernel through hnumo_wind_set, a step between them as in a run.
    python tools/wind_cost.py merge --out wind_cost.json cost_*.json --stats cfg=DIR ...
        one file: the measurements plus the kernels' time per launch from the profiler runs and
        (16 M + 64) npoin_q bytes over that time against the stream copy.
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "h-numo_amd"))


def algorithmic_bytes(npoin_q: int, M: int) -> int:
    """Per launch: M patterns read as 16-byte pairs; tau_wind and tau_wind_ave written as pairs (32), the two qstat
    rows (16) and the two qstatE rows (16)."""
    return (16 * M + 64) * npoin_q


def engine_for(config):
    import numpy as np
    from hnumo.case import build_case, make_config
    from hnumo.engine import Engine
    case = build_case(make_config(config), dense=False)
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    rng = np.random.default_rng(3)
    t0 = np.asarray(case.arrays["tau_wind"])
    pat = np.zeros(t0.shape + (4,), order="F")
    pat[:, :, 0] = t0
    for m in range(1, 4):
        pat[:, :, m] = rng.uniform(-0.001, 0.001, size=t0.shape)   # (small: the profiled run steps under them)
    return case, e, st, pat


def med(f, n=9):
    f()                                   # warm-up
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": n}


def measure(a):
    import torch
    from hnumo.engine import Engine
    case, e, st, pat = engine_for(a.config)
    S = case.scalars
    nsteps = 20 if S["nelem"] < 10000 else 3
    out = {"config": a.config, "nelem": S["nelem"], "npoin_q": S["npoin_q"], "N_btp": S["N_btp"], "stage_path": e.stage_path,
           "label": "launch overhead (625 elements)" if S["nelem"] < 10000 else "bandwidth"}
    out["ms_per_step"] = e.bench_steps(nsteps)[0] / nsteps
    out["set_and_sync"] = {}
    for M in (1, 2, 3, 4):
        e.wind_begin(pat[:, :, :M])
        c = [1.0, 0.5, 0.25, 0.125][:M]

        def blend():
            e.wind_set(c)
            torch.cuda.synchronize()

        torch.cuda.synchronize()
        out["set_and_sync"][str(M)] = dict(med(blend), algorithmic_bytes=algorithmic_bytes(S["npoin_q"], M))
        e.wind_end()
    e.close()
    nbytes = 1 << 31
    bw, variant = Engine.stream_copy_bw(0, nbytes, 10)
    out["stream_copy_GBps"] = bw
    out["stream_copy_how"] = f"hnumo_stream_copy_bw, {nbytes} bytes, 10 launches, variant {int(variant)}"
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def profile(a):
    import numpy as np
    import torch
    case, e, st, pat = engine_for(a.config)
    for M in (1, 2, 3, 4):
        e.wind_begin(pat[:, :, :M])
        # a step between the blends, as in a run: the blend finds the caches as the step left them
        tab = np.asfortranarray(np.linspace(0.1, 1.0, 6 * M).reshape(M, 6))
        e.wind_schedule(tab, mode="repeat")
        for _ in range(6):
            e.ti_rk_bcl(*st)
        e.wind_schedule(np.zeros((M, 0)))
        for k in range(6):
            e.wind_set(tab[:, k])
            e.ti_rk_bcl(*st)
        e.wind_end()
    torch.cuda.synchronize()
    e.close()


def merge(a):
    res = {"what": "cost of the wind blend (tools/wind_cost.py)", "cases": {}}
    for p in a.files:
        d = json.load(open(p))
        res["cases"][d["config"]] = d
    for spec in a.stats or []:
        cfg, d = spec.split("=", 1)
        f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not f or cfg not in res["cases"]:
            continue
        c = res["cases"][cfg]
        k = c["kernels_us_per_launch"] = {}
        for row in csv.DictReader(open(f[0])):
            m = re.search(r"wind_blend_kernel<(\d+), *(\d+), *(?:\(bool\))?(true|false|1|0)>", row["Name"])
            if not m:
                continue
            M = int(m.group(1))
            nb = algorithmic_bytes(c["npoin_q"], M)
            avg = float(row["AverageNs"]) / 1e3
            gbs = nb / (avg * 1e-6) / 1e9
            k[f"M{M}-{'table' if m.group(3) in ('true', '1') else 'args'}"] = {
                "calls": int(row["Calls"]), "avg_us": avg, "min_us": float(row["MinNs"]) / 1e3, "algorithmic_bytes": nb,
                "achieved_GBps": gbs, "fraction_of_stream_copy": gbs / c["stream_copy_GBps"]}
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("measure", "profile"):
        p = sub.add_parser(name)
        p.add_argument("--config", default="dg25L3")
        p.add_argument("--out", default="wind_cost.json")
    p = sub.add_parser("merge")
    p.add_argument("files", nargs="+")
    p.add_argument("--stats", action="append")
    p.add_argument("--out", required=True)
    a = ap.parse_args()
    {"measure": measure, "profile": profile, "merge": merge}[a.cmd](a)
