"""Cost of the vorticity products (kernels_vort.hip, hnumo_vort_*), DESIGN.md §6.1.4.

    python tools/vort_cost.py measure --config dg25L3 --out cost_dg25L3.json
        resident engine: wall time of one series sample (hnumo_vort_record, then a device
        synchronise; median of 5 after one warm-up) and of hnumo_vort_fields (the kernel without the
        series, the copy back and the host transpose), beside ms_per_step and beside the host path
        for the same numbers (hnumo_sync + HostVorticity); the stream-copy bandwidth of the same run.
        hnumo_vort_record without a series is refused (code 4), so the series-off kernel is timed
        through hnumo_vort_fields here and alone in the profiler run.
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \
            python tools/vort_cost.py profile --config dg25L3
        six samples with the series and six field read-outs under the profiler (a run of its own, no
        counters), a step before each.
    python tools/vort_cost.py merge --out vort_cost.json cost_*.json --stats cfg=DIR ...
        one file: the measurements plus the kernels' time per launch from the profiler runs and the
        achieved bandwidth of vort_kernel against the stream copy.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "h-numo_amd"))


def algorithmic_bytes(npoin: int, L: int, series: bool) -> int:
    """vort_kernel per launch and node: q read (24 L), the four metric rows (32), f (8), the four
    fields written (32 L), the weight read (8; series on)."""
    return (24 * L + 32 + 8 + 32 * L + (8 if series else 0)) * npoin


def engine_for(config):
    from hnumo.case import build_case, make_config
    from hnumo.engine import Engine
    case = build_case(make_config(config))
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    return case, e, st


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
    from hnumo import vorticity as V
    from hnumo.engine import Engine
    case, e, (q, qb, qp) = engine_for(a.config)
    S = case.scalars
    nsteps = 20 if S["nelem"] < 10000 else 3
    out = {"config": a.config, "nelem": S["nelem"], "npoin": S["npoin"], "nlayers": S["nlayers"],
           "stage_path": e.stage_path, "label": "launch overhead (625 elements)" if S["nelem"] < 10000 else "bandwidth"}
    out["ms_per_step"] = e.bench_steps(nsteps)[0] / nsteps
    f = V.coriolis_of(case)

    def record():
        e.vort_record()
        torch.cuda.synchronize()
        e.vort_series(clear=True)

    e.vort_begin(f, 0, 64)
    torch.cuda.synchronize()
    out["record_series_on"] = med(record)
    out["record_series_off"] = "refused (code 4: no series); the series-off kernel runs in hnumo_vort_fields"
    out["fields_copy_and_transpose"] = med(e.vort_fields)
    e.vort_end()
    host = V.HostVorticity(case)

    def host_sample():
        e.sync(q, qb, qp)
        host.add(q)

    def host_fields():
        e.sync(q, qb, qp)
        host.fields(q)

    out["host_path_series"] = med(host_sample)
    out["host_path_fields"] = med(host_fields)
    t = time.perf_counter()
    e.sync(q, qb, qp)
    out["sync_alone_ms"] = (time.perf_counter() - t) * 1e3
    out["ratio_series"] = out["host_path_series"]["median_ms"] / out["record_series_on"]["median_ms"]
    out["ratio_fields"] = out["host_path_fields"]["median_ms"] / out["fields_copy_and_transpose"]["median_ms"]
    e.close()
    nbytes = 1 << 31
    bw, variant = Engine.stream_copy_bw(0, nbytes, 10)
    out["stream_copy_GBps"] = bw
    out["stream_copy_how"] = f"hnumo_stream_copy_bw, {nbytes} bytes, 10 launches, variant {int(variant)}"
    out["algorithmic_bytes_per_launch"] = {"series_on": algorithmic_bytes(S["npoin"], S["nlayers"], True),
                                           "series_off": algorithmic_bytes(S["npoin"], S["nlayers"], False)}
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def profile(a):
    import torch
    from hnumo import vorticity as V
    case, e, st = engine_for(a.config)
    # a step before every sample, as in a run: the sample finds the caches as the step left them
    e.vort_begin(V.coriolis_of(case), 0, 16)
    e.stats_begin(0, 16)                  # the neighbouring kernel, in the same run
    for _ in range(6):
        e.ti_rk_bcl(*st)
        e.vort_record()
        e.ti_rk_bcl(*st)
        e.stats_accumulate()
    for _ in range(6):
        e.ti_rk_bcl(*st)
        e.vort_fields()
    torch.cuda.synchronize()
    e.close()


def merge(a):
    res = {"what": "cost of the vorticity products (tools/vort_cost.py)", "cases": {}}
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
            if "vort_kernel" in row["Name"] or "stats_" in row["Name"]:
                name = row["Name"].split("hnumo::")[1].split("(")[0]
                k[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                           "min_us": float(row["MinNs"]) / 1e3}
        L, npoin = c["nlayers"], c["npoin"]
        for name, v in k.items():
            if name.startswith("vort_kernel"):
                nb = c["algorithmic_bytes_per_launch"]["series_on" if "true" in name else "series_off"]
            elif name.startswith("stats_accumulate_kernel"):
                nb = (24 * L + 64 * L + (8 if "true" in name else 0)) * npoin
            else:
                continue
            v["algorithmic_bytes"] = nb
            v["achieved_GBps"] = nb / (v["avg_us"] * 1e-6) / 1e9
            v["fraction_of_stream_copy"] = v["achieved_GBps"] / c["stream_copy_GBps"]
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("measure", "profile"):
        p = sub.add_parser(name)
        p.add_argument("--config", default="dg25L3")
        p.add_argument("--out", default="vort_cost.json")
    p = sub.add_parser("merge")
    p.add_argument("files", nargs="+")
    p.add_argument("--stats", action="append")
    p.add_argument("--out", required=True)
    a = ap.parse_args()
    {"measure": measure, "profile": profile, "merge": merge}[a.cmd](a)
