"""Cost of the online flow statistics (kernels_stats.hip, hnumo_stats_*), DESIGN.md §6.1.1.

    python tools/flowstats_cost.py measure --config dg25L3 --out cost_dg25L3.json
        resident engine: wall time of one sample (hnumo_stats_accumulate, then a device
        synchronise; series on and off; median of 5 after one warm-up) beside ms_per_step, beside
        the host path for the same numbers (hnumo_sync + HostFlowStats.add) and beside the step loop
        with every=1; the stream-copy bandwidth of the same run.
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \
            python tools/flowstats_cost.py profile --config dg25L3
        six samples with and six without the series under the profiler (a run of its own), a step
        before each.
    python tools/flowstats_cost.py merge --out flowstats_cost.json cost_*.json --stats cfg=DIR ...
        one file: the measurements plus the kernels' time per launch from the profiler runs and
        the achieved bandwidth of stats_accumulate_kernel against the stream copy.
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


def algorithmic_bytes(npoin: int, L: int) -> int:
    """stats_accumulate_kernel per launch: per node q read (24 L), the four sums read and written
    (64 L), the weight read (8; series on)."""
    return (24 * L + 64 * L + 8) * npoin


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
    from hnumo import flowstats as F
    from hnumo.engine import Engine
    case, e, (q, qb, qp) = engine_for(a.config)
    S = case.scalars
    nsteps = 20 if S["nelem"] < 10000 else 3
    out = {"config": a.config, "nelem": S["nelem"], "npoin": S["npoin"], "nlayers": S["nlayers"],
           "stage_path": e.stage_path, "label": "launch overhead (625 elements)" if S["nelem"] < 10000 else "bandwidth"}
    out["ms_per_step"] = e.bench_steps(nsteps)[0] / nsteps

    def sample():
        e.stats_accumulate()
        torch.cuda.synchronize()

    for tag, cap in (("series_on", 64), ("series_off", 0)):
        e.stats_begin(0, cap)
        torch.cuda.synchronize()
        out["sample_" + tag] = med(sample)
    e.stats_end()
    for tag, ser in (("series_on", True), ("series_off", False)):
        host = F.HostFlowStats(case, series=ser)

        def host_sample():
            e.sync(q, qb, qp)
            host.add(q)

        out["host_path_" + tag] = med(host_sample)
        t = time.perf_counter()
        e.sync(q, qb, qp)
        out["host_path_" + tag]["sync_alone_ms"] = (time.perf_counter() - t) * 1e3
        out["ratio_" + tag] = out["host_path_" + tag]["median_ms"] / out["sample_" + tag]["median_ms"]

    def loop():
        t = time.perf_counter()
        for _ in range(nsteps):
            e.ti_rk_bcl(q, qb, qp)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / nsteps

    spread = lambda r: {"median": statistics.median(r), "min": min(r), "max": max(r), "runs": len(r)}
    loop()
    out["loop_ms_per_step_stats_off"] = spread([loop() for _ in range(5)])
    e.stats_begin(1, nsteps)
    loop()
    e.stats_series(clear=True)
    runs = []
    for _ in range(5):
        runs.append(loop())
        e.stats_series(clear=True)
    out["loop_ms_per_step_every1_series_on"] = spread(runs)
    e.stats_end()
    e.close()
    nbytes = 1 << 31
    bw, variant = Engine.stream_copy_bw(0, nbytes, 10)
    out["stream_copy_GBps"] = bw
    out["stream_copy_how"] = f"hnumo_stream_copy_bw, {nbytes} bytes, 10 launches, variant {int(variant)}"
    out["algorithmic_bytes_per_launch"] = algorithmic_bytes(S["npoin"], S["nlayers"])
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def profile(a):
    import torch
    case, e, st = engine_for(a.config)
    # a step before every sample, as in a run: the sample finds the caches as the step left them
    for cap in (16, 0):
        e.stats_begin(0, cap)
        for _ in range(6):
            e.ti_rk_bcl(*st)
            e.stats_accumulate()
        torch.cuda.synchronize()
    e.stats_fields()
    e.close()


def merge(a):
    res = {"what": "cost of one flow-statistics sample (tools/flowstats_cost.py)", "cases": {}}
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
            if "stats_" in row["Name"]:
                name = row["Name"].split("hnumo::")[1].split("(")[0]
                k[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                           "min_us": float(row["MinNs"]) / 1e3}
        for name, v in k.items():
            if name.startswith("stats_accumulate_kernel"):
                nb = c["algorithmic_bytes_per_launch"] - (0 if "true" in name else 8 * c["npoin"])
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
        p.add_argument("--out", default="flowstats_cost.json")
    p = sub.add_parser("merge")
    p.add_argument("files", nargs="+")
    p.add_argument("--stats", action="append")
    p.add_argument("--out", required=True)
    a = ap.parse_args()
    {"measure": measure, "profile": profile, "merge": merge}[a.cmd](a)
