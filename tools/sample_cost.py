"""Cost of sampling the resident state (kernels_sample.hip, hnumo_sample_*), DESIGN.md §6.1.2.

    python tools/sample_cost.py measure --config dg25L3 --out cost_dg25L3.json
        resident engine, two sets: the output grid (dg25L3: its 20 km grid, 101 x 101; dg316L3: about
        one point per element-quarter, 631 x 631) and 16 stations.  Per set the wall time of
        hnumo_sample (sample, copy back, transpose) and of hnumo_sample_record + a device synchronise
        (median of 5 after one warm-up), beside the host path for the same numbers (hnumo_sync +
        HostSampler.sample) and ms_per_step; the one-off cost of hnumo_sample_create; the
        stream-copy bandwidth of the same run.
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \
            python tools/sample_cost.py profile --config dg25L3
        six recordings of each set under the profiler (a run of its own), a step before each.
    python tools/sample_cost.py merge --out sample_cost.json cost_*.json --stats cfg=DIR ...
        one file: the measurements plus sample_kernel's time per launch from the profiler runs and
        its achieved bandwidth against the stream copy.
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

LDS_BYTES, CHUNK = 32768, 256          # sample_plan.h: SP_LDS_BYTES, SP_CHUNK


def element_reads(elem, K: int) -> int:
    """Element records the kernel reads for a plan: the distinct elements of every chunk (at most
    CHUNK points and K distinct elements; the rule of sample_chunks in sample_plan.h)."""
    reads = npts = nel = last = 0
    for e in np.sort(np.asarray(elem), kind="stable"):
        fresh = e != 0 and e != last
        if npts == CHUNK or (fresh and nel == K):
            npts = nel = last = 0
        if fresh:
            nel += 1
            reads += 1
            last = e
        npts += 1
    return reads


def algorithmic_bytes(elem, ngl: int, L: int) -> dict:
    """sample_kernel per launch, source STATE: per element read q (24 L), qb (32) and zbot (8) at
    its P nodes; per point the 2 ngl weights, slot and perm (8) and the V values written."""
    P, V, M = ngl * ngl, 5 * L + 4, len(elem)
    K = LDS_BYTES // (8 * ((V * P) | 1))
    reads = element_reads(elem, K)
    return {"K": K, "element_reads": reads, "elements_touched": int(np.unique(elem[elem > 0]).size),
            "fields": reads * P * (24 * L + 40), "weights_and_lists": M * (16 * ngl + 8), "output": M * 8 * V,
            "total": reads * P * (24 * L + 40) + M * (16 * ngl + 8) + M * 8 * V}


def sets_for(case):
    """name -> xy of the two sets"""
    from hnumo import sample as S
    c = np.asarray(case.arrays["coord"])[0:2]
    lo, hi = c.min(axis=1), c.max(axis=1)
    if case.scalars["nelem"] < 10000:
        dx = dy = 20.0e3                                     # compute_ssh.m:61-62
    else:
        n = 2 * int(round(np.sqrt(case.scalars["nelem"])))   # about one point per element-quarter
        dx, dy = (hi[0] - lo[0]) / (n - 2), (hi[1] - lo[1]) / (n - 2)
    xi, yi, xy = S.regular_grid(case, dx, dy)
    rng = np.random.default_rng(16)
    st = lo[:, None] + (hi - lo)[:, None] * rng.uniform(0.05, 0.95, (2, 16))
    return {"grid": (xy, f"{xi.size} x {yi.size}"), "stations": (np.asfortranarray(st), "16")}


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
    from hnumo import sample as S
    from hnumo.engine import Engine
    case, e, (q, qb, qp) = engine_for(a.config)
    Sc = case.scalars
    nsteps = 20 if Sc["nelem"] < 10000 else 3
    out = {"config": a.config, "nelem": Sc["nelem"], "npoin": Sc["npoin"], "nlayers": Sc["nlayers"], "ngl": Sc["ngl"],
           "stage_path": e.stage_path, "sets": {}}
    out["ms_per_step"] = e.bench_steps(nsteps)[0] / nsteps
    t = time.perf_counter()
    e.sync(q, qb, qp)
    out["sync_alone_ms"] = (time.perf_counter() - t) * 1e3
    for name, (xy, shape) in sets_for(case).items():
        r = out["sets"][name] = {"points": int(xy.shape[1]), "shape": shape}
        t = time.perf_counter()
        ds = S.DeviceSampler(e, xy=xy)
        r["create_ms"] = (time.perf_counter() - t) * 1e3
        elem, xi, eta = ds.plan()
        r["located"] = int((elem > 0).sum())
        r["algorithmic_bytes"] = algorithmic_bytes(elem, Sc["ngl"], Sc["nlayers"])
        ds.series_begin(0, 8)
        torch.cuda.synchronize()

        def record():
            ds.record()
            torch.cuda.synchronize()

        r["sample"] = med(ds.sample)
        r["record_and_synchronise"] = med(record)
        hs = ds.host_sampler()

        def host_path():
            e.sync(q, qb, qp)
            return hs.sample(q, qb)

        r["host_path"] = med(host_path)
        t = time.perf_counter()
        want = hs.sample(q, qb)
        r["host_path"]["mirror_alone_ms"] = (time.perf_counter() - t) * 1e3
        r["equal_mirror"] = bool(np.array_equal(ds.sample(), want))
        r["ratio_host_over_sample"] = r["host_path"]["median_ms"] / r["sample"]["median_ms"]
        r["ratio_host_over_record"] = r["host_path"]["median_ms"] / r["record_and_synchronise"]["median_ms"]
        ds.destroy()
    e.close()
    nbytes = 1 << 31
    bw, variant = Engine.stream_copy_bw(0, nbytes, 10)
    out["stream_copy_GBps"] = bw
    out["stream_copy_how"] = f"hnumo_stream_copy_bw, {nbytes} bytes, 10 launches, variant {int(variant)}"
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def profile(a):
    import torch
    from hnumo import sample as S
    case, e, st = engine_for(a.config)
    # a step before every recording, as in a run: the sample finds the caches as the step left them;
    # the grid's launches come first in the trace, then the stations'
    for name, (xy, _) in sets_for(case).items():
        ds = S.DeviceSampler(e, xy=xy)
        ds.series_begin(0, 6)
        for _ in range(6):
            e.ti_rk_bcl(*st)
            ds.record()
        torch.cuda.synchronize()
        ds.destroy()
    e.close()


def merge(a):
    res = {"what": "cost of sampling the resident state (tools/sample_cost.py)", "cases": {}}
    for p in a.files:
        d = json.load(open(p))
        res["cases"][d["config"]] = d
    for spec in a.stats or []:
        cfg, d = spec.split("=", 1)
        c = res["cases"].get(cfg)
        tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not tr or c is None:
            continue
        # per launch from the trace, in launch order: six of the grid, then six of the stations
        rows = [r for r in csv.DictReader(open(tr[0])) if "sample_kernel" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
        for name, part in (("grid", us[:6]), ("stations", us[6:12])):
            if not part:
                continue
            s = c["sets"][name]
            k = s["kernel_us"] = {"calls": len(part), "median_us": statistics.median(part), "min_us": min(part),
                                  "max_us": max(part), "workgroups": int(rows[0 if name == "grid" else 6].get("Grid_Size_X", 0) or 0) // CHUNK}
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
        p.add_argument("--out", default="sample_cost.json")
    p = sub.add_parser("merge")
    p.add_argument("files", nargs="+")
    p.add_argument("--stats", action="append")
    p.add_argument("--out", required=True)
    a = ap.parse_args()
    {"measure": measure, "profile": profile, "merge": merge}[a.cmd](a)
