"""Cost of a region set's sample (kernels_region.hip, hnumo_regions_*), DESIGN.md §6.1.9.

    python tools/regions_cost.py measure --config dg316L3 --out cost_dg316L3.json
        resident engine, two steps taken: the time of one sample (region_accumulate_kernel and the tree's
        launches) of a set whose one region holds every element and of a set of nely zonal strips (one per
        element row), for the FLOW rows, the VORT rows and both, and in the same run of a statistics sample
        and a vorticity sample with their series (the kernel and the tree), each two ways -- `queued`: QUEUE
        samples launched back to back and one device synchronise, divided by QUEUE (the kernels run one after
        the other on the engine stream, so the launch overhead is hidden behind the kernel before: the kernel
        time); `single`: one sample and a synchronise (what a caller who waits sees) -- median of 5 after a
        warm-up; the bytes a sample moves, the stream-copy rate of the same run and the fraction of it each
        reaches.
    python tools/regions_cost.py merge --out regions_cost.json cost_*.json
        one file.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "h-numo_amd"))
QUEUE = 20
CAP = 6 * (QUEUE + 1) + 4


def region_bytes(npoin: int, nelem: int, L: int, mask: int) -> int:
    """region_accumulate_kernel per launch with every element a member.  Per node and layer q read (24); per
    node jac (8), with VORT the four metric rows and f (40); per element its member entry (4) and V partials
    written (8 V).  (The tree reads the partials once more: 8 V per element.)"""
    V = (4 * L if mask & 1 else 0) + (3 * L if mask & 2 else 0)
    return (24 * L + 8 + (40 if mask & 2 else 0)) * npoin + (4 + 16 * V) * nelem


def stats_bytes(npoin: int, nelem: int, L: int) -> int:
    """stats_accumulate_kernel with the series: per node and layer q read (24), the four sums read and written
    (64); per node jac (8); per element 2L partials written and read by the tree."""
    return (88 * L + 8) * npoin + 32 * L * nelem


def vort_bytes(npoin: int, nelem: int, L: int) -> int:
    """vort_kernel<.,.,true>: per node and layer q read (24), four fields written (32); per node the metric
    rows, f and jac (48); per element 3L partials written and read by the tree."""
    return (56 * L + 48) * npoin + 48 * L * nelem


def med(f, n=5):
    f()                                   # warm-up
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": n}


def measure(a):
    import numpy as np
    import torch
    from hnumo import regions as RG
    from hnumo import vorticity as V
    from hnumo.case import build_case, make_config
    from hnumo.engine import Engine
    rest = build_case(make_config(a.config))
    S, cfg = rest.scalars, rest.cfg
    e = Engine(rest)
    st = e.state()
    e.set_resident(True)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    npoin, L, ne = S["npoin"], S["nlayers"], S["nelem"]
    out = {"config": a.config, "nelem": ne, "npoin": npoin, "nlayers": L, "ngl": S["ngl"],
           "label": "launch overhead (625 elements)" if ne < 10000 else "bandwidth", "queue": QUEUE}
    f = V.coriolis_of(rest)
    torch.cuda.synchronize()

    def timed(sample):
        def single():
            sample()
            torch.cuda.synchronize()

        def queued():
            for _ in range(QUEUE):
                sample()
            torch.cuda.synchronize()
        q, s = med(queued), med(single)
        return {"queued_ms_per_sample": {k: (v / QUEUE if k.endswith("_ms") else v) for k, v in q.items()}, "single": s}

    nstrip = cfg["nely"]
    strips, R = RG.strips(rest, 1, np.linspace(cfg["ydims"][0], cfg["ydims"][1], nstrip + 1))
    assert R == nstrip and (np.bincount(strips, minlength=R + 1)[1:] == cfg["nelx"]).all() and not (strips == 0).any()
    out["nstrips"] = int(R)
    one = np.ones(ne, np.int32)
    for name, lab, nreg in (("one_region", one, 1), ("strips", strips, R)):
        for rows, tag in ((RG.FLOW, "flow"), (RG.VORT, "vort"), (RG.FLOW | RG.VORT, "both")):
            sid = e.regions_create(lab, nreg, rows, f, 0, CAP)
            c = timed(lambda: e.regions_sample(sid))
            c["tree_passes"] = 1 if max(np.bincount(lab)[1:]) <= 1024 else 2 if max(np.bincount(lab)[1:]) <= 1024 * 1024 else 3
            c["mask"] = int(rows)
            out[f"regions_{name}_{tag}"] = c
            e.regions_destroy(sid)
    e.stats_begin(0, CAP)
    out["stats_sample_series"] = timed(e.stats_accumulate)
    e.stats_end()
    e.vort_begin(f, 0, CAP)
    out["vort_sample_series"] = timed(e.vort_record)
    e.vort_end()
    e.close()
    nbytes = 1 << 31
    bw, variant = Engine.stream_copy_bw(0, nbytes, 10)
    out["stream_copy_GBps"] = bw
    out["stream_copy_how"] = f"hnumo_stream_copy_bw, {nbytes} bytes, 10 launches, variant {int(variant)}"
    derive(out)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def derive(out):
    """the byte counts and what follows from them and the measured times"""
    npoin, ne, L, bw = out["npoin"], out["nelem"], out["nlayers"], out["stream_copy_GBps"]
    for key, c in out.items():
        if key.startswith("regions_"):
            nb = region_bytes(npoin, ne, L, c["mask"])
        elif key == "stats_sample_series":
            nb = stats_bytes(npoin, ne, L)
        elif key == "vort_sample_series":
            nb = vort_bytes(npoin, ne, L)
        else:
            continue
        c["algorithmic_bytes"] = nb
        c["achieved_GBps"] = nb / (c["queued_ms_per_sample"]["median_ms"] * 1e-3) / 1e9
        c["fraction_of_stream_copy"] = c["achieved_GBps"] / bw
    t = lambda k: out[k]["queued_ms_per_sample"]["median_ms"]
    out["time_ratio_strips_to_one_region"] = {tag: t(f"regions_strips_{tag}") / t(f"regions_one_region_{tag}")
                                              for tag in ("flow", "vort", "both")}
    out["time_ratio_regions_vort_to_vort_series"] = t("regions_one_region_vort") / t("vort_sample_series")
    out["time_ratio_regions_flow_to_stats_series"] = t("regions_one_region_flow") / t("stats_sample_series")


def merge(a):
    res = {"what": "cost of a region set's sample (tools/regions_cost.py)", "cases": {}}
    for p in a.files:
        d = json.load(open(p))
        derive(d)                         # (from the measured times: the byte counts are this file's)
        res["cases"][d["config"]] = d
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("measure")
    p.add_argument("--config", default="dg25L3")
    p.add_argument("--out", default="regions_cost.json")
    p = sub.add_parser("merge")
    p.add_argument("files", nargs="+")
    p.add_argument("--out", required=True)
    a = ap.parse_args()
    {"measure": measure, "merge": merge}[a.cmd](a)
