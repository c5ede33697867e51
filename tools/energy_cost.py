"""Cost of the energy budget (kernels_energy.hip, hnumo_energy_*), DESIGN.md §6.1.8.

    python tools/energy_cost.py measure --config dg25L3 --out cost_dg25L3.json
        resident engine, two steps taken: the time of one sample of energy_sample_kernel with the series
        (the kernel and the tree's launches) and without it and, in the same run, of stats_accumulate_kernel
        (series off), each two ways -- `queued`: QUEUE samples launched
        back to back and one device synchronise, divided by QUEUE (the kernels run one after the other
        on the engine stream, so the launch overhead is hidden behind the kernel before: the kernel
        time); `single`: one sample and a synchronise (what a caller who waits sees) -- median of 5 after
        a warm-up; the bytes a sample moves, the stream-copy rate of the same run, the fraction of it
        each kernel reaches and the ratio of the samples.
    python tools/energy_cost.py merge --out energy_cost.json cost_*.json
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


def energy_bytes(npoin: int, npq: int, L: int, series: bool) -> int:
    """energy_sample_kernel per launch.  Per node and layer: q read (24), S_V read and written (16); per node the
    four metric rows (32).  Per quad point: the wind (16), (S_W, S_D) read and written (32).  With the series:
    zref per node and layer (8), jac and zbot per node (16), wjac per quad point (8)."""
    nodal = (24 + 16 + (8 if series else 0)) * L + 32 + (16 if series else 0)
    return nodal * npoin + (48 + (8 if series else 0)) * npq


def stats_bytes(npoin: int, L: int) -> int:
    """stats_accumulate_kernel per launch, series off: per node and layer q read (24), the four sums
    read and written (64)."""
    return (24 + 64) * L * npoin


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
    from hnumo import covariance as CV
    from hnumo.case import build_case, make_config
    from hnumo.engine import Engine
    rest = build_case(make_config(a.config))
    S = rest.scalars
    e = Engine(rest)
    st = e.state()
    e.set_resident(True)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    npoin, L = S["npoin"], S["nlayers"]
    out = {"config": a.config, "nelem": S["nelem"], "npoin": npoin, "npoin_q": S["npoin_q"], "nlayers": L, "ngl": S["ngl"],
           "botfr": S["botfr"],
           "label": "launch overhead (625 elements)" if S["nelem"] < 10000 else "bandwidth", "queue": QUEUE}
    e.stats_begin(0, 0)
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

    e.energy_begin(CV.rest_elevations(rest), 0, 2 * 6 * (QUEUE + 1))
    out["energy_sample_series"] = timed(e.energy_sample)
    e.energy_begin(CV.rest_elevations(rest), 0, 0)
    out["energy_sample"] = timed(e.energy_sample)
    out["stats_sample"] = timed(e.stats_accumulate)
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
    npoin, npq, L, bw = out["npoin"], out["npoin_q"], out["nlayers"], out["stream_copy_GBps"]
    for key, nb in (("energy_sample_series", energy_bytes(npoin, npq, L, True)), ("energy_sample", energy_bytes(npoin, npq, L, False)),
                    ("stats_sample", stats_bytes(npoin, L))):
        c = out[key]
        c["algorithmic_bytes"] = nb
        c["achieved_GBps"] = nb / (c["queued_ms_per_sample"]["median_ms"] * 1e-3) / 1e9
        c["fraction_of_stream_copy"] = c["achieved_GBps"] / bw
    out["bytes_per_node"] = {"per node and layer": 40, "per node": 32, "series: per node and layer": 8, "series: per node": 16}
    out["bytes_per_quad_point"] = {"always": 48, "series": 8}
    out["bytes_ratio_energy_to_stats"] = energy_bytes(npoin, npq, L, False) / stats_bytes(npoin, L)
    out["time_ratio_energy_to_stats"] = (out["energy_sample"]["queued_ms_per_sample"]["median_ms"] /
                                         out["stats_sample"]["queued_ms_per_sample"]["median_ms"])


def merge(a):
    res = {"what": "cost of the energy budget (tools/energy_cost.py)", "cases": {}}
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
    p.add_argument("--out", default="energy_cost.json")
    p = sub.add_parser("merge")
    p.add_argument("files", nargs="+")
    p.add_argument("--out", required=True)
    a = ap.parse_args()
    {"measure": measure, "merge": merge}[a.cmd](a)
