#!/usr/bin/env python3
"""Closure of the energy budget (hnumo/energy.py), reported and not a test: DESIGN.md §6.1.8.

    python tools/energy_budget.py [--config dg25L3] [--nelx 8 --nely 8] [--seconds 60] [--out budget.json]

Runs the CPU oracle on a small wind-driven case from rest for as many steps as fit in about --seconds, with
HostEnergy sampling every step (zref: the rest elevations).  With E_n = sum_k (KE_k + APE_k) after step n it
prints E_n - E_0 beside dt * sum_{i=1..n} (W - D - sum_k V_k)_i, the right-endpoint sum of the sampled rates,
and beside the trapezoidal sum.  The mirror is the code under test, so it cannot be its own judge: the
residual is a figure, not an assertion.  It contains the numerical dissipation of the face fluxes, the LDG
face terms eps leaves out, the splitting's time-averaged drag (the model's drag acts on the sub-cycle's
averaged barotropic state, D on the layer state q), and the KE<->APE conversion only in so far as the
discrete pressure work and thickness flux do not cancel.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "h-numo_amd"), os.path.join(REPO, "oracle")):
    sys.path.insert(0, p)


def main(a):
    import oracle as O
    from hnumo import covariance as CV
    from hnumo import energy as EN
    from hnumo.case import build_case, make_config
    case = build_case(make_config(a.config, nelx=a.nelx, nely=a.nely))
    S = case.scalars
    L, dt = S["nlayers"], S["dt"]
    he = EN.HostEnergy(case, zref=CV.rest_elevations(case))
    o = O.Oracle(case)
    q, qb, qp = o.state()
    he.add(q)                                   # E_0 and the rates at rest
    t0 = time.time()
    n = 0
    while time.time() - t0 < a.seconds and n < a.max_steps:
        o.ti_rk_bcl(q, qb, qp)
        he.add(q)
        n += 1
    ser = he.series()
    E = ser[:2 * L].sum(axis=0)
    rate = ser[3 * L] - ser[3 * L + 1] - ser[2 * L:3 * L].sum(axis=0)
    right = dt * np.cumsum(rate[1:])
    trap = dt * np.cumsum(0.5 * (rate[1:] + rate[:-1]))
    dE = E[1:] - E[0]
    out = {"config": a.config, "nelx": a.nelx, "nely": a.nely, "ngl": S["ngl"], "nlayers": L, "dt": dt, "steps": n,
           "botfr": S["botfr"], "cd": S["cd"], "visc": S["visc"],
           "E0": float(E[0]), "dE": float(dE[-1]), "dKE": float(ser[:L, -1].sum() - ser[:L, 0].sum()),
           "dAPE": float(ser[L:2 * L, -1].sum() - ser[L:2 * L, 0].sum()),
           "dt_sum_W": float(dt * ser[3 * L, 1:].sum()), "dt_sum_D": float(dt * ser[3 * L + 1, 1:].sum()),
           "dt_sum_V": float(dt * ser[2 * L:3 * L, 1:].sum()),
           "dt_sum_rates_right": float(right[-1]), "dt_sum_rates_trapezoid": float(trap[-1]),
           "residual_right": float(dE[-1] - right[-1]), "residual_trapezoid": float(dE[-1] - trap[-1]),
           "residual_over_dt_sum_W": float((dE[-1] - trap[-1]) / (dt * ser[3 * L, 1:].sum()))}
    print(f"{'step':>6s} {'E_n - E_0':>16s} {'dt*sum(W-D-V)':>16s} {'trapezoid':>16s}")
    for i in sorted(set(list(range(0, n, max(1, n // 10))) + [n - 1])):
        print(f"{i + 1:6d} {dE[i]:16.8e} {right[i]:16.8e} {trap[i]:16.8e}")
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="dg25L3")
    ap.add_argument("--nelx", type=int, default=8)
    ap.add_argument("--nely", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--max-steps", type=int, default=100000)
    ap.add_argument("--out", default="")
    main(ap.parse_args())
