"""Regional budgets: the integral series of PARTS of the domain -- subpolar against subtropical gyre, the
western boundary strip against the interior, zonal strips whose per-layer meridional transport, cumulated
over the layers, is the overturning streamfunction in layer space.

    HostRegions      the numpy statement of the definitions, fed with q_df arrays on the host
    DeviceRegions    the same read-outs from the engine, which reduces every region of a set at once where
                     the state lives (kernels_region.hip through hnumo_regions_*): no sync, nothing copied
                     per sample
    strips, boxes    labels from element centroids
    overturning      Psi_k(r) from a series of zonal strips

Definitions (normative; include/hnumo_engine.h, DESIGN.md §6.1.9, csrc/region_plan.h,
csrc/kernels_region.hip).  A region set labels every owned element with a region r in 0..R; label 0: the
element is in no region.  Up to REGION_MAXSETS = 4 sets exist at once (overlapping partitions, such as
strips and basins, are separate sets).  The members of region r, in ascending local element number, have
local positions 0..n_r-1.  IEEE double, no FMA, IEEE division; every sum left to right from its first
product.  Per member element e, layer k, node I = e*P + j*ngl + i, w_I the nodal jac:

    FLOW rows (mask bit 0), the statements of §6.1.1 (flowstats.py):
        dp = q(1); h = (alpha_k/gravity)*dp; u = q(2)/dp; v = q(3)/dp
        VOL_k = int h;  TU_k = int (u*h);  TV_k = int (v*h);  KE_k = int ((0.5*(u*u+v*v))*h)
    VORT rows (mask bit 1), the statements of §6.1.4 (vorticity.py); f the caller's coriolis_df, 0 for None:
        Z_k = int ((0.5*(zeta*zeta))*h);  PZ_k = int ((0.5*(pv*pv))*h);  G_k = int zeta

`int` in two steps: per element the products w_I*x_I added in node order from the first product; per region
the element sums combined by flowstats.tree_sum over the LOCAL POSITIONS.  An empty region reads +0.0 in
every row.  Ghost elements are never members.  Entry (V, R), V = 4L*[FLOW] + 3L*[VORT]: FLOW rows first,
4(k-1) + {0 VOL, 1 TU, 2 TV, 3 KE}, then the VORT rows, 3(k-1) + {0 Z, 1 PZ, 2 G}.  A set whose only region
holds all owned elements has the KE_k, VOL_k bits of flowstats' series and the Z_k, PZ_k, G_k bits of
vorticity's.  The two classes agree bit for bit (tests/test_regions_gpu.py).

Out of scope: labels per node (strips finer than an element; sample sets cover lines); fluxes across region
boundaries (they need the step's own face fluxes); combining ranks (the host adds them).
"""
from __future__ import annotations

import numpy as np

from .abi import REGION_FLOW, REGION_MAXSETS, REGION_VORT, region_rows
from .flowstats import tree_sum
from .vorticity import HostVorticity, coriolis_of

FLOW, VORT = REGION_FLOW, REGION_VORT
FLOW_NAMES = ("VOL", "TU", "TV", "KE")
VORT_NAMES = ("Z", "PZ", "G")


def rows_mask(rows) -> int:
    """A mask given as a number, or by name: "flow", "vort", "flow+vort" or "both"."""
    if isinstance(rows, str):
        return {"flow": FLOW, "vort": VORT, "flow+vort": FLOW | VORT, "both": FLOW | VORT}[rows]
    return int(rows)


def row_names(nlayers: int, rows) -> list:
    m = rows_mask(rows)
    out = [f"{n}{k + 1}" for k in range(nlayers) for n in FLOW_NAMES] if m & FLOW else []
    return out + ([f"{n}{k + 1}" for k in range(nlayers) for n in VORT_NAMES] if m & VORT else [])


def _owned(case) -> int:
    return int(getattr(case, "nelem_owned", 0) or case.scalars["nelem"])


def _check_labels(labels, R, ne, mask):
    lab = np.asarray(labels).reshape(-1)
    if int(R) < 1:
        raise ValueError(f"regions: nregions must be >= 1, got {R}")
    if lab.size != ne:
        raise ValueError(f"regions: {lab.size} labels, expected nelem_owned = {ne}")
    if mask == 0 or mask & ~(FLOW | VORT):
        raise ValueError(f"regions: rows must hold FLOW (1), VORT (2) or both, got {mask}")
    if lab.size and (lab.min() < 0 or lab.max() > R):
        raise ValueError(f"regions: labels must lie in 0..{R}")
    return lab.astype(np.int32)


def centroids(case):
    """(2, nelem_owned): the mean of each owned element's node coordinates."""
    ne, P = _owned(case), case.scalars["ngl"] ** 2
    c = np.asarray(case.arrays["coord"], dtype=np.float64)[0:2, :ne * P]
    return c.reshape(2, ne, P).mean(axis=2)


def strips(case, axis: int, edges):
    """Labels (nelem_owned) int32 and R = len(edges) - 1: region r holds the elements whose centroid
    coordinate along `axis` (0: x, zonal position; 1: y) lies in [edges[r-1], edges[r]); outside: 0."""
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    if edges.size < 2 or not (np.diff(edges) > 0).all():
        raise ValueError("strips: edges must ascend strictly and hold at least two values")
    c = centroids(case)[int(axis)]
    lab = np.searchsorted(edges, c, side="right")
    lab[(c < edges[0]) | (c >= edges[-1])] = 0
    return lab.astype(np.int32), edges.size - 1


def boxes(case, rects):
    """Labels (nelem_owned) int32 and R = len(rects): region r holds the elements whose centroid lies in
    rects[r-1] = (x0, x1, y0, y1), half-open [x0, x1) x [y0, y1); the first matching rectangle wins; none: 0."""
    c = centroids(case)
    lab = np.zeros(c.shape[1], dtype=np.int32)
    for r, (x0, x1, y0, y1) in enumerate(rects, start=1):
        hit = (lab == 0) & (c[0] >= x0) & (c[0] < x1) & (c[1] >= y0) & (c[1] < y1)
        lab[hit] = r
    return lab, len(rects)


def overturning(series, area, widths, nlayers=None):
    """Psi (L, R, count): Psi_k(r) = sum_{k' <= k} TV_k'(r) / dy_r, cumulated from the top layer down, of a
    FLOW series (V, R, count) over zonal strips of meridional widths `widths` (R,).  TV_k/dy_r is the strip's
    mean meridional transport across a line of latitude.  A strip of zero area reads 0."""
    s = np.asarray(series, dtype=np.float64)
    area = np.asarray(area, dtype=np.float64).reshape(-1)
    dy = np.asarray(widths, dtype=np.float64).reshape(-1)
    R = s.shape[1]
    if area.size != R or dy.size != R:
        raise ValueError(f"overturning: area and widths must hold R = {R} values")
    L = int(nlayers) if nlayers else (s.shape[0] // 4 if s.shape[0] % 7 else s.shape[0] // 7)
    if s.shape[0] not in (4 * L, 7 * L):
        raise ValueError(f"overturning: the series has {s.shape[0]} rows: it needs the FLOW rows of {L} layers")
    psi = np.zeros((L, R, s.shape[2]))
    acc = np.zeros((R, s.shape[2]))
    for k in range(L):
        acc = acc + s[4 * k + 2]
        psi[k] = np.where((area > 0)[:, None], acc / dy[:, None], 0.0)
    return psi


class HostRegions:
    """The numpy mirror.  case: a hnumo.case.Case (or a rank's case of a partition: only its owned elements
    count).  labels (nelem_owned) in 0..R; rows: FLOW, VORT or FLOW | VORT; coriolis as HostVorticity's
    (True: coriolis_of(case); False or None: 0; or an array (npoin))."""

    needs_host_state = True      # time_loop syncs a resident stepper before add(q)

    def __init__(self, case, labels, R: int, rows=FLOW, coriolis=None):
        A, S = case.arrays, case.scalars
        self.L, self.npoin, self.P = S["nlayers"], S["npoin"], S["ngl"] ** 2
        self.ne = _owned(case)
        self.nown = self.ne * self.P
        self.R, self.mask = int(R), rows_mask(rows)
        self.labels = _check_labels(labels, R, self.ne, self.mask)
        self.V = region_rows(self.L, self.mask)
        # region r's members in ascending element number: their order is their local position
        self.members = [np.flatnonzero(self.labels == r) for r in range(1, self.R + 1)]
        self.ag = [A["alpha"][k] / S["gravity"] for k in range(self.L)]
        self.w = np.asarray(A["jac"], dtype=np.float64).reshape(-1, order="F")[:self.nown]
        self.vort = HostVorticity(case, coriolis=coriolis, series=False) if self.mask & VORT else None
        self._series = []

    def _element(self, x):
        """per element the products w_I*x_I added in node order, from the first product"""
        return np.add.accumulate((self.w * np.asarray(x).reshape(-1)).reshape(self.ne, self.P), axis=1)[:, -1]

    def element_sums(self, q_df):
        """(V, ne): the element partials of every row, for all owned elements"""
        out = np.zeros((self.V, self.ne))
        o = slice(0, self.nown)
        row = 0
        if self.mask & FLOW:
            for k in range(self.L):
                dp = np.asarray(q_df[0, o, k], dtype=np.float64)
                h = self.ag[k] * dp
                u, v = q_df[1, o, k] / dp, q_df[2, o, k] / dp
                for x in (h, u * h, v * h, (0.5 * (u * u + v * v)) * h):
                    out[row] = self._element(x)
                    row += 1
        if self.mask & VORT:
            el = self.vort.element_sums(q_df)          # (3, L, ne)
            for k in range(self.L):
                out[row:row + 3] = el[:, k]
                row += 3
        return out

    def _reduce(self, el):
        e = np.zeros((el.shape[0], self.R), order="F")
        for r, m in enumerate(self.members):
            for v in range(el.shape[0]):
                e[v, r] = tree_sum(el[v, m])
        return e

    def entry(self, q_df):
        """(V, R) of the state."""
        return self._reduce(self.element_sums(q_df))

    def add(self, q_df):
        """One series sample of the state."""
        self._series.append(self.entry(q_df))

    @property
    def area(self):
        """(R,): sum of w_I per region, by the same per-element order and the same tree with x = 1.0."""
        return self._reduce(self._element(np.ones(self.nown))[None, :])[0]

    @property
    def series(self):
        """(V, R, count)."""
        out = np.zeros((self.V, self.R, len(self._series)), order="F")
        for i, e in enumerate(self._series):
            out[:, :, i] = e
        return out


class DeviceRegions:
    """The same read-outs from an hnumo.engine.Engine.  every = k >= 1: the engine samples itself after every
    k-th successful step (leave add() alone then); every = 0: add() takes a sample.  series: the number of
    samples the series can hold."""

    needs_host_state = False

    def __init__(self, engine, labels, R: int, rows=FLOW, coriolis=None, every: int = 0, series: int = 0):
        self.engine = engine
        self.R, self.mask = int(R), rows_mask(rows)
        if coriolis is True:
            f = coriolis_of(engine.case)
        elif coriolis is False or coriolis is None:
            f = None
        else:
            f = coriolis
        self.id = engine.regions_create(labels, self.R, self.mask, f, every, series)

    def add(self, q_df=None):
        """One sample of the state on the device (q_df is ignored; no sync)."""
        self.engine.regions_sample(self.id)

    @property
    def area(self):
        return self.engine.regions_area(self.id)

    @property
    def series(self):
        return self.engine.regions_series(self.id)

    def read(self, clear: bool = False):
        return self.engine.regions_series(self.id, clear=clear)

    def end(self):
        self.engine.regions_destroy(self.id)
