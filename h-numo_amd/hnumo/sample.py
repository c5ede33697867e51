"""Sampling the solution at arbitrary points: the element's own Lagrange interpolant evaluated on a
regular output grid, a cross-section or a few stations, where the post-processing scripts
`griddata` the nodal values (Examples/double_gyre/compute_ssh.m:58-70, compute_ke.m, compute_eke.m,
plot_gyre.m, Examples/bump/plot_bump*.m, Examples/lake/plot_lake_2D.m).

    lagrange_weights  the 1-D weights of the definition
    HostSampler       the numpy statement of the definitions, fed with synced states on the host
    DeviceSampler     the same read-outs from the engine, which samples where the state lives
                      (kernels_sample.hip through hnumo_sample_*): no sync, and a series kept on the
                      device from every k-th step
    regular_grid      the meshgrid(xmin:dx:xmax, ymin:dy:ymax) of those scripts
    write_ssh_grid    compute_ssh.m's numoNNNN text format

Definitions (normative; include/hnumo_engine.h).  A sample set is M points, each
a 1-based local element `elem` (0: not on this rank) and reference coordinates (xi, eta) in
[-1,1]^2, with the 1-D LGL nodes xgl(ngl).  Weights: Lx[i] = l_i(xi) by w = 1.0; for m = 0..ngl-1,
m != i: w = w * ((xi - xgl[m]) / (xgl[i] - xgl[m])) -- each factor a quotient first, multiplied in
the order of m; Ly[j] from eta likewise.  Nodal fields of element e, node I = e*P + j*ngl + i:

    STATE  V = 5L + 4: rows 5k..5k+4 = layer k's h, u, v, dp, elevation as diagnostics.layer_fields
           forms them, rows 5L..5L+3 = qb_df(1:4, I)
    STATS  V = 5L: hbar, um, vm, mke, eke of flowstats' fields per layer
    VORT   V = 4L: zeta, delta, pv, ow of vorticity's fields per layer
    COV    V = 16L: the 16 fields of covariance's fields per layer

Value: val = sum_j Ly[j] * r_j with r_j = sum_i Lx[i] * F(e, j*ngl + i), both sums left to right
from their first product.  Points with elem = 0 read 0.0 in every row.  At xi = xgl[a], eta =
xgl[b] the weights are exactly 0 and 1 and the sample is the nodal value.  The two classes agree
bit for bit (tests/test_sample_gpu.py).
"""
from __future__ import annotations

import numpy as np

from . import basis as _basis
from . import diagnostics as _diag

STATE, STATS = 0, 1   # HNUMO_SAMPLE_STATE, HNUMO_SAMPLE_STATS
VORT = 2              # HNUMO_SAMPLE_VORT
COV = 3               # HNUMO_SAMPLE_COV
SOURCES = {"state": STATE, "stats": STATS, "vort": VORT, "cov": COV}


def source_id(source) -> int:
    """A source given by name ("state", "stats", "vort", "cov") or by its number."""
    return SOURCES[source] if isinstance(source, str) else int(source)


def lagrange_weights(xgl, x):
    """l_i(x), i = 0..ngl-1, on the nodes xgl: (ngl,) for a scalar x, (ngl, M) for x of shape (M,)."""
    xgl = np.asarray(xgl, dtype=np.float64).reshape(-1)
    xs = np.asarray(x, dtype=np.float64)
    xv = xs.reshape(-1)
    ngl = xgl.size
    out = np.zeros((ngl, xv.size))
    for i in range(ngl):
        w = np.ones(xv.size)
        for m in range(ngl):
            if m != i:
                w = w * ((xv - xgl[m]) / (xgl[i] - xgl[m]))
        out[i] = w
    return out[:, 0] if xs.ndim == 0 else out


def nval(nlayers: int, source: int) -> int:
    source = source_id(source)
    if source == COV:
        return 16 * nlayers
    return 4 * nlayers if source == VORT else 5 * nlayers if source == STATS else 5 * nlayers + 4


def case_xgl(case):
    """The 1-D LGL nodes of the case's elements (mod_basis xgl)."""
    return _basis.lgl(case.scalars["ngl"])[0]


def owned_elements(case) -> int:
    return int(getattr(case, "nelem_owned", 0) or case.scalars["nelem"])


class HostSampler:
    """The numpy mirror: M points (elem, xi, eta) of `case` (or of a rank's case of a partition).
    sample(q_df, qb_df) -> (5L + 4, M); sample_stats(fields) -> (5L, M) from flowstats' fields
    (5, npoin, L)."""

    def __init__(self, case, elem, xi, eta, source: int = STATE, xgl=None):
        S = case.scalars
        self.case, self.source = case, source_id(source)
        self.ngl, self.L, self.npoin = S["ngl"], S["nlayers"], S["npoin"]
        self.P = self.ngl ** 2
        self.elem = np.asarray(elem, dtype=np.int64).reshape(-1)
        self.xi = np.asarray(xi, dtype=np.float64).reshape(-1)
        self.eta = np.asarray(eta, dtype=np.float64).reshape(-1)
        self.M = self.elem.size
        if self.xi.size != self.M or self.eta.size != self.M:
            raise ValueError("elem, xi and eta must have one entry per point")
        if self.M < 1 or (self.elem < 0).any() or (self.elem > owned_elements(case)).any():
            raise ValueError("elem must lie in 0..nelem_owned (0: not on this rank)")
        if not (np.abs(self.xi) <= 1.0).all() or not (np.abs(self.eta) <= 1.0).all():
            raise ValueError("xi, eta must lie in [-1,1]")
        self.xgl = case_xgl(case) if xgl is None else np.asarray(xgl, dtype=np.float64).reshape(-1)
        self.Lx = lagrange_weights(self.xgl, self.xi)      # (ngl, M)
        self.Ly = lagrange_weights(self.xgl, self.eta)
        self.on = self.elem > 0
        self.node0 = np.where(self.on, self.elem - 1, 0) * self.P

    def _interp(self, F):
        """F: (V, npoin) nodal fields -> (V, M)."""
        ngl = self.ngl
        val = None
        for j in range(ngl):
            r = self.Lx[0] * F[:, self.node0 + j * ngl]
            for i in range(1, ngl):
                r = r + self.Lx[i] * F[:, self.node0 + j * ngl + i]
            val = self.Ly[0] * r if j == 0 else val + self.Ly[j] * r
        out = np.zeros((F.shape[0], self.M), order="F")
        out[:, self.on] = val[:, self.on]
        return out

    def _rows(self, f5):
        """(5, 4 or 16, npoin, L) -> (5L, 4L or 16L, npoin): layer after layer"""
        return np.concatenate([f5[:, :, k] for k in range(self.L)], axis=0)

    def sample_vort(self, fields):
        """(4L, M) from vorticity's fields (4, npoin, L) = HostVorticity.fields(q_df)."""
        return self._interp(self._rows(np.asarray(fields)))

    def sample(self, q_df, qb_df):
        with np.errstate(all="ignore"):                 # (nodes of ghost elements may hold anything)
            f5 = _diag.layer_fields(self.case, q_df)
        return self._interp(np.concatenate([self._rows(f5), np.asarray(qb_df)[0:4]], axis=0))

    def sample_stats(self, fields):
        return self._interp(self._rows(np.asarray(fields)))

    def sample_cov(self, fields):
        """(16L, M) from covariance's fields (16, npoin, L) = HostEddyCov.fields()."""
        return self._interp(self._rows(np.asarray(fields)))


class DeviceSampler:
    """The same read-outs from an hnumo.engine.Engine.  Give either xy (2, M) physical points, which
    the engine locates in its owned elements from the case's coord, or elem (M) with xi_eta (2, M)."""

    def __init__(self, engine, xy=None, elem=None, xi_eta=None, source: int = STATE, xgl=None, coord=None):
        source = source_id(source)
        self.engine, self.source = engine, source
        case = engine.case
        xgl = case_xgl(case) if xgl is None else xgl
        if xy is not None:
            coord = case.arrays["coord"] if coord is None else coord
            self.id = engine.sample_create(coord, xgl, xy, source)
        else:
            self.id = engine.sample_create_ref(xgl, elem, xi_eta, source)

    def plan(self):
        """(elem (M), xi (M), eta (M)) as the engine holds them."""
        elem, xe = self.engine.sample_plan(self.id)
        return elem, xe[0].copy(), xe[1].copy()

    def host_sampler(self):
        """The numpy mirror on this set's own plan."""
        return HostSampler(self.engine.case, *self.plan(), source=self.source)

    def sample(self, q_df=None, qb_df=None):
        """(V, M) of the state (or statistics) on the device now; the arguments are ignored."""
        return self.engine.sample(self.id)

    sample_stats = sample_cov = sample

    def series_begin(self, every: int = 0, capacity: int = 0):
        self.engine.sample_series_begin(self.id, every, capacity)

    def record(self):
        self.engine.sample_record(self.id)

    def series(self, clear: bool = False):
        return self.engine.sample_series(self.id, clear)

    def destroy(self):
        self.engine.sample_destroy(self.id)


def regular_grid(case, dx: float, dy: float):
    """(xi (nx,), yi (ny,), xy (2, nx*ny)) of meshgrid(xmin:dx:xmax, ymin:dy:ymax): xi[i] = xmin + i*dx
    while i*dx <= xmax - xmin, likewise yi; xmin..ymax from the owned nodes' coord.  xy is in
    MATLAB's column-major meshgrid order: point m = i*ny + j is (xi[i], yi[j])."""
    n = owned_elements(case) * case.scalars["ngl"] ** 2
    c = np.asarray(case.arrays["coord"])[0:2, :n]
    xmin, xmax, ymin, ymax = c[0].min(), c[0].max(), c[1].min(), c[1].max()

    def axis(lo, hi, d):
        if not d > 0:
            raise ValueError("regular_grid: dx and dy must be > 0")
        k = int(np.floor((hi - lo) / d))
        while (k + 1) * d <= hi - lo:
            k += 1
        while k > 0 and k * d > hi - lo:
            k -= 1
        return lo + np.arange(k + 1) * d

    xi, yi = axis(xmin, xmax, dx), axis(ymin, ymax, dy)
    X, Y = np.meshgrid(xi, yi)                      # (ny, nx), as MATLAB's
    xy = np.zeros((2, xi.size * yi.size), order="F")
    xy[0] = X.reshape(-1, order="F")
    xy[1] = Y.reshape(-1, order="F")
    return xi, yi, xy


def write_ssh_grid(path, xi, yi, ssh):
    """compute_ssh.m:68-70's numoNNNN file: '%23.16f\\n' per value -- the meshgrid arrays xi/1e3,
    then yi/1e3, then ssh, each (ny, nx) in MATLAB's column-major order.  xi (nx,), yi (ny,) are
    the axes; ssh is (ny, nx), or flat in that order."""
    xi, yi = np.asarray(xi, dtype=np.float64).reshape(-1), np.asarray(yi, dtype=np.float64).reshape(-1)
    X, Y = np.meshgrid(xi, yi)
    ssh = np.asarray(ssh, dtype=np.float64)
    if ssh.ndim == 2:
        if ssh.shape != X.shape:
            raise ValueError(f"ssh: shape {ssh.shape}, expected (ny, nx) = {X.shape}")
        ssh = ssh.reshape(-1, order="F")
    if ssh.size != X.size:
        raise ValueError(f"ssh: {ssh.size} values, expected {X.size}")
    with open(path, "w") as f:
        for a in (X.reshape(-1, order="F") / 1e3, Y.reshape(-1, order="F") / 1e3, ssh.reshape(-1)):
            f.write("".join("%23.16f\n" % v for v in a))
