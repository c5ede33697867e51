"""Vorticity products of the layer velocity: relative vorticity, divergence, layer potential
vorticity and the Okubo-Weiss parameter, with the enstrophy, potential-enstrophy and circulation
series -- what a double-gyre or eddying run is judged by.  The reference stops short of them
(write_output.F90:32,41 allocates `vorticity` and never fills it; mod_gradient.F90 has no curl on the
MLSWE path), so the arithmetic is defined here.

    HostVorticity    the numpy statement of the definitions, fed with q_df arrays on the host
    DeviceVorticity  the same read-outs from the engine, which forms them where the state lives
                     (kernels_vort.hip through hnumo_vort_*): no sync, nothing copied per sample
    coriolis_of      coriolis_df(npoin) of a case (or of a rank's case of a partition)

Definitions (normative; include/hnumo_engine.h).  Owned element e, layer k, node
(i, j), I = e*P + j*ngl + i, every sum left to right from its first product:

    dp = q(1,I,k); h = (alpha_k/gravity)*dp; u = q(2,I,k)/dp; v = q(3,I,k)/dp
    D(m,i) = dpsi[m, i] = l_m'(xgl_i)
    u_xi = sum_m D(m,i)*u(m,j);  u_eta = sum_m D(m,j)*u(i,m)          (v likewise)
    u_x = u_xi*ksi_x + u_eta*eta_x;  u_y = u_xi*ksi_y + u_eta*eta_y   (v likewise)
    zeta = v_x - u_y;  delta = u_x + v_y;  pv = (zeta + f)/h
    sn = u_x - v_y;  ss = v_x + u_y;  ow = (sn*sn + ss*ss) - zeta*zeta

This is the element's own (broken) gradient: no face terms, nothing crosses an element, and jumps at
element edges are not lifted.  Fields (4,npoin,L) = zeta, delta, pv, ow.  Series (3,L,count):
Z_k = integral of (0.5*(zeta*zeta))*h, PZ_k = integral of (0.5*(pv*pv))*h, G_k = integral of zeta over
the owned elements -- per element the products jac_I*x_I added in node order, the element sums
combined by flowstats.tree_sum.  Nodes of ghost elements are never formed and read 0.  The two
classes agree bit for bit (tests/test_vort_gpu.py).
"""
from __future__ import annotations

import numpy as np

from .flowstats import tree_sum

FIELD_NAMES = ("zeta", "delta", "pv", "ow")
SERIES_NAMES = ("enstrophy", "potential_enstrophy", "circulation")


def coriolis_of(case):
    """coriolis_df(npoin) = f0 + beta*(y - ym) (mod_initial_mlswe.F90:280-352): the case's own array,
    or the same statement on a rank's coord."""
    A, cfg = case.arrays, case.cfg
    if "coriolis_df" in A:
        return np.asarray(A["coriolis_df"], dtype=np.float64).reshape(-1)
    y = np.asarray(A["coord"])[1]
    return np.asarray(cfg["f0"] + cfg["beta"] * (y - 0.5 * cfg["ydims"][1]), dtype=np.float64)


def _node_order(a, nown):
    return np.asarray(a, dtype=np.float64).reshape(-1, order="F")[:nown]


class HostVorticity:
    """The numpy mirror.  case: a hnumo.case.Case (or a rank's case of a partition: only its owned
    elements count).  coriolis: True -- f = coriolis_of(case); False or None -- f = 0; or an array
    (npoin).  series=False skips the series."""

    needs_host_state = True      # time_loop syncs a resident stepper before add(q)

    def __init__(self, case, coriolis=True, series: bool = True):
        A, S = case.arrays, case.scalars
        self.L, self.npoin, self.ngl = S["nlayers"], S["npoin"], S["ngl"]
        self.P = self.ngl ** 2
        self.ne = int(getattr(case, "nelem_owned", 0) or S["nelem"])
        self.nown = self.ne * self.P
        self.ag = [A["alpha"][k] / S["gravity"] for k in range(self.L)]
        self.D = np.asarray(A["dpsi"], dtype=np.float64)
        shp = (self.ne, self.ngl, self.ngl)                     # [e, j, i]
        self.ex, self.ey, self.nx, self.ny = (_node_order(A[k], self.nown).reshape(shp)
                                              for k in ("ksi_x", "ksi_y", "eta_x", "eta_y"))
        self.w = _node_order(A["jac"], self.nown)
        if coriolis is True:
            f = coriolis_of(case)
        elif coriolis is False or coriolis is None:
            f = np.zeros(self.npoin)
        else:
            f = np.asarray(coriolis, dtype=np.float64).reshape(-1)
        if f.size != self.npoin:
            raise ValueError(f"coriolis: {f.size} values, expected npoin = {self.npoin}")
        self.f = f[:self.nown].reshape(shp)
        self._series = [] if series else None

    def _grad(self, a):
        """(a_xi, a_eta) of a[e, j, i]: the ordered sums over m"""
        D = self.D
        a_xi = D[0, :][None, None, :] * a[:, :, 0:1]
        a_eta = D[0, :][None, :, None] * a[:, 0:1, :]
        for m in range(1, self.ngl):
            a_xi = a_xi + D[m, :][None, None, :] * a[:, :, m:m + 1]
            a_eta = a_eta + D[m, :][None, :, None] * a[:, m:m + 1, :]
        return a_xi, a_eta

    def _layer(self, q_df, k):
        """(zeta, delta, pv, ow, h) of layer k on the owned nodes, each [e, j, i]"""
        shp = (self.ne, self.ngl, self.ngl)
        o = slice(0, self.nown)
        dp = np.asarray(q_df[0, o, k], dtype=np.float64).reshape(shp)
        h = self.ag[k] * dp
        u = np.asarray(q_df[1, o, k]).reshape(shp) / dp
        v = np.asarray(q_df[2, o, k]).reshape(shp) / dp
        u_xi, u_eta = self._grad(u)
        v_xi, v_eta = self._grad(v)
        u_x = u_xi * self.ex + u_eta * self.nx
        u_y = u_xi * self.ey + u_eta * self.ny
        v_x = v_xi * self.ex + v_eta * self.nx
        v_y = v_xi * self.ey + v_eta * self.ny
        zeta = v_x - u_y
        delta = u_x + v_y
        pv = (zeta + self.f) / h
        sn, ss = u_x - v_y, v_x + u_y
        ow = (sn * sn + ss * ss) - zeta * zeta
        return zeta, delta, pv, ow, h

    def fields(self, q_df):
        """(4, npoin, L) = zeta, delta, pv, ow of the state q_df(3,npoin,L); 0 at ghost nodes."""
        out = np.zeros((4, self.npoin, self.L), order="F")
        for k in range(self.L):
            for c, x in enumerate(self._layer(q_df, k)[:4]):
                out[c, :self.nown, k] = x.reshape(-1)
        return out

    def element_sums(self, q_df):
        """(3, L, ne): per element the products jac_I*x_I of Z, PZ, G added in node order from the
        first product -- what tree_sum combines into an entry of the series."""
        out = np.zeros((3, self.L, self.ne))
        for k in range(self.L):
            zeta, _, pv, _, h = self._layer(q_df, k)
            for c, x in enumerate(((0.5 * (zeta * zeta)) * h, (0.5 * (pv * pv)) * h, zeta)):
                out[c, k] = np.add.accumulate((self.w * x.reshape(-1)).reshape(self.ne, self.P), axis=1)[:, -1]
        return out

    def entry(self, q_df):
        """(3, L) = Z_k, PZ_k, G_k of the state."""
        el = self.element_sums(q_df)
        e = np.zeros((3, self.L), order="F")
        for k in range(self.L):
            for c in range(3):
                e[c, k] = tree_sum(el[c, k])
        return e

    def add(self, q_df):
        """One series sample of the state."""
        if self._series is not None:
            self._series.append(self.entry(q_df))

    @property
    def series(self):
        """(3, L, count): Z_k, PZ_k, G_k per sample."""
        s = self._series or []
        out = np.zeros((3, self.L, len(s)), order="F")
        for i, e in enumerate(s):
            out[:, :, i] = e
        return out


class DeviceVorticity:
    """The same read-outs from an hnumo.engine.Engine.  every = k >= 1: the engine takes a series
    sample itself after every k-th successful step (leave add() alone then); every = 0: add() takes
    one.  series: the number of samples the series can hold (0: none).  coriolis as HostVorticity's."""

    needs_host_state = False

    def __init__(self, engine, every: int = 0, series: int = 0, coriolis=True):
        self.engine = engine
        if coriolis is True:
            f = coriolis_of(engine.case)
        elif coriolis is False or coriolis is None:
            f = None
        else:
            f = coriolis
        engine.vort_begin(f, every, series)

    def fields(self, q_df=None):
        """(4, npoin, L) of the state on the device now (q_df is ignored)."""
        return self.engine.vort_fields()

    def add(self, q_df=None):
        """One series sample of the state on the device (q_df is ignored; no sync)."""
        self.engine.vort_record()

    @property
    def series(self):
        return self.engine.vort_series()

    def end(self):
        self.engine.vort_end()
