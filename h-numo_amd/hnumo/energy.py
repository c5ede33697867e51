"""Energy budget: the power the wind puts into the top layer, the power the bottom drag removes, the
interior viscous dissipation, and the kinetic and available potential energy these change -- products of
fields that decorrelate within a few steps, formed at the quadrature points where the model applies its
forcing and accumulated sample by sample instead of from snapshots.

    HostEnergy    the numpy statement of the definitions, fed with q_df arrays (and the wind) on the host
    DeviceEnergy  the same read-outs from the engine, which samples where the state and the wind live
                  (kernels_energy.hip through hnumo_energy_*): no sync, nothing copied per sample
    quad_coords   the node coordinates interpolated to the quad points, for plotting the quad maps

Definitions (normative; include/hnumo_engine.h, csrc/energy_plan.h; IEEE double, no FMA,
every sum left to right from its first product).  Owned element e, nodes I = e*P + j*ngl + i, quad points
Iq = e*Q + jq*nq + iq (nq = 2*ngl - 1), w_I the nodal jac, wq_Iq the quad weight wjac, tau(1:2,Iq) the wind
at the time of the sample.  At the nodes, per layer k:

    dp = q(1,I,k);  u = q(2,I,k)/dp;  v = q(3,I,k)/dp;  m = dp/gravity            (mass per area)
    ke_k  = (0.5*(u*u + v*v))*m
    z_k   = elevation of layer k's top interface as diagnostics.layer_fields forms it (row 5)
    d_k   = z_k - zref(I,k)                                   (zref given at begin; None: 0.0)
    c_1   = 0.5*(gravity*(1.0/alpha_1));  c_k = 0.5*(gravity*(1.0/alpha_k - 1.0/alpha_(k-1)))  (k >= 2)
    ape_k = c_k*(d_k*d_k)
    u_x,u_y,v_x,v_y = the element's own gradient, the statements of vorticity.HostVorticity
    eps_k = (visc_mlswe*((u_x*u_x + u_y*u_y) + (v_x*v_x + v_y*v_y)))*m

At the quad points a nodal field a(i,j) is interpolated in two passes, in this order:

    t(iq,n)  = psiq(1,iq)*a(1,n);  for m = 2..ngl: t = t + psiq(m,iq)*a(m,n)
    A(iq,jq) = psiq(1,jq)*t(iq,1); for n = 2..ngl: A = A + psiq(n,jq)*t(iq,n)

applied to u_1, v_1 (top layer) and u_L, v_L, dp_L (bottom layer): U1, V1, UL, VL, DPL.  Then

    W = tau(1,Iq)*U1 + tau(2,Iq)*V1
    botfr == 0:  D = +0.0
    botfr == 1:  spd = (cd_mlswe/gravity)*DPL
    botfr == 2:  spd = (cd_mlswe/alpha_L)*sqrt(UL*UL + VL*VL)
                 tb_u = spd*UL;  tb_v = spd*VL;  D = tb_u*UL + tb_v*VL

tau and tb are stresses (mod_rhs_btp.F90:171, d(u dp)/dt = gravity*(tau - tb) + ...), m = dp/g is mass per
area: W, D and eps are W/m^2, and d(sum KE + sum APE)/dt ~ W - D - sum V.  One sample adds W, D to the sums
S_W, S_D (2,npoin_q) and eps_k to S_V (npoin,L), in sample order from +0.0; with a series it appends the
3L+2 integrals KE_1..L, APE_1..L, V_1..L, W, D over the owned elements -- per element the products jac_I*x_I
in node order (wjac_Iq*x_Iq in quad order) from the first, the element sums combined by
flowstats.tree_sum.  Ghost elements are never visited and read 0.  The two classes agree bit for bit
(tests/test_energy_gpu.py).

What the terms are not: the drag law is evaluated on the layer state q, not on the sub-cycle's (qb, qprime)
split or its time average; the wind is credited to the top layer; eps is the interior estimate, without the
LDG face terms; the KE<->APE conversion is not formed.  The budget closes to discretisation error, not to
bits (tools/energy_budget.py).
"""
from __future__ import annotations

import numpy as np

from .covariance import _zref_arg, elevations
from .flowstats import tree_sum
from .vorticity import HostVorticity


def series_names(L: int):
    return tuple(f"{n}_{k + 1}" for n in ("KE", "APE", "V") for k in range(L)) + ("W", "D")


def _psiq(case):
    return np.asarray(case.arrays["psiq"], dtype=np.float64)          # psiq[m, iq]


def _to_quad(psiq, a):
    """a[e, n, m] (node (i = m, j = n)) -> A[e, jq, iq]: the two passes, each sum in order."""
    ngl = psiq.shape[0]
    t = psiq[0][None, None, :] * a[:, :, 0:1]                          # t[e, n, iq]
    for m in range(1, ngl):
        t = t + psiq[m][None, None, :] * a[:, :, m:m + 1]
    A = psiq[0][None, :, None] * t[:, 0:1, :]                          # A[e, jq, iq]
    for n in range(1, ngl):
        A = A + psiq[n][None, :, None] * t[:, n:n + 1, :]
    return A


def quad_coords(case):
    """(2, npoin_q): the node coordinates x, y interpolated to the quad points of every element."""
    S = case.scalars
    ngl, ne = S["ngl"], S["nelem"]
    xy = np.asarray(case.arrays["coord"], dtype=np.float64)
    out = np.zeros((2, S["npoin_q"]), order="F")
    for c in range(2):
        out[c] = _to_quad(_psiq(case), xy[c].reshape(ne, ngl, ngl)).reshape(-1)
    return out


class HostEnergy:
    """The numpy mirror.  case: a hnumo.case.Case (or a rank's case of a partition: only its owned elements
    count).  zref: (npoin, L), or None: 0.  series=False keeps the sums only."""

    needs_host_state = True      # time_loop syncs a resident stepper before add(q)

    def __init__(self, case, zref=None, series: bool = True):
        self.case = case
        self.hv = HostVorticity(case, coriolis=False, series=False)       # the one gradient
        hv = self.hv
        A, S = case.arrays, case.scalars
        self.L, self.npoin, self.ngl, self.P, self.ne, self.nown = hv.L, hv.npoin, hv.ngl, hv.P, hv.ne, hv.nown
        self.nq = S["nq"]
        if self.nq != 2 * self.ngl - 1:
            raise ValueError(f"nq = {self.nq}, expected 2*ngl - 1 = {2 * self.ngl - 1}")
        self.Q, self.npq = self.nq ** 2, S["npoin_q"]
        self.nqown = self.ne * self.Q
        self.g, self.cd, self.visc, self.botfr = S["gravity"], S["cd"], S["visc"], int(S["botfr"])
        if self.botfr not in (0, 1, 2):
            raise ValueError(f"botfr = {self.botfr}, expected 0, 1 or 2")
        self.alpha = [float(a) for a in np.asarray(A["alpha"]).reshape(-1)[:self.L]]
        self.c = [0.5 * (self.g * (1.0 / self.alpha[0]))] + \
                 [0.5 * (self.g * (1.0 / self.alpha[k] - 1.0 / self.alpha[k - 1])) for k in range(1, self.L)]
        self.w = hv.w
        self.wq = np.asarray(A["jacq"], dtype=np.float64).reshape(-1, order="F")[:self.nqown]
        self.psiq = _psiq(case)
        z = _zref_arg(zref, self.npoin, self.L)
        self.zref = np.zeros((self.npoin, self.L), order="F") if z is None else z
        self._quad = np.zeros((2, self.npq), order="F")
        self._nodal = np.zeros((self.npoin, self.L), order="F")
        self.nsamples = 0
        self._series = [] if series else None
        self.partials = None         # (3L+2, ne) of the last sample with a series

    def terms(self, q_df, tau=None):
        """(ke, ape, eps: each (L, nown); W, D: each (nqown)) of the state q_df under the wind tau(2, npoin_q)."""
        o = slice(0, self.nown)
        shp = (self.ne, self.ngl, self.ngl)
        tau = np.asarray(self.case.arrays["tau_wind"] if tau is None else tau, dtype=np.float64)
        if tau.shape != (2, self.npq):
            raise ValueError(f"tau: shape {tau.shape}, expected (2, npoin_q) = (2, {self.npq})")
        elev = elevations(self.case, q_df)
        hv, L = self.hv, self.L
        ke, ape, eps = (np.zeros((L, self.nown)) for _ in range(3))
        uv = []
        for k in range(L):
            dp = np.asarray(q_df[0, o, k], dtype=np.float64)
            u, v = q_df[1, o, k] / dp, q_df[2, o, k] / dp
            m = dp / self.g
            ke[k] = (0.5 * (u * u + v * v)) * m
            d = elev[o, k] - self.zref[o, k]
            ape[k] = self.c[k] * (d * d)
            u3, v3 = u.reshape(shp), v.reshape(shp)
            u_xi, u_eta = hv._grad(u3)
            v_xi, v_eta = hv._grad(v3)
            u_x, u_y = u_xi * hv.ex + u_eta * hv.nx, u_xi * hv.ey + u_eta * hv.ny
            v_x, v_y = v_xi * hv.ex + v_eta * hv.nx, v_xi * hv.ey + v_eta * hv.ny
            eps[k] = ((self.visc * ((u_x * u_x + u_y * u_y) + (v_x * v_x + v_y * v_y))) * m.reshape(shp)).reshape(-1)
            uv.append((u3, v3, dp.reshape(shp)))
        qo = slice(0, self.nqown)
        U1, V1 = (_to_quad(self.psiq, a).reshape(-1) for a in uv[0][:2])
        W = tau[0, qo] * U1 + tau[1, qo] * V1
        if self.botfr == 0:
            D = np.zeros(self.nqown)
        else:
            UL, VL, DPL = (_to_quad(self.psiq, a).reshape(-1) for a in uv[L - 1])
            spd = (self.cd / self.g) * DPL if self.botfr == 1 else (self.cd / self.alpha[L - 1]) * np.sqrt(UL * UL + VL * VL)
            tb_u, tb_v = spd * UL, spd * VL
            D = tb_u * UL + tb_v * VL
        return ke, ape, eps, W, D

    def add(self, q_df, tau=None):
        """One sample.  tau (2, npoin_q): the wind of the step that made q_df; None: the case's tau_wind."""
        ke, ape, eps, W, D = self.terms(q_df, tau)
        o, qo = slice(0, self.nown), slice(0, self.nqown)
        self._quad[0, qo] = self._quad[0, qo] + W
        self._quad[1, qo] = self._quad[1, qo] + D
        for k in range(self.L):
            self._nodal[o, k] = self._nodal[o, k] + eps[k]
        self.nsamples += 1
        if self._series is not None:
            # per element in node (quad) order, from the first product
            el = lambda wx, n: np.add.accumulate(wx.reshape(self.ne, n), axis=1)[:, -1]
            rows = [el(self.w * x[k], self.P) for x in (ke, ape, eps) for k in range(self.L)]
            rows += [el(self.wq * W, self.Q), el(self.wq * D, self.Q)]
            self.partials = np.array(rows)
            self._series.append(np.array([tree_sum(r) for r in rows]))

    def series(self):
        """(3L+2, count): KE_1..L, APE_1..L, V_1..L, W, D per sample."""
        if self._series is None:
            raise ValueError("energy budget: no series")
        out = np.zeros((3 * self.L + 2, len(self._series)), order="F")
        for i, e in enumerate(self._series):
            out[:, i] = e
        return out

    def sums(self):
        """(quad (2, npoin_q) = S_W, S_D; nodal (npoin, L) = S_V; the sample count)."""
        return self._quad.copy(order="F"), self._nodal.copy(order="F"), self.nsamples

    def set_sums(self, quad, nodal, nsamples: int):
        a, b = np.array(quad, dtype=np.float64, order="F"), np.array(nodal, dtype=np.float64, order="F")
        if a.shape != self._quad.shape or b.shape != self._nodal.shape:
            raise ValueError(f"sums: shapes {a.shape}, {b.shape}, expected {self._quad.shape}, {self._nodal.shape}")
        if int(nsamples) < 0:
            raise ValueError("nsamples must be >= 0")
        self._quad, self._nodal, self.nsamples = a, b, int(nsamples)

    def means(self):
        """(quad (2, npoin_q) = S_W/N, S_D/N; nodal (npoin, L) = S_V/N)."""
        if self.nsamples == 0:
            raise ValueError("energy budget: no samples yet")
        N = float(self.nsamples)
        return np.asfortranarray(self._quad / N), np.asfortranarray(self._nodal / N)


class DeviceEnergy:
    """The same read-outs from an hnumo.engine.Engine.  every = k >= 1: the engine samples itself after
    every k-th successful step (leave add() alone then); every = 0: add() takes a sample.  series: the
    number of samples the series can hold (0: sums only).  zref as HostEnergy's."""

    needs_host_state = False

    def __init__(self, engine, zref=None, every: int = 0, series: int = 0):
        self.engine = engine
        engine.energy_begin(zref, every, series)

    def add(self, q_df=None, tau=None):
        """One sample of the state and the wind on the device (q_df and tau are ignored; no sync)."""
        self.engine.energy_sample()

    def series(self, clear: bool = False):
        return self.engine.energy_series(clear)

    def sums(self):
        return self.engine.energy_sums()

    @property
    def nsamples(self) -> int:
        return self.engine.energy_sums()[2]

    def set_sums(self, quad, nodal, nsamples: int):
        self.engine.energy_set_sums(quad, nodal, nsamples)

    def means(self):
        return self.engine.energy_means()

    def end(self):
        self.engine.energy_end()
