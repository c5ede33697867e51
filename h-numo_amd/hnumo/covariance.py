"""Eddy covariances: the thickness-weighted Reynolds stresses (the EKE is half their trace), the eddy
thickness flux (bolus transport), the interface and SSH variance, the eddy potential-vorticity flux and
the eddy potential enstrophy -- covariances of fields that decorrelate within a few steps, accumulated
sample by sample instead of from snapshots.

    HostEddyCov    the numpy statement of the definitions, fed with q_df arrays on the host
    DeviceEddyCov  the same read-outs from the engine, which accumulates where the state lives
                   (kernels_cov.hip through hnumo_cov_*): no sync, nothing copied per sample
    rest_elevations  zref(npoin,L) of a case's own (rest) state

Definitions (normative; include/hnumo_engine.h; every sum left to right, no FMA).
Per owned node I of element e and layer k, per sample:

    dp, h, u, v        as flowstats / vorticity form them (h = (alpha_k/gravity)*dp, quotient first;
                       u = q2/dp; v = q3/dp)
    z                  = elevation of layer k's top interface as diagnostics.layer_fields forms it (row 5;
                         summed upward from zbot_df)
    d                  = z - zref(I,k)                  (zref given at begin, None: 0.0)
    zeta, pv           = zeta and pv of vorticity.HostVorticity for this node and layer (f as given, None: 0.0)
    a                  = zeta + f(I)

One sample adds these 14 terms to running sums (14,npoin,L), in sample order from +0.0:

    S_h  += h        S_u  += u          S_v  += v
    S_uh += u*h      S_vh += v*h
    S_uuh += (u*u)*h S_uvh += (u*v)*h   S_vvh += (v*v)*h
    S_d  += d        S_dd += d*d
    S_a  += a        S_ua += u*a        S_va += v*a        S_qa += pv*a

Fields (16,npoin,L) after n samples, N = float(n):

    hbar = S_h/N   ubar = S_u/N   vbar = S_v/N   um = S_uh/S_h   vm = S_vh/S_h
    Ruu = S_uuh/S_h - um*um    Ruv = S_uvh/S_h - um*vm    Rvv = S_vvh/S_h - vm*vm
    Fu  = S_uh/N - ubar*hbar   Fv  = S_vh/N - vbar*hbar
    dbar = S_d/N               dvar = S_dd/N - dbar*dbar
    qm  = S_a/S_h              Qu  = S_ua/S_h - um*qm     Qv = S_va/S_h - vm*qm
    ens = 0.5*(S_qa/S_h - qm*qm)

Integrals (3,L): of hbar*(0.5*(Ruu+Rvv)), of dvar and of hbar*ens over the owned elements -- per element
the products jac_I*x_I added in node order from the first, the element sums combined by
flowstats.tree_sum.  Nodes of ghost elements are never accumulated and read 0.  The two classes agree
bit for bit (tests/test_cov_gpu.py).
"""
from __future__ import annotations

import numpy as np

from . import diagnostics as _diag
from .flowstats import tree_sum
from .vorticity import HostVorticity, coriolis_of

SUM_NAMES = ("S_h", "S_u", "S_v", "S_uh", "S_vh", "S_uuh", "S_uvh", "S_vvh", "S_d", "S_dd", "S_a", "S_ua", "S_va", "S_qa")
FIELD_NAMES = ("hbar", "ubar", "vbar", "um", "vm", "Ruu", "Ruv", "Rvv", "Fu", "Fv", "dbar", "dvar", "qm", "Qu", "Qv", "ens")
INTEGRAL_NAMES = ("eke", "dvar", "potential_enstrophy")
NSUM, NFIELD, NINT = 14, 16, 3


def elevations(case, q_df):
    """(npoin, L): the elevation of every layer's top interface of the state q_df (row 5 of layer_fields)."""
    with np.errstate(all="ignore"):                 # (nodes of ghost elements may hold anything)
        return np.asfortranarray(_diag.layer_fields(case, q_df)[4])


def rest_elevations(case):
    """zref(npoin, L) of the case's own state: the rest elevations when the case starts at rest."""
    return elevations(case, np.asarray(case.arrays["q_df"]))


def _zref_arg(zref, npoin, L):
    if zref is None:
        return None
    z = np.array(zref, dtype=np.float64, order="F")
    if z.shape != (npoin, L):
        raise ValueError(f"zref: shape {z.shape}, expected (npoin, nlayers) = ({npoin}, {L})")
    return z


def _fields(sums, n, nown):
    S = np.asarray(sums)
    out = np.zeros((NFIELD,) + S.shape[1:], order="F")
    o = slice(0, nown)
    Sh, Su, Sv, Suh, Svh, Suuh, Suvh, Svvh, Sd, Sdd, Sa, Sua, Sva, Sqa = (S[c, o] for c in range(NSUM))
    N = float(n)
    hbar, ubar, vbar, um, vm = Sh / N, Su / N, Sv / N, Suh / Sh, Svh / Sh
    dbar, qm = Sd / N, Sa / Sh
    vals = (hbar, ubar, vbar, um, vm,
            Suuh / Sh - um * um, Suvh / Sh - um * vm, Svvh / Sh - vm * vm,
            Suh / N - ubar * hbar, Svh / N - vbar * hbar,
            dbar, Sdd / N - dbar * dbar,
            qm, Sua / Sh - um * qm, Sva / Sh - vm * qm,
            0.5 * (Sqa / Sh - qm * qm))
    for c, x in enumerate(vals):
        out[c, o] = x
    return out


class HostEddyCov:
    """The numpy mirror.  case: a hnumo.case.Case (or a rank's case of a partition: only its owned
    elements count).  coriolis: as HostVorticity's (True: coriolis_of(case); False or None: 0; or an
    array (npoin)).  zref: (npoin, L), or None: 0."""

    needs_host_state = True      # time_loop syncs a resident stepper before add(q)

    def __init__(self, case, coriolis=True, zref=None):
        self.case = case
        self.hv = HostVorticity(case, coriolis=coriolis, series=False)     # the one gradient
        hv = self.hv
        self.L, self.npoin, self.P, self.ne, self.nown = hv.L, hv.npoin, hv.P, hv.ne, hv.nown
        self.ag, self.w = hv.ag, hv.w
        self.f = hv.f.reshape(-1)
        z = _zref_arg(zref, self.npoin, self.L)
        self.zref = np.zeros((self.npoin, self.L), order="F") if z is None else z
        self._sums = np.zeros((NSUM, self.npoin, self.L), order="F")
        self.nsamples = 0

    def add(self, q_df):
        o = slice(0, self.nown)
        elev = elevations(self.case, q_df)
        for k in range(self.L):
            dp = np.asarray(q_df[0, o, k], dtype=np.float64)
            h = self.ag[k] * dp
            u, v = q_df[1, o, k] / dp, q_df[2, o, k] / dp
            zeta, _, pv, _, _ = self.hv._layer(q_df, k)
            zeta, pv = zeta.reshape(-1), pv.reshape(-1)
            a = zeta + self.f
            d = elev[o, k] - self.zref[o, k]
            terms = (h, u, v, u * h, v * h, (u * u) * h, (u * v) * h, (v * v) * h, d, d * d, a, u * a, v * a, pv * a)
            for c, x in enumerate(terms):
                self._sums[c, o, k] = self._sums[c, o, k] + x
        self.nsamples += 1

    def sums(self):
        """(sums (14, npoin, L), the sample count)."""
        return self._sums.copy(order="F"), self.nsamples

    def set_sums(self, sums, nsamples: int):
        s = np.array(sums, dtype=np.float64, order="F")
        if s.shape != self._sums.shape:
            raise ValueError(f"sums: shape {s.shape}, expected {self._sums.shape}")
        if int(nsamples) < 0:
            raise ValueError("nsamples must be >= 0")
        self._sums, self.nsamples = s, int(nsamples)

    def fields(self):
        if self.nsamples == 0:
            raise ValueError("eddy covariances: no samples yet")
        return _fields(self._sums, self.nsamples, self.nown)

    def element_sums(self):
        """(3, L, ne): per element the products jac_I*x_I of the three integrands added in node order
        from the first product -- what tree_sum combines into the integrals."""
        F = self.fields()
        out = np.zeros((NINT, self.L, self.ne))
        o = slice(0, self.nown)
        for k in range(self.L):
            hbar, Ruu, Rvv, dvar, ens = (F[c, o, k] for c in (0, 5, 7, 11, 15))
            for c, x in enumerate((hbar * (0.5 * (Ruu + Rvv)), dvar, hbar * ens)):
                out[c, k] = np.add.accumulate((self.w * x).reshape(self.ne, self.P), axis=1)[:, -1]
        return out

    def integrals(self):
        """(3, L) = the integrals of hbar*(0.5*(Ruu+Rvv)), dvar, hbar*ens over the owned elements."""
        el = self.element_sums()
        out = np.zeros((NINT, self.L), order="F")
        for k in range(self.L):
            for c in range(NINT):
                out[c, k] = tree_sum(el[c, k])
        return out


class DeviceEddyCov:
    """The same read-outs from an hnumo.engine.Engine.  every = k >= 1: the engine samples itself after
    every k-th successful step (leave add() alone then); every = 0: add() takes a sample.  coriolis and
    zref as HostEddyCov's."""

    needs_host_state = False

    def __init__(self, engine, every: int = 0, coriolis=True, zref=None):
        self.engine = engine
        if coriolis is True:
            f = coriolis_of(engine.case)
        elif coriolis is False or coriolis is None:
            f = None
        else:
            f = coriolis
        engine.cov_begin(f, zref, every)

    def add(self, q_df=None):
        """One sample of the state on the device (q_df is ignored; no sync)."""
        self.engine.cov_accumulate()

    def sums(self):
        return self.engine.cov_sums()

    @property
    def nsamples(self) -> int:
        return self.engine.cov_sums()[1]

    def set_sums(self, sums, nsamples: int):
        self.engine.cov_set_sums(sums, nsamples)

    def fields(self):
        return self.engine.cov_fields()

    def integrals(self):
        return self.engine.cov_integrals()

    def end(self):
        self.engine.cov_end()
