"""Online flow statistics: the time means, MKE / EKE and kinetic-energy series that the
double-gyre post-processing (Examples/double_gyre/compute_eke.m, compute_ke.m) forms from hundreds
of `mlswe####` snapshots, accumulated sample by sample instead.

    tree_sum         the position-based pairwise sum of the series' definition
    HostFlowStats    the numpy statement of the definitions, fed with q_df arrays on the host
    DeviceFlowStats  the same read-outs from the engine, which accumulates where the state lives
                     (kernels_stats.hip through hnumo_stats_*): no sync, nothing copied per sample

Definitions (normative; include/hnumo_engine.h).  Per owned node and layer, from
q_df(3,npoin,L) as diagnostics.layer_fields forms them:

    dp = q(1); h = (alpha_k/gravity)*dp; u = q(2)/dp; v = q(3)/dp
    uh = u*h;  vh = v*h;  e = (0.5*(u*u + v*v))*h

A sample adds h, uh, vh, e to the sums S_h, S_uh, S_vh, S_e (4,npoin,L), in sample order from
+0.0.  Fields (5,npoin,L) after n samples: hbar = S_h/n, um = S_uh/S_h, vm = S_vh/S_h,
mke = S_e/S_h, eke = mke - 0.5*(um*um + vm*vm).  Series (2,L,count): KE_k, VOL_k = the integrals
of e and h over the owned elements -- per element the products jac_I*e_I added in node order, the
element sums combined by tree_sum.  Nodes of ghost elements are never accumulated and read 0.
The two classes agree bit for bit (tests/test_flowstats_gpu.py).
"""
from __future__ import annotations

import numpy as np

FIELD_NAMES = ("hbar", "um", "vm", "mke", "eke")


def tree_sum(x) -> float:
    """Pairwise sum by position: entry i of the next level is x[2i] + x[2i+1], or x[2i] alone when
    2i+1 does not exist, until one value is left.  Any split into aligned power-of-two blocks
    gives the same bits."""
    x = np.array(x, dtype=np.float64).reshape(-1)
    if x.size == 0:
        return 0.0
    while x.size > 1:
        m = x.size // 2
        y = x[0:2 * m:2] + x[1:2 * m:2]
        x = np.concatenate([y, x[2 * m:]])
    return float(x[0])


def _fields(sums, n, nown):
    S = np.asarray(sums)
    out = np.zeros((5,) + S.shape[1:], order="F")
    o = slice(0, nown)
    Sh = S[0, o]
    um, vm, mke = S[1, o] / Sh, S[2, o] / Sh, S[3, o] / Sh
    out[0, o] = Sh / float(n)
    out[1, o] = um
    out[2, o] = vm
    out[3, o] = mke
    out[4, o] = mke - 0.5 * (um * um + vm * vm)
    return out


class HostFlowStats:
    """The numpy mirror.  case: a hnumo.case.Case (or a rank's case of a partition: only its owned
    elements count).  series=False skips the KE/VOL series."""

    needs_host_state = True      # time_loop syncs a resident stepper before add(q)

    def __init__(self, case, series: bool = True):
        A, S = case.arrays, case.scalars
        self.L, self.npoin, self.P = S["nlayers"], S["npoin"], S["ngl"] ** 2
        self.ne = int(getattr(case, "nelem_owned", 0) or S["nelem"])
        self.nown = self.ne * self.P
        self.ag = [A["alpha"][k] / S["gravity"] for k in range(self.L)]
        self.w = np.asarray(A["jac"], dtype=np.float64).reshape(-1, order="F")[:self.nown]
        self.sums = np.zeros((4, self.npoin, self.L), order="F")
        self.nsamples = 0
        self._series = [] if series else None

    def add(self, q_df):
        o = slice(0, self.nown)
        entry = np.zeros((2, self.L), order="F")
        for k in range(self.L):
            dp = np.asarray(q_df[0, o, k], dtype=np.float64)
            h = self.ag[k] * dp
            u, v = q_df[1, o, k] / dp, q_df[2, o, k] / dp
            uh, vh = u * h, v * h
            e = (0.5 * (u * u + v * v)) * h
            for c, x in enumerate((h, uh, vh, e)):
                self.sums[c, o, k] = self.sums[c, o, k] + x
            if self._series is not None:
                for c, x in enumerate((e, h)):
                    # per element in node order, from the first product
                    el = np.add.accumulate((self.w * x).reshape(self.ne, self.P), axis=1)[:, -1]
                    entry[c, k] = tree_sum(el)
        self.nsamples += 1
        if self._series is not None:
            self._series.append(entry)

    def fields(self):
        if self.nsamples == 0:
            raise ValueError("flow statistics: no samples yet")
        return _fields(self.sums, self.nsamples, self.nown)

    @property
    def series(self):
        """(2, L, count): KE_k and VOL_k per sample."""
        s = self._series or []
        out = np.zeros((2, self.L, len(s)), order="F")
        for i, e in enumerate(s):
            out[:, :, i] = e
        return out

    def ke_normalised(self):
        """(L, count): KE_k/VOL_k, compute_ke.m's per-layer series up to its unit factor."""
        s = self.series
        return s[0] / s[1]


class DeviceFlowStats:
    """The same read-outs from an hnumo.engine.Engine.  every = k >= 1: the engine samples itself
    after every k-th successful step (leave add() alone then); every = 0: add() takes a sample.
    series: the number of samples the KE/VOL series can hold (0: none)."""

    needs_host_state = False

    def __init__(self, engine, every: int = 0, series: int = 0):
        self.engine = engine
        engine.stats_begin(every, series)

    def add(self, q_df=None):
        """One sample of the state on the device (q_df is ignored; no sync)."""
        self.engine.stats_accumulate()

    @property
    def sums(self):
        return self.engine.stats_sums()[0]

    @property
    def nsamples(self) -> int:
        return self.engine.stats_sums()[1]

    def set_sums(self, sums, nsamples: int):
        self.engine.stats_set_sums(sums, nsamples)

    def fields(self):
        return self.engine.stats_fields()

    @property
    def series(self):
        return self.engine.stats_series()

    def ke_normalised(self):
        s = self.series
        return s[0] / s[1]

    def end(self):
        self.engine.stats_end()
