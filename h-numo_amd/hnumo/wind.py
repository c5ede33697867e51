"""Time-dependent wind stress: the host mirror of csrc/kernels_wind.hip and the objects hnumo.diagnostics.time_loop
takes as ``wind=``.

The wind is a linear combination of M <= MAXM patterns T_m(2, npoin_q), given as one array (2, npoin_q, M).
Arithmetic (normative, include/hnumo_engine.h; IEEE double, no FMA), per component and quad point:

    tau = c_0*T_0;  for m = 1..M-1: tau = tau + c_m*T_m        (left to right, product first)
    s = 0.0;  N_btp times: s = s + tau;  tau_wind_ave = s / float(N_btp)

``blend`` and ``ave`` are these statements in numpy; an engine whose wind was set to ``blend(patterns, c)`` is,
bit for bit, an engine created with it.  A schedule is a table coef(M, nrows): step k of a run uses row
``row_for(k, nrows, first, mode)``.  ``ramp`` and ``seasonal`` build the two tables every double-gyre run reaches
for: a spin-up and a yearly cycle.
"""
from __future__ import annotations

import math

import numpy as np

MAXM = 4                       # HNUMO_WIND_MAXM
HOLD, REPEAT = 0, 1            # HNUMO_WIND_HOLD / HNUMO_WIND_REPEAT
MODES = {"hold": HOLD, "repeat": REPEAT}


def _patterns(patterns):
    p = np.asarray(patterns, dtype=np.float64)
    if p.ndim == 2:
        p = p[:, :, None]
    if p.ndim != 3 or p.shape[0] != 2 or not 1 <= p.shape[2] <= MAXM:
        raise ValueError(f"patterns: shape {p.shape}, expected (2, npoin_q, M) with 1 <= M <= {MAXM}")
    return p


def blend(patterns, coef):
    """tau_wind(2, npoin_q) = c_0*T_0 + c_1*T_1 + ..., added left to right from the first product."""
    p = _patterns(patterns)
    c = np.asarray(coef, dtype=np.float64).reshape(-1)
    if c.size != p.shape[2]:
        raise ValueError(f"coef: {c.size} coefficients for M = {p.shape[2]} patterns")
    tau = c[0] * p[:, :, 0]
    for m in range(1, c.size):
        tau = tau + c[m] * p[:, :, m]
    return np.asfortranarray(tau)


def ave(tau, N_btp: int):
    """tau_wind_ave of mod_rk_mlswe.F90:117,129: tau added N_btp times to 0.0, divided by N_btp."""
    tau = np.asarray(tau, dtype=np.float64)
    s = np.zeros_like(tau)
    for _ in range(int(N_btp)):
        s = s + tau
    return s / float(int(N_btp))


def _mode(mode) -> int:
    m = MODES.get(mode, mode) if isinstance(mode, str) else mode
    if m not in (HOLD, REPEAT):
        raise ValueError(f"mode: {mode!r}, expected 'hold' or 'repeat'")
    return int(m)


def row_for(k: int, nrows: int, first: int = 0, mode=HOLD) -> int:
    """The table row of step k (0-based): first + k, held at the last row or taken modulo nrows; -1 without rows."""
    if k < 0 or first < 0 or nrows < 0:
        raise ValueError("k, first and nrows must be >= 0")
    if nrows == 0:
        return -1
    r = first + k
    return r % nrows if _mode(mode) == REPEAT else min(r, nrows - 1)


def ramp(nsteps: int):
    """coef(1, nsteps) for HOLD: the wind grows linearly from 1/nsteps of the pattern to all of it at the last row."""
    if nsteps < 1:
        raise ValueError("nsteps must be >= 1")
    return np.asfortranarray((np.arange(1, nsteps + 1, dtype=np.float64) / float(nsteps)).reshape(1, nsteps))


def seasonal(period_steps: int):
    """coef(2, period_steps) for REPEAT: row r is (1, sin(2 pi r / period_steps)) -- a steady pattern plus a
    second one that swings through a cycle of period_steps steps."""
    if period_steps < 1:
        raise ValueError("period_steps must be >= 1")
    t = np.zeros((2, period_steps), order="F")
    t[0] = 1.0
    t[1] = [math.sin(2.0 * math.pi * r / period_steps) for r in range(period_steps)]
    return t


def _table(coef, M: int):
    t = np.asfortranarray(coef, dtype=np.float64)
    if t.ndim == 1:
        t = np.asfortranarray(t.reshape(1, -1))
    if t.ndim != 2 or t.shape[0] != M:
        raise ValueError(f"coef: shape {t.shape}, expected (M = {M}, nrows)")
    return t


class DeviceWind:
    """A scheduled wind on an hnumo.engine.Engine: the patterns and the table go to the device once, and the
    engine blends the row of each step before its launches; nothing is copied per step.  In time_loop the
    schedule is installed at the loop's first step with ``first`` = that step's number, so that a restarted
    run resumes the table; later calls of before_step do nothing."""

    def __init__(self, engine, patterns, coef, mode="hold"):
        self.engine = engine
        self.patterns = _patterns(patterns)
        self.coef = _table(coef, self.patterns.shape[2])
        self.mode = _mode(mode)
        self._installed = False
        engine.wind_begin(self.patterns)

    def before_step(self, stepper, nstep: int):
        if not self._installed:
            self.engine.wind_schedule(self.coef, first=int(nstep), mode=self.mode)
            self._installed = True

    @property
    def next_row(self) -> int:
        return self.engine.wind_get()[1]

    @property
    def tau_wind(self):
        return self.engine.wind_get()[0]

    tau = tau_wind                 # (the wind the last step used, under the name HostWind keeps it)

    def end(self):
        self.engine.wind_end()
        self._installed = False


class HostWind:
    """The same schedule for a stepper that has ``set_tau_wind`` (in tests, one backed by the CPU oracle): before
    step nstep it hands blend(patterns, coef[:, row_for(nstep, ...)]) to the stepper -- only when the row changes."""

    def __init__(self, patterns, coef, mode="hold"):
        self.patterns = _patterns(patterns)
        self.coef = _table(coef, self.patterns.shape[2])
        self.mode = _mode(mode)
        self._row = -1
        self.tau = None            # the wind handed over last (None: none yet)

    def before_step(self, stepper, nstep: int):
        r = row_for(int(nstep), self.coef.shape[1], 0, self.mode)
        if r >= 0 and r != self._row:
            self.tau = blend(self.patterns, self.coef[:, r])
            stepper.set_tau_wind(self.tau)
            self._row = r
