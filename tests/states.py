"""States that move, for tests (a plain helper module).

Every initial condition of hnumo/case.py starts at rest with flat interfaces, so a test that feeds
a case's own state never drives transport across a face: the upwinded layer fluxes, the layer
overlap at a face, the drag and the viscosity all see u = v = 0 and a continuous thickness.
``moving_state`` builds a state of the same case that is neither at rest nor continuous, and
``with_state`` hands it to everything that reads a Case (the oracle, the engine, the bundle of
the reference harness, the partitioners).

The amplitudes are small on purpose: a DG step has no limiter, and a 10 % jump or velocities of
0.05 c drive a layer thickness negative within two steps.  tests/test_states_cpu.py checks, from
the state alone, that the values below are still large enough to move every layer across every
interior face in both directions.
"""
import copy
import math

import numpy as np

# the amplitudes every moving cell of tests/matrix.py uses (conditions (a)-(d) of
# tests/test_states_cpu.py hold for them on every cell):
#   AMP   relative amplitude of the smooth thickness modulation
#   FR    velocity amplitude as a fraction of the gravity-wave speed sqrt(alpha_L pb')
#   JUMP  relative amplitude of the element-checkerboard jump of the thickness (and, scaled, of
#         the velocities)
AMP, FR, JUMP = 0.01, 0.002, 0.02
DEFAULT = dict(amp=AMP, fr=FR, jump=JUMP)


def moving_state(case, *, amp=AMP, fr=FR, jump=JUMP):
    """(q_df, qb_df, qprime_df) of ``case`` in Fortran order, in motion:

    * thickness of layer k = the case's own thickness times
      1 + amp sin(2 pi X + phi_k) cos(2 pi Y - phi_k) + (-1)^k (1 - k/4) jump c(e),
      X, Y the node coordinates scaled to the unit square, phi_k = 0.7 k the per-layer phase and
      c(e) = +-1 the element checkerboard (the weight 1 - k/4 keeps the jumps of equal layers from
      cancelling in the interface heights, so that the layers of the two sides of a face overlap);
    * velocities of layer k = (-1)^k fr sqrt(alpha_L pb') times a smooth part of one wavelength
      across the domain plus half a checkerboard, in both components;
    * qb_df and qprime_df derived from them by the statements of the initial conditions
      (hnumo.case.derived_state)."""
    from hnumo.case import derived_state
    A, S, cfg = case.arrays, case.scalars, case.cfg
    L, P, nelem = S["nlayers"], S["ngl"] ** 2, S["nelem"]
    x, y = np.asarray(A["coord"][0]), np.asarray(A["coord"][1])
    X = (x - cfg["xdims"][0]) / (cfg["xdims"][1] - cfg["xdims"][0])
    Y = (y - cfg["ydims"][0]) / (cfg["ydims"][1] - cfg["ydims"][0])
    e = np.arange(nelem)
    cb = np.repeat(np.where((e % cfg["nelx"] + e // cfg["nelx"]) % 2 == 0, 1.0, -1.0), P)
    pb = np.asarray(A["pbprime_df"])
    c = np.sqrt(np.asarray(A["alpha"])[L - 1] * pb)
    q0 = np.asarray(A["q_df"])
    q = np.zeros_like(q0, order="F")
    tp = 2.0 * math.pi
    for k in range(L):
        s = 1.0 if k % 2 == 0 else -1.0
        ph = 0.7 * k
        h = q0[0, :, k] * (1.0 + amp * np.sin(tp * X + ph) * np.cos(tp * Y - ph) + s * (1.0 - 0.25 * k) * jump * cb)
        u = s * fr * c * (np.sin(tp * X + ph) * np.cos(tp * Y) + 0.5 * cb)
        v = s * fr * c * (np.cos(tp * X) * np.sin(tp * Y + ph) - 0.5 * cb)
        q[0, :, k] = h
        q[1, :, k] = u * h
        q[2, :, k] = v * h
    qb, qp = derived_state(q, pb)
    return q, np.asfortranarray(qb), np.asfortranarray(qp)


def with_state(case, q, qb, qp):
    """A copy of ``case`` whose arrays carry the state (the static tables are shared, not copied)."""
    c = copy.copy(case)
    c.arrays = dict(case.arrays)
    c.arrays.update(q_df=np.array(q, dtype=np.float64, order="F"), qb_df=np.array(qb, dtype=np.float64, order="F"),
                    qprime_df=np.array(qp, dtype=np.float64, order="F"))
    return c


def moving_case(case, **params):
    """``case`` carrying its moving state (``params``: amp, fr, jump; default the module's)."""
    return with_state(case, *moving_state(case, **{**DEFAULT, **params}))
