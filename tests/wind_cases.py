"""What the wind tests share (a plain helper module): the cases, the patterns, the oracle runs.

The cases are the parity matrix's dg3 family (wind, f, beta, L = 3) through matrix.cell_config with a moving
state: N = 2 and 4 on 4x4 elements, N = 7 on 3x3, N = 4 on a warped mesh -- npoin_q = 400, 1296, 2025, all
ragged against 256 lanes, and odd Q = 25, 81, 225, so that every element's qstatE record carries its pad word.
Pattern 0 is the case's own wind; the others are seeded uniform random values in +-0.05 at every quad point and
component, so that any slip of an index shows.

The expected state of a run comes from one Oracle per distinct tau, each created from the case with
arrays["tau_wind"] replaced by wind.blend(...) and fed the running state.
"""
import copy

import numpy as np

import matrix as M

CELLS = {
    "N2": dict(N=2, family="dg3", visc=0, walls="free", botfr=0, shear=0, mesh="brick", state="moving"),
    "N4": dict(N=4, family="dg3", visc=0, walls="free", botfr=0, shear=0, mesh="brick", state="moving"),
    "N7": dict(N=7, family="dg3", visc=0, walls="free", botfr=0, shear=0, mesh="brick", state="moving"),
    "N4warp": dict(N=4, family="dg3", visc=0, walls="noslip", botfr=2, shear=0, mesh="warp", state="moving"),
}
NPQ = {"N2": 400, "N4": 1296, "N7": 2025, "N4warp": 1296}
# the zero-wind case: a lake cell of the matrix, N = 3, two layers
LAKE = "N3-lake2-v3-free-b0-s1-brick-moving"


def case_of(name, case_factory):
    """The Case of a wind cell (or of the matrix cell LAKE)."""
    cell = M.BY_NAME[name] if name in M.BY_NAME else CELLS[name]
    return M.cell_case(cell, case_factory)


def patterns(case, nm, seed=7):
    """(2, npoin_q, nm): the case's own wind, then nm - 1 random patterns in +-0.05."""
    rng = np.random.default_rng(seed)
    t0 = np.asarray(case.arrays["tau_wind"], dtype=np.float64)
    p = np.zeros(t0.shape + (nm,), order="F")
    p[:, :, 0] = t0
    for m in range(1, nm):
        p[:, :, m] = rng.uniform(-0.05, 0.05, size=t0.shape)
    return p


def with_wind(case, tau):
    """A copy of ``case`` created with the wind ``tau`` (the other tables are shared, not copied)."""
    c = copy.copy(case)
    c.arrays = dict(case.arrays)
    c.arrays["tau_wind"] = np.array(tau, dtype=np.float64, order="F")
    return c


class Oracles:
    """One Oracle per distinct tau of a case, made on first use."""

    def __init__(self, case):
        self.case = case
        self._o = {}

    def of(self, tau):
        import oracle as O
        key = np.ascontiguousarray(tau).tobytes()
        if key not in self._o:
            self._o[key] = O.Oracle(with_wind(self.case, tau))
        return self._o[key]

    def run(self, taus, state=None):
        """Step i under taus[i] from ``state`` (default the case's own): the states after every step (copies) and
        the last step's oracle."""
        st = state if state is not None else tuple(np.array(self.case.arrays[k], order="F")
                                                    for k in ("q_df", "qb_df", "qprime_df"))
        st = tuple(np.array(a, order="F") for a in st)
        out, o = [], None
        for tau in taus:
            o = self.of(tau)
            o.ti_rk_bcl(*st)
            out.append(tuple(a.copy(order="F") for a in st))
        return out, o


class OracleStepper:
    """An oracle-backed stepper with set_tau_wind, for time_loop(wind=HostWind): a new wind means the oracle
    of the case created with it."""

    def __init__(self, case):
        self.oracles = Oracles(case)
        self.tau = np.asarray(case.arrays["tau_wind"])
        self.winds = []

    def set_tau_wind(self, tau):
        self.tau = np.array(tau, order="F")
        self.winds.append(self.tau)

    def ti_rk_bcl(self, q, qb, qp):
        self.oracles.of(self.tau).ti_rk_bcl(q, qb, qp)


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))
