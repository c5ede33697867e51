"""Energy budget (hnumo_energy_*, hnumo/energy.py), the parts that need no GPU: the declarations on both
sides of the boundary, the numpy mirror HostEnergy against analytic identities and on the CPU oracle's
moving states (tests/states.py), and time_loop's energy hook.  Comparisons are np.array_equal unless they
state their bound; RTOL = 1e-10 is the project's second-line tolerance."""
import io
import math
import os
import re

import numpy as np
import pytest

import states
import wind_cases as WC
from hnumo import covariance as CV
from hnumo import diagnostics as D
from hnumo import energy as EN
from hnumo import flowstats as F
from hnumo import wind as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hnumo_energy_begin", "hnumo_energy_sample", "hnumo_energy_series", "hnumo_energy_sums", "hnumo_energy_set_sums",
       "hnumo_energy_means", "hnumo_energy_end")
RTOL = 1e-10
EPS = float(np.finfo(np.float64).eps)
BRICKS = [("dg25L3", {"nelx": 4, "nely": 4}), ("dg25N7L3", {"nelx": 3, "nely": 3}), ("bump10", {"nop": 2, "nelx": 6, "nely": 6})]
WARPED = BRICKS + [("qmbump8", {})]           # uniform fields and a linear shear are exact on warped elements too
MOVING = [("bump10", {"nop": 2}, 3), ("dg25L3", {"nelx": 5, "nely": 3}, 4)]
_states = {}


def test_header_fortran_module_and_python_declare_the_energy_budget():
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    f90 = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    py = open(os.path.join(REPO, "h-numo_amd", "hnumo", "engine.py")).read()
    abi = open(os.path.join(REPO, "h-numo_amd", "hnumo", "abi.py")).read()
    public = re.search(r"public :: hnumo_engine_create.*?\n\s*\n", f90, re.S).group(0)
    for fn in NEW:
        assert re.search(r"\bint\s+%s\s*\(hnumo_engine \*eng" % fn, hdr), fn
        assert f"name='{fn}'" in f90, fn
        assert re.search(r"\b%s\b" % fn, public), fn
        assert f"L.{fn}.argtypes" in abi, fn
        assert re.search(r"def %s\(self" % fn[len("hnumo_"):], py), fn
    assert re.search(r"#define HNUMO_ABI_VERSION 10\b", hdr)      # additive: the version stays
    assert re.search(r"HNUMO_ABI_EXPECTED = 10\b", f90)
    assert EN.series_names(2) == ("KE_1", "KE_2", "APE_1", "APE_2", "V_1", "V_2", "W", "D")


# ------------------------------------------------------------------ analytic identities
def rel(got, want):
    return abs(got - want) / abs(want)


def geometry(case):
    """(x, y at the nodes, the domain's area -- the sum of the quad weights, which is the sum of the nodal ones --
    its x and y extents)"""
    xy = np.asarray(case.arrays["coord"])
    (x0, x1), (y0, y1) = case.cfg["xdims"], case.cfg["ydims"]
    area = float(np.asarray(case.arrays["jacq"]).sum())
    assert rel(area, (x1 - x0) * (y1 - y0)) < 1e-12 and rel(float(np.asarray(case.arrays["jac"]).sum()), area) < 1e-12
    return xy[0], xy[1], area, (x0, x1), (y0, y1)


def uniform_state(case, U, V, dps):
    """q_df with layer k at thickness dps[k] everywhere, moving at (U, V)*(1 + 0.1 k)"""
    S = case.scalars
    q = np.zeros((3, S["npoin"], S["nlayers"]), order="F")
    for k in range(S["nlayers"]):
        f = 1.0 + 0.1 * k
        q[0, :, k] = dps[k]
        q[1, :, k] = (U * f) * dps[k]
        q[2, :, k] = (V * f) * dps[k]
    return q


def dps_of(case):
    return [3.0e6 * (1.0 + 0.5 * k) for k in range(case.scalars["nlayers"])]


@pytest.mark.parametrize("name,kw", WARPED)
def test_uniform_flow_under_a_uniform_wind(case_factory, name, kw):
    case = case_factory(name, **kw)
    _, _, area, _, _ = geometry(case)
    L = case.scalars["nlayers"]
    U, V, t1, t2 = 0.3, -0.2, 0.07, 0.11
    tau = np.zeros((2, case.scalars["npoin_q"]), order="F")
    tau[0], tau[1] = t1, t2
    he = EN.HostEnergy(case)
    he.add(uniform_state(case, U, V, dps_of(case)), tau)
    assert rel(he.series()[3 * L, 0], (t1 * U + t2 * V) * area) < RTOL            # the top layer's velocity
    quad, _, n = he.sums()
    assert n == 1 and np.abs(quad[0] / (t1 * U + t2 * V) - 1.0).max() < RTOL


@pytest.mark.parametrize("botfr", [1, 2])
@pytest.mark.parametrize("name,kw", WARPED)
def test_uniform_flow_drag(case_factory, name, kw, botfr):
    case = case_factory(name, botfr=botfr, cd=1e-3, **kw)
    _, _, area, _, _ = geometry(case)
    S, L = case.scalars, case.scalars["nlayers"]
    U, V = 0.3, -0.2
    dps = dps_of(case)
    f = 1.0 + 0.1 * (L - 1)
    sp2 = (U * f) ** 2 + (V * f) ** 2
    he = EN.HostEnergy(case)
    he.add(uniform_state(case, U, V, dps))
    alphaL = float(np.asarray(case.arrays["alpha"]).reshape(-1)[L - 1])
    want = (S["cd"] / S["gravity"]) * dps[L - 1] * sp2 * area if botfr == 1 else (S["cd"] / alphaL) * sp2 ** 1.5 * area
    assert want > 0 and rel(he.series()[3 * L + 1, 0], want) < RTOL


@pytest.mark.parametrize("name,kw", WARPED)
def test_linear_shear_dissipation(case_factory, name, kw):
    """u = s*(y - ybar), v = 0, uniform dp: V_k = visc*s^2*(dp/g)*area; u_x contributes below the bound."""
    case = case_factory(name, visc=50.0, **kw)
    x, y, area, _, (y0, y1) = geometry(case)
    S, L = case.scalars, case.scalars["nlayers"]
    s = 1.0e-6
    dps = dps_of(case)
    q = uniform_state(case, 0.0, 0.0, dps)
    for k in range(L):
        q[1, :, k] = (s * (y - 0.5 * (y0 + y1))) * dps[k]
    he = EN.HostEnergy(case)
    he.add(q)
    for k in range(L):
        assert rel(he.series()[2 * L + k, 0], S["visc"] * s * s * (dps[k] / S["gravity"]) * area) < RTOL, k


@pytest.mark.parametrize("name,kw", BRICKS[:2])
def test_linear_interface_displacement_against_a_flat_zref(case_factory, name, kw):
    """Interface k alone tilted by a*(x - xbar): APE_k = c_k*a^2*integral of (x - xbar)^2, the other rows 0."""
    case = case_factory(name, **kw)
    x, y, area, (x0, x1), (y0, y1) = geometry(case)
    S, L, g = case.scalars, case.scalars["nlayers"], case.scalars["gravity"]
    assert np.ptp(case.arrays["zbot_df"]) == 0
    alpha = np.asarray(case.arrays["alpha"]).reshape(-1)
    ag = [alpha[k] / g for k in range(L)]
    H = [400.0 * (k + 1) for k in range(L)]                     # layer thicknesses in metres
    zref = np.zeros((S["npoin"], L), order="F")
    for k in range(L):
        zref[:, k] = float(case.arrays["zbot_df"][0]) + sum(H[k:])
    a = 1.0e-5                                                  # 10 m across a 1000 km basin
    tilt = a * (x - 0.5 * (x0 + x1))
    integral = (x1 - x0) ** 3 / 12.0 * (y1 - y0)
    for k in range(L):
        h = [np.full(S["npoin"], H[l]) for l in range(L)]
        h[k] = h[k] + tilt
        if k > 0:
            h[k - 1] = h[k - 1] - tilt
        q = np.zeros((3, S["npoin"], L), order="F")
        for l in range(L):
            q[0, :, l] = h[l] / ag[l]
        he = EN.HostEnergy(case, zref=zref)
        he.add(q)
        ape = he.series()[L:2 * L, 0]
        assert rel(ape[k], he.c[k] * a * a * integral) < RTOL, (k, ape)
        assert all(ape[l] < 1e-12 * ape[k] for l in range(L) if l != k), (k, ape)


# ------------------------------------------------------------------ exact statements, moving states
def oracle_states(case_factory, name, kw, nsteps):
    """(the moving case, the CPU oracle's states after steps 1..nsteps of it), computed once."""
    key = (name, tuple(sorted(kw.items())), nsteps)
    if key not in _states:
        import oracle as O
        case = states.moving_case(case_factory(name, **kw))
        o = O.Oracle(case)
        q, qb, qp = o.state()
        out = []
        for _ in range(nsteps):
            o.ti_rk_bcl(q, qb, qp)
            out.append(q.copy(order="F"))
        assert all(np.isfinite(x).all() for x in out)
        _states[key] = (case, out)
    return _states[key]


def mirror(case, qs, **kw):
    he = EN.HostEnergy(case, **kw)
    for q in qs:
        he.add(q)
    return he


def plus_zero(a):
    a = np.asarray(a)
    return not a.any() and not np.signbit(a).any()


def test_zero_wind_no_drag_no_viscosity_give_plus_zero(case_factory):
    case, qs = oracle_states(case_factory, *MOVING[0])
    S, L = case.scalars, case.scalars["nlayers"]
    assert not np.asarray(case.arrays["tau_wind"]).any() and S["botfr"] == 0 and S["visc"] == 0
    he = mirror(case, qs)
    ser = he.series()
    quad, nodal, n = he.sums()
    assert n == len(qs) and ser.shape == (3 * L + 2, len(qs))
    assert plus_zero(ser[3 * L]) and plus_zero(quad[0])                     # W, S_W
    assert plus_zero(ser[3 * L + 1]) and plus_zero(quad[1])                 # D, S_D
    assert plus_zero(ser[2 * L:3 * L]) and plus_zero(nodal)                 # V, S_V
    assert (ser[:2 * L] > 0).all()


def test_terms_are_non_negative_and_non_trivial(case_factory):
    case, qs = oracle_states(case_factory, *MOVING[1])
    S, L = case.scalars, case.scalars["nlayers"]
    assert np.asarray(case.arrays["tau_wind"]).any() and S["botfr"] == 1 and S["visc"] > 0
    he = mirror(case, qs, zref=CV.rest_elevations(case_factory(MOVING[1][0], **MOVING[1][1])))
    ser = he.series()
    quad, nodal, _ = he.sums()
    assert np.isfinite(ser).all() and (ser[:3 * L] > 0).all() and (ser[3 * L + 1] > 0).all()
    assert (quad[1] >= 0).all() and (nodal >= 0).all() and quad[0].any() and quad[1].any() and nodal.any()
    ke, ape, eps, Wq, Dq = he.terms(qs[0])
    assert (ke >= 0).all() and (ape >= 0).all() and (eps >= 0).all() and (Dq >= 0).all() and (Wq > 0).any() and (Wq < 0).any()
    mq, mn = he.means()
    assert np.array_equal(mq, quad / float(len(qs))) and np.array_equal(mn, nodal / float(len(qs)))


@pytest.mark.parametrize("name,kw,nsteps", MOVING)
def test_first_ape_row_is_zero_against_the_first_states_elevations(case_factory, name, kw, nsteps):
    case, qs = oracle_states(case_factory, name, kw, nsteps)
    L = case.scalars["nlayers"]
    ser = mirror(case, qs, zref=CV.elevations(case, qs[0])).series()
    assert plus_zero(ser[L:2 * L, 0]) and (ser[L:2 * L, 1:] > 0).all()


@pytest.mark.parametrize("name,kw,nsteps", MOVING)
def test_ke_equals_the_flow_statistics_ke_over_alpha(case_factory, name, kw, nsteps):
    """Both are sums of positive terms through the same tree; a term differs by at most four roundings."""
    case, qs = oracle_states(case_factory, name, kw, nsteps)
    S, L = case.scalars, case.scalars["nlayers"]
    he, fs = mirror(case, qs), F.HostFlowStats(case)
    for q in qs:
        fs.add(q)
    bound = (2 * (S["ngl"] ** 2 + math.ceil(math.log2(S["nelem"]))) + 8) * EPS
    for k in range(L):
        want = fs.series[0, k] / he.alpha[k]
        assert (np.abs(he.series()[k] - want) <= bound * want).all(), (k, np.abs(he.series()[k] / want - 1).max(), bound)


def chunked_tree(x, chunk=1024):
    return F.tree_sum([F.tree_sum(x[c:c + chunk]) for c in range(0, len(x), chunk)])


def test_chunked_tree_equals_the_unchunked_one(case_factory):
    """37*37 = 1369 elements at N=2: two aligned chunks of 1024, the second ragged."""
    case = states.moving_case(case_factory("dg25L3", nelx=37, nely=37, nop=2))
    assert case.scalars["nelem"] == 1369
    he = EN.HostEnergy(case)
    he.add(case.arrays["q_df"])
    row = he.series()[:, 0]
    assert he.partials.shape == (row.size, 1369)
    for r in range(row.size):
        assert chunked_tree(he.partials[r]) == row[r], r
    assert row[:-2].all() and row[-1] > 0


def test_sums_round_trip_and_a_run_continues_on_the_same_bits(case_factory):
    case, qs = oracle_states(case_factory, *MOVING[1])
    whole = mirror(case, qs)
    first = mirror(case, qs[:2])
    quad, nodal, n = first.sums()
    second = EN.HostEnergy(case)
    second.set_sums(quad, nodal, n)
    for a, b in zip(second.sums(), first.sums()):
        assert np.array_equal(a, b)
    for q in qs[2:]:
        second.add(q)
    for a, b in zip(second.sums(), whole.sums()):
        assert np.array_equal(a, b)
    assert np.array_equal(second.series(), whole.series()[:, 2:])
    with pytest.raises(ValueError):
        second.set_sums(quad[:, :-1], nodal, 1)
    with pytest.raises(ValueError):
        second.set_sums(quad, nodal, -1)
    with pytest.raises(ValueError):
        EN.HostEnergy(case).means()
    with pytest.raises(ValueError):
        EN.HostEnergy(case, series=False).series()


def test_quad_coords_interpolate_the_node_coordinates(case_factory):
    case = case_factory("qmbump8")
    xq = EN.quad_coords(case)
    S = case.scalars
    assert xq.shape == (2, S["npoin_q"]) and np.isfinite(xq).all()
    xy = np.asarray(case.arrays["coord"])
    for c in range(2):                                          # inside each element's own node box
        lo, hi = (f(xy[c].reshape(S["nelem"], -1), axis=1) for f in (np.min, np.max))
        q = xq[c].reshape(S["nelem"], -1)
        tol = 1e-12 * np.abs(xy[c]).max()
        assert (q >= lo[:, None] - tol).all() and (q <= hi[:, None] + tol).all()
    # an affine element: the quad points' mean weighted by wjac is the centroid the nodes give
    brick = case_factory("bump10", nop=2, nelx=6, nely=6)
    xb, Sb = EN.quad_coords(brick), brick.scalars
    wq = np.asarray(brick.arrays["jacq"]).reshape(-1, order="F").reshape(Sb["nelem"], -1)
    wn = np.asarray(brick.arrays["jac"]).reshape(-1, order="F").reshape(Sb["nelem"], -1)
    cq = (wq * xb[0].reshape(Sb["nelem"], -1)).sum(axis=1) / wq.sum(axis=1)
    cn = (wn * np.asarray(brick.arrays["coord"])[0].reshape(Sb["nelem"], -1)).sum(axis=1) / wn.sum(axis=1)
    assert np.abs(cq - cn).max() < 1e-9 * np.abs(cn).max()


# ------------------------------------------------------------------ time_loop
@pytest.mark.parametrize("ramp", [False, True])
def test_time_loop_feeds_the_host_object_the_steps_wind(case_factory, tmp_path, ramp):
    """4 steps on the CPU oracle, energy_every = 2: samples of steps 2 and 4, each under the wind its step used
    (with a HostWind ramp: rows 1 and 3 of the table; without: the case's own)."""
    case = WC.case_of("N2", case_factory)
    S = case.scalars
    pat = WC.patterns(case, 1)
    table = W.ramp(4)
    taus = [W.blend(pat, table[:, r]) if ramp else np.asarray(case.arrays["tau_wind"]) for r in range(4)]
    sts, _ = WC.Oracles(case).run(taus)
    want = EN.HostEnergy(case)
    for i in (1, 3):
        want.add(sts[i][0], taus[i])
    he = EN.HostEnergy(case)
    stepper = WC.OracleStepper(case)
    q, qb, qp = D.time_loop(case, stepper, 4 * S["dt"] * (1 - 1e-9), out_dir=str(tmp_path), lcheck_conserved=False,
                            lprint_diagnostics=False, out=io.StringIO(), wind=W.HostWind(pat, table) if ramp else None,
                            energy=he, energy_every=2)
    assert WC.same_state((q, qb, qp), sts[3])
    assert he.nsamples == 2 and np.array_equal(he.series(), want.series())
    for a, b in zip(he.sums(), want.sums()):
        assert np.array_equal(a, b)
    L = S["nlayers"]
    assert he.series()[3 * L].all()
    if ramp:                                                    # the wind grew: so did its power
        own = EN.HostEnergy(case)
        own.add(sts[1][0])
        assert not np.array_equal(own.series()[3 * L, 0], he.series()[3 * L, 0])
    with pytest.raises(ValueError):
        D.time_loop(case, stepper, S["dt"], out_dir=str(tmp_path), energy=he, energy_every=0)
