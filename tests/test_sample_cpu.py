"""Sample sets (hnumo_sample_*, hnumo/sample.py), the parts that need no GPU: the declarations on
both sides of the boundary, the Lagrange weights, the numpy mirror HostSampler on the CPU oracle's
states, and the numoNNNN writer.  Every comparison is np.array_equal unless it says otherwise."""
import os
import re

import numpy as np
import pytest

from hnumo import diagnostics as D
from hnumo import sample as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hnumo_sample_create", "hnumo_sample_create_ref", "hnumo_sample_plan", "hnumo_sample",
       "hnumo_sample_series_begin", "hnumo_sample_record", "hnumo_sample_series", "hnumo_sample_destroy")
EPS = 2.0 ** -52
_states = {}


def test_header_fortran_module_and_python_declare_the_sample_sets():
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    f90 = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    py = open(os.path.join(REPO, "h-numo_amd", "hnumo", "engine.py")).read()
    public = re.search(r"public :: hnumo_engine_create.*?\n\s*\n", f90, re.S).group(0)
    for fn in NEW:
        assert re.search(r"\bint\s+%s\s*\(hnumo_engine \*eng" % fn, hdr), fn
        assert f"name='{fn}'" in f90, fn
        assert re.search(r"\b%s\b" % fn, public), fn
        assert f"L.{fn}.argtypes" in py, fn
        assert re.search(r"def %s\(self" % fn[len("hnumo_"):], py), fn
    assert re.search(r"#define HNUMO_ABI_VERSION 10\b", hdr)      # additive: the version stays
    assert re.search(r"HNUMO_ABI_EXPECTED = 10\b", f90)
    for name, v in (("HNUMO_SAMPLE_STATE", 0), ("HNUMO_SAMPLE_STATS", 1)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr) and re.search(r"%s = %d\b" % (name, v), f90)
    assert (S.STATE, S.STATS) == (0, 1)


@pytest.mark.parametrize("ngl", [3, 4, 5, 6, 8])
def test_lagrange_weights(ngl):
    from hnumo.basis import lgl
    xgl = lgl(ngl)[0]
    for a in range(ngl):
        assert np.array_equal(S.lagrange_weights(xgl, xgl[a]), np.eye(ngl)[a])
    assert np.array_equal(S.lagrange_weights(xgl, xgl), np.eye(ngl))
    rng = np.random.default_rng(ngl)
    x = rng.uniform(-1.0, 1.0, 1000)
    w = S.lagrange_weights(xgl, x)
    assert w.shape == (ngl, 1000)
    # each weight carries 2(ngl-1) roundings and the weights are O(1)
    assert np.abs(w.sum(axis=0) - 1.0).max() <= 4 * ngl ** 2 * EPS
    # the formula, on plain floats: each factor a quotient first, multiplied in the order of m
    for p in range(5):
        for i in range(ngl):
            r = 1.0
            for m in range(ngl):
                if m != i:
                    r = r * ((float(x[p]) - float(xgl[m])) / (float(xgl[i]) - float(xgl[m])))
            assert w[i, p] == r
    assert np.array_equal(S.lagrange_weights(xgl, float(x[3])), w[:, 3])


def oracle_state(case_factory, name, kw, nsteps=2):
    """The CPU oracle's state after nsteps of the case (computed once)."""
    key = (name, tuple(sorted(kw.items())), nsteps)
    if key not in _states:
        import oracle as O
        case = case_factory(name, **kw)
        o = O.Oracle(case)
        q, qb, qp = o.state()
        for _ in range(nsteps):
            o.ti_rk_bcl(q, qb, qp)
        assert np.isfinite(q).all() and np.isfinite(qb).all()
        _states[key] = (case, q, qb)
    return _states[key]


def node_points(case):
    ngl, ne = case.scalars["ngl"], S.owned_elements(case)
    P = ngl * ngl
    xgl = S.case_xgl(case)
    e = np.repeat(np.arange(ne), P)
    ln = np.tile(np.arange(P), ne)
    return e + 1, xgl[ln % ngl], xgl[ln // ngl]


@pytest.mark.parametrize("name,kw", [("bump10", {"nop": 2}), ("dg25L3", {"nelx": 5, "nely": 3})])
def test_host_sampler_at_the_nodes_is_the_nodal_value(case_factory, name, kw):
    case, q, qb = oracle_state(case_factory, name, kw)
    L, npoin = case.scalars["nlayers"], case.scalars["npoin"]
    hs = S.HostSampler(case, *node_points(case))
    got = hs.sample(q, qb)
    assert got.shape == (5 * L + 4, npoin) and got.flags["F_CONTIGUOUS"]
    f5 = D.layer_fields(case, q)
    for k in range(L):
        assert np.array_equal(got[5 * k:5 * k + 5], f5[:, :, k]), k
    assert np.array_equal(got[5 * L:], qb[0:4])
    assert (q[1] != 0).any()                                    # a state that moves
    # the statistics' rows: any (5, npoin, L) fields
    hs2 = S.HostSampler(case, *node_points(case), source=S.STATS)
    gs = hs2.sample_stats(f5)
    assert gs.shape == (5 * L, npoin)
    for k in range(L):
        assert np.array_equal(gs[5 * k:5 * k + 5], f5[:, :, k])
    # points with elem = 0 read 0.0 in every row; the rest do not change
    elem, xi, eta = node_points(case)
    elem = elem.copy()
    elem[::3] = 0
    g0 = S.HostSampler(case, elem, xi, eta).sample(q, qb)
    assert not g0[:, ::3].any() and np.array_equal(g0[:, elem > 0], got[:, elem > 0])


def test_host_sampler_reproduces_polynomials_on_an_affine_brick(case_factory):
    """dp = a polynomial of degree <= N in x and in y: the interpolant is that polynomial, so random
    interior points return it within the project's second-line tolerance, 1e-10 relative."""
    case = case_factory("dg25L3", nelx=5, nely=3)
    N, ngl, L = case.scalars["ngl"] - 1, case.scalars["ngl"], case.scalars["nlayers"]
    coord = np.asarray(case.arrays["coord"])
    sx, sy = coord[0].max(), coord[1].max()
    rng = np.random.default_rng(2)
    cx, cy = rng.uniform(0.5, 1.5, N + 1), rng.uniform(0.5, 1.5, N + 1)

    def poly(x, y):
        return 100.0 + np.polyval(cx, x / sx) * np.polyval(cy, y / sy)

    q = np.array(case.arrays["q_df"], order="F")
    qb = np.array(case.arrays["qb_df"], order="F")
    q[0, :, 0] = poly(coord[0], coord[1])
    M = 500
    ne, P = case.scalars["nelem"], ngl * ngl
    e = rng.integers(0, ne, M)
    xi, eta = rng.uniform(-1, 1, M), rng.uniform(-1, 1, M)
    # the affine map of the brick's elements from their corner nodes
    x0, x1 = coord[0, e * P], coord[0, e * P + ngl - 1]
    y0, y1 = coord[1, e * P], coord[1, e * P + P - 1]
    x, y = 0.5 * ((1 - xi) * x0 + (1 + xi) * x1), 0.5 * ((1 - eta) * y0 + (1 + eta) * y1)
    got = S.HostSampler(case, e + 1, xi, eta).sample(q, qb)
    want = poly(x, y)
    assert got.shape == (5 * L + 4, M)
    rel = np.abs(got[3] - want).max() / np.abs(want).max()
    print("polynomial reproduction, max relative error", rel)
    assert rel <= 1e-10
    assert np.ptp(want) > 0.1 * np.abs(want).max()              # the polynomial varies over the points


def test_host_sampler_rejects_bad_points(case_factory):
    case = case_factory("bump10", nop=2)
    ne = case.scalars["nelem"]
    for elem, xi, eta in (([ne + 1], [0.0], [0.0]), ([-1], [0.0], [0.0]), ([1], [1.5], [0.0]), ([1], [0.0], [np.nan]),
                          ([1, 2], [0.0], [0.0]), ([], [], [])):
        with pytest.raises(ValueError):
            S.HostSampler(case, elem, xi, eta)


def test_regular_grid(case_factory):
    case = case_factory("dg25L3", nelx=5, nely=3)
    xi, yi, xy = S.regular_grid(case, 300.0e3, 700.0e3)
    assert np.array_equal(xi, np.arange(7) * 300.0e3) and np.array_equal(yi, np.arange(3) * 700.0e3)
    X, Y = np.meshgrid(xi, yi)
    assert xy.shape == (2, 21) and np.array_equal(xy[0], X.reshape(-1, order="F")) and np.array_equal(xy[1], Y.reshape(-1, order="F"))
    xi, yi, xy = S.regular_grid(case, 2000.0e3, 2000.0e3)      # i*dx <= xmax - xmin: both ends
    assert np.array_equal(xi, [0.0, 2000.0e3]) and np.array_equal(yi, [0.0, 2000.0e3])
    xi, yi, xy = S.regular_grid(case, 2000.0e3 * (1 + EPS), 3.0e9)
    assert xi.size == 1 and yi.size == 1 and xy.shape == (2, 1)
    with pytest.raises(ValueError):
        S.regular_grid(case, 0.0, 1.0)


def test_write_ssh_grid(tmp_path):
    xi, yi = np.array([0.0, 20.0e3, 40.0e3]), np.array([-1.0e3, 19.0e3])          # nx = 3, ny = 2
    ssh = np.array([[0.125, -1.5, 2.0], [1.0 / 3.0, 1.0e-17, -123456.789]])      # (ny, nx)
    p = tmp_path / "numo0001"
    S.write_ssh_grid(str(p), xi, yi, ssh)
    X = [0.0, 0.0, 20.0, 20.0, 40.0, 40.0]                      # meshgrid arrays, column-major
    Y = [-1.0, 19.0] * 3
    Z = [0.125, 1.0 / 3.0, -1.5, 1.0e-17, 2.0, -123456.789]
    want = "".join("%23.16f\n" % v for v in X + Y + Z).encode()
    assert p.read_bytes() == want
    assert want.splitlines()[0] == b"     0.0000000000000000" and len(want) == 18 * 24 + 1   # (one value is a character wider)
    assert b"-123456.7890000000043074\n" in want
    S.write_ssh_grid(str(p), xi, yi, np.array(Z))               # flat, already in that order
    assert p.read_bytes() == want
    with pytest.raises(ValueError):
        S.write_ssh_grid(str(p), xi, yi, ssh.T)
