"""Region sets (hnumo_regions_*, hnumo/regions.py), the parts that need no GPU: the numpy mirror HostRegions
against analytic integrals (checks that do not go through a second implementation), against the whole-domain
series of HostFlowStats and HostVorticity bit for bit, the partition sum, empty regions, label 0, the label
helpers, the overturning and time_loop.

Bounds, from the inputs:

    uniform flow       TU_k(r) = u0*h0_k*area_r to 1e-10 relative: DESIGN.md §3's second-line tolerance
    solid body         |G(r) - 2W*area_r| <= B*area_r, B the forward bound of tests/test_vort_cpu.py
    partition sum      |sum_r x(r) - x(all)| <= 2*eps*(ceil(log2 ne) + R)*sum_e |element partial|: the
                       first-order bound of a pairwise sum of ne terms (log2 ne roundings on a term's path)
                       for either side, plus the R - 1 adds of the regions, with a factor 2
"""
import io
import math

import numpy as np
import pytest

import states
from hnumo import flowstats as F
from hnumo import regions as RG
from hnumo import vorticity as V

EPS = np.finfo(np.float64).eps
OMEGA = 1.0e-5


def thirds(case, extra_empty=0):
    """labels by element number modulo: three uneven regions, every 7th element unlabelled"""
    ne = RG._owned(case)
    e = np.arange(ne)
    lab = np.where(e % 7 == 3, 0, np.where(e % 5 < 1, 1, np.where(e % 5 < 3, 2, 3))).astype(np.int32)
    return lab, 3 + extra_empty


def oracle_state(case, nsteps=1):
    import oracle as O
    o = O.Oracle(case)
    q, qb, qp = o.state()
    for _ in range(nsteps):
        o.ti_rk_bcl(q, qb, qp)
    assert np.isfinite(q).all()
    return q


_oracle = {}


@pytest.fixture(scope="module")
def moved(case_factory):
    """(case, q after one oracle step from the moving state), once"""
    if "s" not in _oracle:
        case = states.moving_case(case_factory("bump10", nop=2))
        _oracle["s"] = (case, oracle_state(case))
    return _oracle["s"]


@pytest.mark.parametrize("name,kw", [("qmbump8", {}), ("dg25L3", {"nelx": 5, "nely": 3})])
def test_uniform_flow_transport_is_u0_h0_area(case_factory, name, kw):
    case = case_factory(name, **kw)
    A, Sc = case.arrays, case.scalars
    L, P, ne = Sc["nlayers"], Sc["ngl"] ** 2, Sc["nelem"]
    u0, v0 = 0.3, -0.2
    q = np.zeros_like(np.asarray(A["q_df"]), order="F")
    dp0 = [900.0 + 250.0 * k for k in range(L)]
    for k in range(L):
        q[0, :, k], q[1, :, k], q[2, :, k] = dp0[k], u0 * dp0[k], v0 * dp0[k]
    lab, R = thirds(case)
    hr = RG.HostRegions(case, lab, R, RG.FLOW)
    e = hr.entry(q)
    # the areas independently: the plain sum of jac over the region's nodes
    w = np.asarray(A["jac"], dtype=np.float64).reshape(-1, order="F")[:ne * P].reshape(ne, P)
    for r in range(R):
        area = w[lab == r + 1].sum()
        assert area > 0 and abs(hr.area[r] - area) <= 1e-10 * area
        for k in range(L):
            h0 = (A["alpha"][k] / Sc["gravity"]) * dp0[k]
            for c, exact in ((0, h0 * area), (1, u0 * h0 * area), (2, v0 * h0 * area), (3, 0.5 * (u0 * u0 + v0 * v0) * h0 * area)):
                got = e[4 * k + c, r]
                assert abs(got - exact) <= 1e-10 * abs(exact), (name, r, k, c, got, exact)


@pytest.mark.parametrize("name,kw", [("qmbump8", {}), ("dg25L3", {"nelx": 5, "nely": 3})])
def test_solid_body_circulation_is_two_omega_area(case_factory, name, kw):
    """u = -W(y - yc), v = W(x - xc): zeta = 2W exactly on bilinear elements, so G(r) = 2W*area_r."""
    case = case_factory(name, **kw)
    A, Sc, cfg = case.arrays, case.scalars, case.cfg
    L, P, ne, ngl = Sc["nlayers"], Sc["ngl"] ** 2, Sc["nelem"], Sc["ngl"]
    x, y = np.asarray(A["coord"][0]), np.asarray(A["coord"][1])
    xc, yc = 0.5 * (cfg["xdims"][0] + cfg["xdims"][1]), 0.5 * (cfg["ydims"][0] + cfg["ydims"][1])
    u, v = -OMEGA * (y - yc), OMEGA * (x - xc)
    q = np.array(A["q_df"], order="F")
    for k in range(L):
        q[1, :, k], q[2, :, k] = u * q[0, :, k], v * q[0, :, k]
    met = sum(np.abs(np.asarray(A[k])) for k in ("ksi_x", "ksi_y", "eta_x", "eta_y")).max()
    B = 64 * EPS * ngl * np.abs(np.asarray(A["dpsi"])).max() * max(np.abs(u).max(), np.abs(v).max()) * met
    assert B < 1e-3 * OMEGA
    lab, R = thirds(case)
    hr = RG.HostRegions(case, lab, R, RG.VORT, coriolis=True)
    e = hr.entry(q)
    w = np.asarray(A["jac"], dtype=np.float64).reshape(-1, order="F")[:ne * P].reshape(ne, P)
    for r in range(R):
        area = w[lab == r + 1].sum()
        for k in range(L):
            G = e[3 * k + 2, r]
            assert abs(G - 2 * OMEGA * area) <= B * area, (name, r, k, G, 2 * OMEGA * area, B * area)
            assert e[3 * k, r] > 0 and e[3 * k + 1, r] > 0


def test_whole_domain_region_has_the_bits_of_the_whole_domain_series(moved):
    case, q = moved
    L, ne = case.scalars["nlayers"], case.scalars["nelem"]
    hr = RG.HostRegions(case, np.ones(ne, np.int32), 1, RG.FLOW | RG.VORT, coriolis=True)
    hr.add(q)
    s = hr.series
    assert s.shape == (7 * L, 1, 1)
    fs = F.HostFlowStats(case)
    fs.add(q)
    hv = V.HostVorticity(case)
    hv.add(q)
    for k in range(L):
        assert s[4 * k + 3, 0, 0] == fs.series[0, k, 0] and s[4 * k, 0, 0] == fs.series[1, k, 0]
        for c in range(3):
            assert s[4 * L + 3 * k + c, 0, 0] == hv.series[c, k, 0]
    assert np.abs(s).min() > 0
    # rows alone are the same rows
    assert np.array_equal(RG.HostRegions(case, np.ones(ne, np.int32), 1, RG.FLOW).entry(q), s[:4 * L, :, 0])
    assert np.array_equal(RG.HostRegions(case, np.ones(ne, np.int32), 1, RG.VORT, coriolis=True).entry(q), s[4 * L:, :, 0])
    # f matters to PZ and to nothing else
    nof = RG.HostRegions(case, np.ones(ne, np.int32), 1, RG.VORT).entry(q)
    if case.cfg["f0"] or case.cfg["beta"]:
        assert (nof[1::3] != s[4 * L + 1::3, :, 0]).all()
    assert np.array_equal(nof[0::3], s[4 * L::3, :, 0]) and np.array_equal(nof[2::3], s[4 * L + 2::3, :, 0])


def test_regions_that_partition_the_mesh_sum_to_the_whole(moved):
    case, q = moved
    ne = case.scalars["nelem"]
    e = np.arange(ne)
    lab = (1 + (e * 7 + e // 3) % 4).astype(np.int32)             # four regions, every element in one
    R = 4
    assert set(lab) == {1, 2, 3, 4}
    hr = RG.HostRegions(case, lab, R, RG.FLOW | RG.VORT, coriolis=True)
    parts = hr.entry(q)
    whole = RG.HostRegions(case, np.ones(ne, np.int32), 1, RG.FLOW | RG.VORT, coriolis=True).entry(q)[:, 0]
    mag = np.abs(hr.element_sums(q)).sum(axis=1)
    bound = 2 * EPS * (math.ceil(math.log2(ne)) + R) * mag
    total = parts[:, 0]
    for r in range(1, R):
        total = total + parts[:, r]
    assert (np.abs(total - whole) <= bound).all(), (np.abs(total - whole), bound)
    assert (bound < 1e-12 * np.maximum(mag, 1e-300)).all()          # the bound means something
    assert hr.area.sum() > 0


def test_empty_regions_read_plus_zero_and_label_zero_is_excluded(moved):
    case, q = moved
    lab, R = thirds(case, extra_empty=2)                            # regions 4 and 5 have no element
    hr = RG.HostRegions(case, lab, R, RG.FLOW | RG.VORT)
    e = hr.entry(q)
    assert not e[:, 3:].any() and not np.signbit(e[:, 3:]).any()
    assert not hr.area[3:].any() and (hr.area[:3] > 0).all()
    assert (lab == 0).any()
    # moving the unlabelled elements' state changes nothing; labelling them does
    P = case.scalars["ngl"] ** 2
    q2 = q.copy(order="F")
    nodes = (np.flatnonzero(lab == 0)[:, None] * P + np.arange(P)[None, :]).ravel()
    q2[1:, nodes, :] *= 3.0
    assert np.array_equal(hr.entry(q2), e)
    lab1 = np.where(lab == 0, 1, lab).astype(np.int32)
    e1 = RG.HostRegions(case, lab1, R, RG.FLOW | RG.VORT).entry(q)
    assert (e1[:, 0] != e[:, 0]).any() and np.array_equal(e1[:, 1:], e[:, 1:])
    for bad, R_, rows in ((lab[:-1], R, RG.FLOW), (lab, 0, RG.FLOW), (lab, R, 0), (lab, R, 4), (lab + 9, R, RG.FLOW)):
        with pytest.raises(ValueError):
            RG.HostRegions(case, bad, R_, rows)


def test_strips_boxes_and_overturning(case_factory):
    case = case_factory("dg25L3", nelx=5, nely=3)
    cfg, L = case.cfg, case.scalars["nlayers"]
    (x0, x1), (y0, y1) = cfg["xdims"], cfg["ydims"]
    edges = np.linspace(y0, y1, 4)
    lab, R = RG.strips(case, 1, edges)
    assert R == 3 and lab.dtype == np.int32 and [int((lab == r).sum()) for r in (1, 2, 3)] == [5, 5, 5]
    cy = RG.centroids(case)[1]
    for r in range(1, 4):
        assert ((cy[lab == r] >= edges[r - 1]) & (cy[lab == r] < edges[r])).all()
    # a strip set that leaves the top third out: label 0 there
    lab2, R2 = RG.strips(case, 1, edges[:3])
    assert R2 == 2 and (lab2[lab == 3] == 0).all() and np.array_equal(lab2[lab != 3], lab[lab != 3])
    xm = x0 + 0.2 * (x1 - x0)
    labb, Rb = RG.boxes(case, [(x0, xm, y0, y1 + 1.0), (xm, x1 + 1.0, y0, y1 + 1.0)])
    assert Rb == 2 and int((labb == 1).sum()) == 3 and int((labb == 2).sum()) == 12
    with pytest.raises(ValueError):
        RG.strips(case, 1, [1.0, 1.0])
    # Psi: a uniform northward flow v0 carries v0*h_k*dx_total through every line of latitude
    A, Sc = case.arrays, case.scalars
    q = np.array(A["q_df"], order="F")
    v0 = 0.1
    for k in range(L):
        q[1, :, k], q[2, :, k] = 0.0, v0 * q[0, :, k]
    hr = RG.HostRegions(case, lab, R, RG.FLOW)
    hr.add(q)
    hr.add(q)
    widths = np.diff(edges)
    psi = RG.overturning(hr.series, hr.area, widths)
    assert psi.shape == (L, R, 2)
    acc = 0.0
    for k in range(L):
        hk = (A["alpha"][k] / Sc["gravity"]) * np.asarray(A["q_df"])[0, :, k]
        assert np.ptp(hk) <= 1e-12 * hk.max()                          # the rest state's layers are flat here
        acc = acc + v0 * hk[0] * (x1 - x0)
        assert np.abs(psi[k] - acc).max() <= 1e-10 * abs(acc), (k, psi[k], acc)
    assert np.array_equal(RG.overturning(hr.series, hr.area, widths, nlayers=L), psi)


def test_time_loop_samples_every_regions_every_th_step(case_factory, tmp_path):
    import oracle as O
    from hnumo import diagnostics as D
    case = states.moving_case(case_factory("bump10", nop=2))
    dt = case.scalars["dt"]
    lab, R = thirds(case)
    ne = case.scalars["nelem"]
    a = RG.HostRegions(case, lab, R, RG.FLOW | RG.VORT, coriolis=True)
    b = RG.HostRegions(case, np.ones(ne, np.int32), 1, RG.FLOW)
    D.time_loop(case, O.Oracle(case), 4 * dt, out_dir=str(tmp_path), out=io.StringIO(), lcheck_conserved=False,
                lprint_diagnostics=False, regions=[a, b], regions_every=2)
    o = O.Oracle(case)
    q, qb, qp = o.state()
    want = []
    for s in range(4):
        o.ti_rk_bcl(q, qb, qp)
        if s % 2 == 1:
            want.append((RG.HostRegions(case, lab, R, RG.FLOW | RG.VORT, coriolis=True).entry(q),
                         RG.HostRegions(case, np.ones(ne, np.int32), 1, RG.FLOW).entry(q)))
    assert a.series.shape == (7 * case.scalars["nlayers"], R, 2) and b.series.shape == (4 * case.scalars["nlayers"], 1, 2)
    for i in range(2):
        assert np.array_equal(a.series[:, :, i], want[i][0]) and np.array_equal(b.series[:, :, i], want[i][1])
    assert not np.array_equal(want[0][0], want[1][0])
    with pytest.raises(ValueError):
        D.time_loop(case, O.Oracle(case), dt, out_dir=str(tmp_path), out=io.StringIO(), regions=a, regions_every=0)
