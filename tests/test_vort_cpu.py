"""Vorticity products (hnumo_vort_*, hnumo/vorticity.py), the parts that need no GPU: the index order
of dpsi, the numpy mirror HostVorticity against analytic fields (checks that do not go through a second
implementation), the series' summation order, partitions, time_loop and the sample sets' VORT source.

The analytic bound is computed from the test's inputs, not chosen:

    B = 64 * eps * ngl * max|D| * max(|u|, |v|) * max(|ksi_x| + |ksi_y| + |eta_x| + |eta_y|)

-- the forward rounding bound of the four ngl-term sums D*u (each term within eps of its product, the
partial sums below ngl*max|D|*max|u|) times the metric factors they are multiplied with, with a factor
64 of slack for the roundings of the inputs, of the metric terms and of the few operations after."""
import io

import numpy as np
import pytest

import states
from hnumo import sample as S
from hnumo import vorticity as V
from hnumo.basis import Basis
from hnumo.flowstats import tree_sum

EPS = np.finfo(np.float64).eps
OMEGA = 1.0e-5

# the warped quadrilaterals and the brick: (name, overrides)
GRIDS = [("qmbump8", {}), ("dg25L3", {"nelx": 5, "nely": 3}), ("bump10", {"nop": 2}),
         ("dg25N7L3", {"nelx": 3, "nely": 3})]


@pytest.mark.parametrize("nop", [2, 4, 7])
def test_dpsi_is_indexed_basis_function_first(nop):
    """D(m,i) = dpsi[m, i] = l_m'(xgl_i): the derivative of the interpolant of x is 1 at every node.
    With the transposed matrix the same sums are not."""
    b = Basis(nop)
    D, x, ngl = b.dpsi, b.xgl, nop + 1
    tol = 64 * EPS * ngl * np.abs(D).max() * np.abs(x).max()
    for M, ok in ((D, True), (D.T, False)):
        s = np.zeros(ngl)
        for i in range(ngl):
            acc = M[0, i] * x[0]
            for m in range(1, ngl):
                acc = acc + M[m, i] * x[m]
            s[i] = acc
        assert (np.abs(s - 1.0) <= tol).all() == ok, (nop, ok, s)


def bound(case, umax):
    A, ngl = case.arrays, case.scalars["ngl"]
    met = sum(np.abs(np.asarray(A[k])) for k in ("ksi_x", "ksi_y", "eta_x", "eta_y")).max()
    return 64 * EPS * ngl * np.abs(np.asarray(A["dpsi"])).max() * umax * met


def state_of(case, u, v):
    """q_df of the case's own thicknesses moving with (u, v)(npoin)."""
    q = np.array(case.arrays["q_df"], order="F")
    for k in range(case.scalars["nlayers"]):
        q[1, :, k] = u * q[0, :, k]
        q[2, :, k] = v * q[0, :, k]
    return q


@pytest.mark.parametrize("name,kw", GRIDS)
def test_solid_body_rotation(case_factory, name, kw):
    """u = -W(y - yc), v = W(x - xc): a degree-1 field is Q1 in (xi, eta) on any bilinear element, so it
    is represented exactly, and zeta = 2W, delta = 0, ow = -4W^2, pv = (2W + f)/h, G = 2W * sum(w)."""
    case = case_factory(name, **kw)
    A, Sc, cfg = case.arrays, case.scalars, case.cfg
    x, y = np.asarray(A["coord"][0]), np.asarray(A["coord"][1])
    xc, yc = 0.5 * (cfg["xdims"][0] + cfg["xdims"][1]), 0.5 * (cfg["ydims"][0] + cfg["ydims"][1])
    u, v = -OMEGA * (y - yc), OMEGA * (x - xc)
    q = state_of(case, u, v)
    hv = V.HostVorticity(case)
    f = hv.fields(q)
    B = bound(case, max(np.abs(u).max(), np.abs(v).max()))
    assert B < 1e-3 * OMEGA                                       # the bound means something
    zeta, delta, pv, ow = f
    assert np.abs(zeta - 2 * OMEGA).max() <= B, (np.abs(zeta - 2 * OMEGA).max(), B)
    assert np.abs(delta).max() <= B, (np.abs(delta).max(), B)
    # sn, ss within B of 0 and zeta within B of 2W: |ow + 4W^2| <= 2B^2 + (4W B + B^2), and the rounding
    # of the squares and of the two sums
    B_ow = 4 * OMEGA * B + 3 * B * B + 8 * EPS * 4 * OMEGA ** 2
    assert np.abs(ow + 4 * OMEGA ** 2).max() <= B_ow, (np.abs(ow + 4 * OMEGA ** 2).max(), B_ow)
    fc = V.coriolis_of(case)
    for k in range(Sc["nlayers"]):
        h = (A["alpha"][k] / Sc["gravity"]) * q[0, :, k]
        exact = (2 * OMEGA + fc) / h
        B_pv = (B + 4 * EPS * (2 * OMEGA + np.abs(fc).max())) / h.min()
        assert np.abs(pv[:, k] - exact).max() <= B_pv, (k, np.abs(pv[:, k] - exact).max(), B_pv)
    if cfg["beta"]:
        assert np.ptp(fc) > 0 and np.abs(hv.fields(q)[2] - V.HostVorticity(case, coriolis=False).fields(q)[2]).max() > 0
    sw = float(np.asarray(A["jac"]).sum())
    G = hv.entry(q)[2]
    assert np.abs(G - 2 * OMEGA * sw).max() <= B * sw, (G, 2 * OMEGA * sw, B * sw)


@pytest.mark.parametrize("name,kw", GRIDS[1:])
def test_polynomial_field_on_the_brick(case_factory, name, kw):
    """A field of degree N in each of x and y on affine elements against its analytic derivatives."""
    case = case_factory(name, **kw)
    A, cfg, N = case.arrays, case.cfg, case.scalars["ngl"] - 1
    Lx, Ly = cfg["xdims"][1] - cfg["xdims"][0], cfg["ydims"][1] - cfg["ydims"][0]
    X = (np.asarray(A["coord"][0]) - cfg["xdims"][0]) / Lx
    Y = (np.asarray(A["coord"][1]) - cfg["ydims"][0]) / Ly
    U0 = OMEGA * Lx
    u = U0 * (X ** N - 0.5 * X) * (1.0 + Y ** N)
    v = U0 * (0.25 + X ** N) * (Y ** N - 0.75 * Y)
    u_x = U0 * (N * X ** (N - 1) - 0.5) * (1.0 + Y ** N) / Lx
    u_y = U0 * (X ** N - 0.5 * X) * (N * Y ** (N - 1)) / Ly
    v_x = U0 * (N * X ** (N - 1)) * (Y ** N - 0.75 * Y) / Lx
    v_y = U0 * (0.25 + X ** N) * (N * Y ** (N - 1) - 0.75) / Ly
    zeta, delta, _, ow = V.HostVorticity(case).fields(state_of(case, u, v))[:, :, 0]
    B = bound(case, max(np.abs(u).max(), np.abs(v).max()))
    assert np.abs(v_x - u_y).max() > 1e6 * B                      # the field is far from trivial
    assert np.abs(zeta - (v_x - u_y)).max() <= B
    assert np.abs(delta - (u_x + v_y)).max() <= B
    # each of sn, ss, zeta within B of its exact value g: |g'^2 - g^2| <= 2|g| B + B^2, three of them
    gmax = max(np.abs(u_x - v_y).max(), np.abs(v_x + u_y).max(), np.abs(v_x - u_y).max())
    exact = ((u_x - v_y) ** 2 + (v_x + u_y) ** 2) - (v_x - u_y) ** 2
    B_ow = 3 * (2 * gmax * B + B * B) + 8 * EPS * 3 * gmax ** 2
    assert np.abs(ow - exact).max() <= B_ow, (np.abs(ow - exact).max(), B_ow)


def test_series_bits_do_not_depend_on_the_chunks(case_factory):
    """tree_sum over the element partials = the tree over aligned 1024-element chunks followed by the
    tree over the chunk results, at E = 1369 (two chunks, the second ragged)."""
    case = states.moving_case(case_factory("dg25L3", nelx=37, nely=37, nop=2))
    hv = V.HostVorticity(case)
    q = np.asarray(case.arrays["q_df"])
    el = hv.element_sums(q)
    assert el.shape == (3, 3, 1369)
    entry = hv.entry(q)
    assert np.isfinite(entry).all() and (entry[0] > 0).all()
    for c in range(3):
        for k in range(3):
            x = el[c, k]
            chunks = [tree_sum(x[i:i + 1024]) for i in range(0, x.size, 1024)]
            assert len(chunks) == 2 and tree_sum(chunks) == entry[c, k]


def rank_cases(case, kind):
    if kind == "ghost":
        from hnumo.partition import partition
        return [partition(case, 2, r) for r in range(2)]
    from hnumo.facepart import face_partition
    return [face_partition(case, 2, r, "block") for r in range(2)]


@pytest.mark.parametrize("kind", ["ghost", "face"])
def test_partitions_equal_the_single_rank_mirror(case_factory, kind):
    """Nothing crosses an element: a rank's owned nodes carry the single-rank fields of the same global
    nodes, bit for bit; nodes of ghost elements read 0."""
    case = states.moving_case(case_factory("dg25L3", nelx=4, nely=2))
    P = case.scalars["ngl"] ** 2
    q = np.asarray(case.arrays["q_df"])
    whole = V.HostVorticity(case).fields(q)
    assert np.abs(whole[0]).max() > 0
    for pc in rank_cases(case, kind):
        f = V.HostVorticity(pc).fields(np.asarray(pc.arrays["q_df"]))
        ne = pc.nelem_owned
        assert 0 < ne < case.scalars["nelem"]
        if kind == "ghost":
            assert ne < pc.scalars["nelem"] and not f[:, ne * P:].any()
        gn = (np.asarray(pc.elems[:ne])[:, None] * P + np.arange(P)[None, :]).ravel()
        assert np.array_equal(f[:, :ne * P], whole[:, gn])


def test_time_loop_samples_every_vort_every_th_step(case_factory, tmp_path):
    import oracle as O
    from hnumo import diagnostics as D
    case = states.moving_case(case_factory("bump10", nop=2))
    dt = case.scalars["dt"]
    hv = V.HostVorticity(case)
    D.time_loop(case, O.Oracle(case), 4 * dt, out_dir=str(tmp_path), out=io.StringIO(), lcheck_conserved=False,
                lprint_diagnostics=False, vorticity=hv, vort_every=2)
    o = O.Oracle(case)
    q, qb, qp = o.state()
    want = []
    for s in range(4):
        o.ti_rk_bcl(q, qb, qp)
        if s % 2 == 1:
            want.append(V.HostVorticity(case).entry(q))
    ser = hv.series
    assert ser.shape == (3, case.scalars["nlayers"], 2)
    assert np.array_equal(ser[:, :, 0], want[0]) and np.array_equal(ser[:, :, 1], want[1])
    assert not np.array_equal(want[0], want[1])
    with pytest.raises(ValueError):
        D.time_loop(case, O.Oracle(case), dt, out_dir=str(tmp_path), out=io.StringIO(), vorticity=hv, vort_every=0)


def test_host_sampler_vort_source_returns_the_nodal_field_at_the_nodes(case_factory):
    case = states.moving_case(case_factory("qmbump8"))
    ngl, L = case.scalars["ngl"], case.scalars["nlayers"]
    P = ngl * ngl
    xgl = S.case_xgl(case)
    f = V.HostVorticity(case).fields(np.asarray(case.arrays["q_df"]))
    elems = np.array([1, 7, 64])
    e, b, a = (x.ravel() for x in np.meshgrid(elems, np.arange(ngl), np.arange(ngl), indexing="ij"))
    hs = S.HostSampler(case, e, xgl[a], xgl[b], source=S.VORT)
    got = hs.sample_vort(f)
    assert got.shape == (S.nval(L, S.VORT), e.size) == (4 * L, e.size)
    node = (e - 1) * P + b * ngl + a
    for k in range(L):
        assert np.array_equal(got[4 * k:4 * k + 4], f[:, node, k])
    assert np.abs(got).max() > 0
