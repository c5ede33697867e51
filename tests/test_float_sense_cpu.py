"""The float sets' sensors, the parts that need no GPU: the mirror HostFloats.sense against a HostSampler built by
hand at the same points, the STATE rows u, v against the record's own, potential vorticity along trajectories in
a solid-body rotation (the one check that goes through no second implementation of the interpolant's use: PV is
materially conserved, and a float is the observer that can see it), the trajectory files, merge_series on the
widened records and every refusal of the mirror.

The analytic bound is tests/test_vort_cpu.py's B for the nodal fields, carried to the float: a value is
sum_ij Lx[i] Ly[j] F_ij, so nodal values within B_F of a constant c give a value within lam * B_F + 8 ngl^2 eps
lam |c| of c, where lam = max over the floats of (sum_i |Lx[i]|)(sum_j |Ly[j]|) is computed from the weights
the test's own points have (the weights sum to 1 within 4 ngl^2 eps, tests/test_sample_cpu.py; the ngl^2 products
and sums each round once)."""
import io

import numpy as np
import pytest

import float_cases as FC
import float_migrate_cases as MC
from hnumo import floats as FL
from hnumo import sample as S
from hnumo import vorticity as V
from test_vort_cpu import EPS, OMEGA, bound

STATE, VORT = FL.SENSE_STATE, FL.SENSE_VORT


def advanced(case_factory, which, mask, nadv=3):
    case = FC.moving(case_factory, *FC.CASES[which])
    xy, layer = FC.seeds(case)
    q = case.arrays["q_df"]
    hf = FL.HostFloats(case, xy, layer, sensors=mask)
    dt = FC.big_dt(case, q)
    for _ in range(nadv):
        hf.advance(q, dt)
        hf.record()
    return case, q, hf


@pytest.mark.parametrize("which", [0, 2])
def test_rows_are_those_of_a_sampler_built_by_hand(case_factory, which):
    case, q, hf = advanced(case_factory, which, STATE | VORT)
    L, m, k = case.scalars["nlayers"], np.arange(hf.M), hf.layer - 1
    got = hf.sense(q)
    assert got.shape == (9, hf.M) and set(hf.layer) == set(range(1, L + 1))
    st = S.HostSampler(case, hf.elem, hf.xi, hf.eta, S.STATE).sample(q, np.asarray(case.arrays["qb_df"]))
    vt = S.HostSampler(case, hf.elem, hf.xi, hf.eta, S.VORT).sample_vort(V.HostVorticity(case).fields(q))
    for v in range(5):
        assert np.array_equal(got[v], st[5 * k + v, m]), v
    for v in range(4):
        assert np.array_equal(got[5 + v], vt[4 * k + v, m]), v
    # the masks select: STATE rows first
    assert np.array_equal(FL.HostFloats.sense(_with(hf, STATE), q), got[:5])
    assert np.array_equal(FL.HostFloats.sense(_with(hf, VORT), q), got[5:])
    off = hf.elem == 0
    assert off.any() and not got[:, off].any() and (got[:, ~off] != 0).any(axis=1).all() and np.isfinite(got).all()
    # the last record carries the same rows behind x, y, u, v, elem
    ser = hf.series()
    assert ser.shape == (14, hf.M, 3) and np.array_equal(ser[5:, :, -1], got)
    assert np.array_equal(ser[:5, :, -1], np.stack([hf.x, hf.y, hf.wx, hf.wy, hf.elem.astype(float)]))


def _with(hf, mask):
    import copy
    h2 = copy.copy(hf)
    h2._records = []
    h2.set_sensors(mask)
    return h2


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_state_rows_u_v_equal_the_records_own(case_factory, which):
    """After an advance the stored velocity is vel at the cached location: the same statement."""
    case, q, hf = advanced(case_factory, which, STATE)
    ser = hf.series()
    assert ser.shape == (10, hf.M, 3)
    assert np.array_equal(ser[6], ser[2]) and np.array_equal(ser[7], ser[3])
    assert (ser[2] != 0).sum() > ser[2].size // 2


@pytest.mark.parametrize("name,kw", [("qmbump8", {}), ("dg25L3", {"nelx": 5, "nely": 3})])
def test_pv_is_conserved_along_trajectories_in_solid_body_rotation(case_factory, name, kw):
    """u = -W(y - yc), v = W(x - xc) with a uniform thickness per layer and a uniform f: zeta = 2W, delta = 0 and
    pv = (2W + f)/h_k at every node, so along the whole trajectory of every active float."""
    case = case_factory(name, **kw)
    A, Sc, cfg = case.arrays, case.scalars, case.cfg
    L, ngl = Sc["nlayers"], Sc["ngl"]
    x, y = np.asarray(A["coord"][0]), np.asarray(A["coord"][1])
    xc, yc = 0.5 * (cfg["xdims"][0] + cfg["xdims"][1]), 0.5 * (cfg["ydims"][0] + cfg["ydims"][1])
    u, v = -OMEGA * (y - yc), OMEGA * (x - xc)
    q = np.zeros((3, Sc["npoin"], L), order="F")
    dp = [float(np.asarray(A["q_df"])[0, :, k].mean()) for k in range(L)]
    for k in range(L):
        q[0, :, k], q[1, :, k], q[2, :, k] = dp[k], u * dp[k], v * dp[k]
    f0 = 7.3e-5
    R = 0.5 * min(cfg["xdims"][1] - cfg["xdims"][0], cfg["ydims"][1] - cfg["ydims"][0])
    xy = np.concatenate([FL.seed_ring((xc, yc), r * R, 12, phase=0.1 * i) for i, r in enumerate((0.15, 0.4, 0.65, 0.85))], axis=1)
    layer = (np.arange(xy.shape[1]) % L + 1).astype(np.int32)
    hf = FL.HostFloats(case, xy, layer, sensors=STATE | VORT, coriolis=np.full(Sc["npoin"], f0))
    e0 = hf.elem.copy()
    assert (e0 > 0).all()
    nadv, theta = 16, 0.2
    lam = 0.0
    for _ in range(nadv):
        hf.advance(q, theta / OMEGA)
        hf.record()
        on = hf.elem > 0
        lx, ly = S.lagrange_weights(hf.xgl, hf.xi[on]), S.lagrange_weights(hf.xgl, hf.eta[on])
        lam = max(lam, float((np.abs(lx).sum(axis=0) * np.abs(ly).sum(axis=0)).max()))
    ser = hf.series()
    assert (hf.status == FL.ACTIVE).all() and (ser[4] > 0).all()
    assert (ser[4, :, -1] != e0).sum() > hf.M // 2                 # the floats went through elements
    ang = np.unwrap(np.arctan2(ser[1] - yc, ser[0] - xc), axis=1)
    assert (ang[:, -1] - ang[:, 0] > 0.9 * (nadv - 1) * np.arctan(theta)).all()
    B = bound(case, max(np.abs(u).max(), np.abs(v).max()))
    assert B < 1e-3 * OMEGA and 1.0 <= lam < 10.0
    carry = lambda BF, c: lam * BF + 8 * ngl * ngl * EPS * lam * abs(c)
    zeta, delta, pv = ser[10], ser[11], ser[12]
    assert np.abs(zeta - 2 * OMEGA).max() <= carry(B, 2 * OMEGA), (np.abs(zeta - 2 * OMEGA).max(), carry(B, 2 * OMEGA))
    assert np.abs(delta).max() <= carry(B, 0.0), (np.abs(delta).max(), carry(B, 0.0))
    for k in range(L):
        h = (A["alpha"][k] / Sc["gravity"]) * dp[k]
        exact = (2 * OMEGA + f0) / h
        B_pv = (B + 4 * EPS * (2 * OMEGA + f0)) / h                 # tests/test_vort_cpu.py's, h uniform
        mine = layer == k + 1
        err = np.abs(pv[mine] - exact).max()
        assert err <= carry(B_pv, exact), (k, err, carry(B_pv, exact))
        assert np.abs(ser[5][mine] - h).max() <= carry(2 * EPS * h, h)          # the thickness under the float


def test_trajectory_files_with_and_without_sensors(case_factory, tmp_path):
    case, q, hf = advanced(case_factory, 1, STATE | VORT)
    ser = hf.series()
    p = str(tmp_path / "t.npz")
    FL.write_trajectories(p, ser, hf.layer, hf.status, sensors=STATE | VORT)
    s2, l2, st2, mask = FL.read_trajectories(p, with_sensors=True)
    assert mask == 3 and np.array_equal(s2, ser) and np.array_equal(l2, hf.layer) and np.array_equal(st2, hf.status)
    assert len(FL.read_trajectories(p)) == 3
    # a 5-row series writes the bytes it always did: the three arrays and nothing else
    FL.write_trajectories(p, ser[:5], hf.layer, hf.status)
    buf = io.BytesIO()
    np.savez(buf, series=np.asarray(ser[:5], dtype=np.float64), layer=np.broadcast_to(np.asarray(hf.layer, np.int32), (hf.M,)),
             status=np.asarray(hf.status, np.int32).reshape(-1))
    assert open(p, "rb").read() == buf.getvalue()
    assert FL.read_trajectories(p, with_sensors=True)[3] == 0
    for bad_series, mask in ((ser, 0), (ser[:5], 1), (ser[:10], 2), (ser[:9], 3), (ser, 4), (ser, -1)):
        with pytest.raises(ValueError):
            FL.write_trajectories(p, bad_series, hf.layer, hf.status, sensors=mask)


def test_merge_series_carries_the_sensor_rows(case_factory):
    """Two processor-face ranks of bump10 with the migrating mirror: the merged (5 + S) series is the single-rank
    mirror's (merge_series is row-agnostic; element fields are the element's own, so a rank reads the same bits)."""
    case, parts = MC.partition(case_factory, MC.ROWS[0])
    xy, layer = MC.seeds(case, parts)
    q = case.arrays["q_df"]
    dt = FC.big_dt(case, q)
    one = FL.HostFloats(case, xy, layer, sensors=STATE | VORT)
    grp = FL.HostFloatGroup(parts, xy, layer, coord_scale=one.maxc)
    for hf in grp.ranks:
        hf.set_sensors(STATE | VORT)
    states = [p.arrays["q_df"] for p in parts]
    for _ in range(3):
        one.advance(q, dt)
        one.record()
        grp.advance(states, dt)
        grp.record()
    assert any(grp.crossings)
    merged = FL.merge_series(grp.series(), parts)
    ref = one.series()
    assert merged.shape == ref.shape == (14, one.M, 3)
    assert np.array_equal(merged, ref), int((merged != ref).sum())


def test_refusals_of_the_mirror(case_factory):
    case = FC.moving(case_factory, *FC.CASES[1])
    xy, layer = FC.seeds(case)
    q = case.arrays["q_df"]
    for bad in (4, 8, -1, 7):
        with pytest.raises(ValueError, match="mask"):
            FL.HostFloats(case, xy, layer, sensors=bad)
    hf = FL.HostFloats(case, xy, layer)
    with pytest.raises(ValueError, match="no sensors"):
        hf.sense(q)
    hf.set_sensors(STATE)
    with pytest.raises(ValueError, match="no state"):              # a record before any advance has no state to sense
        hf.record()
    assert hf.series().shape == (10, hf.M, 0)
    hf.advance(q)
    hf.record()
    with pytest.raises(ValueError, match="another width"):         # the series holds 10-row records
        hf.set_sensors(STATE | VORT)
    with pytest.raises(ValueError, match="another width"):
        hf.set_sensors(0)
    hf.set_sensors(STATE)                                            # (the same width: nothing changes)
    assert hf.series(clear=True).shape == (10, hf.M, 1)
    hf.set_sensors(VORT)
    hf.record()
    assert hf.series().shape == (9, hf.M, 1)
    with pytest.raises(ValueError, match="coriolis"):
        FL.HostFloats(case, xy, layer, sensors=VORT, coriolis=np.zeros(3)).sense(q)
    # a set without sensors is the set it always was
    h0 = FL.HostFloats(case, xy, layer)
    h0.record()
    assert h0.series().shape == (5, h0.M, 1)
