"""Sample sets on the device (kernels_sample.hip through hnumo_sample_*): samples and series equal
-- np.array_equal, no tolerance -- the numpy mirror hnumo.sample.HostSampler fed with the per-step
states of a second, non-resident engine on the same case (whose bits equal the resident engine's:
tests/test_engine_gpu.py).  The resident engine is read before any sync."""
import ctypes as C

import numpy as np
import pytest

from hnumo import flowstats as F
from hnumo import sample as S

pytestmark = pytest.mark.gpu
_runs = {}

# dg25L3 5x3: N=4 (P = 25), L=3, E = 15; bump10 at N=2: P = 9, L=2, E = 100; qmbump8: warped
# quadrilaterals; dg25N7L3 3x3: P = 64, L=3, where the arena holds K = 3 elements for E = 9
CASES = [("dg25L3", {"nelx": 5, "nely": 3}), ("bump10", {"nop": 2}), ("qmbump8", {}), ("dg25N7L3", {"nelx": 3, "nely": 3})]


def stepped_states(case_factory, name, kw, nsteps):
    """(case, [(q_df, qb_df) after step 1..nsteps], final (q, qb, qp)) from a non-resident engine
    (computed once per case)."""
    from hnumo.engine import Engine
    key = (name, tuple(sorted(kw.items())), nsteps)
    if key not in _runs:
        case = case_factory(name, **kw)
        e = Engine(case)
        q, qb, qp = e.state()
        out = []
        for _ in range(nsteps):
            e.ti_rk_bcl(q, qb, qp)
            out.append((q.copy(order="F"), qb.copy(order="F")))
        e.close()
        assert all(np.isfinite(a).all() and np.isfinite(b).all() for a, b in out)
        _runs[key] = (case, out, (q, qb, qp))
    return _runs[key]


def resident(case, nsteps):
    from hnumo.engine import Engine
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    for _ in range(nsteps):
        e.ti_rk_bcl(*st)
    return e, st


def node_points(case):
    ngl, ne = case.scalars["ngl"], S.owned_elements(case)
    P = ngl * ngl
    xgl = S.case_xgl(case)
    e = np.repeat(np.arange(ne), P)
    ln = np.tile(np.arange(P), ne)
    return (e + 1).astype(np.int32), np.stack([xgl[ln % ngl], xgl[ln // ngl]])


def grid_and_stations(case, nx=8):
    """regular_grid points (grid lines on the element edges of the brick cases) plus 5 stations off
    the grid: (xy (2, M), number of grid points)."""
    c = np.asarray(case.arrays["coord"])[0:2, :S.owned_elements(case) * case.scalars["ngl"] ** 2]
    lo, hi = c.min(axis=1), c.max(axis=1)
    xi, yi, xy = S.regular_grid(case, (hi[0] - lo[0]) / nx, (hi[1] - lo[1]) / 6)
    rng = np.random.default_rng(3)
    st = lo[:, None] + (hi - lo)[:, None] * rng.uniform(0.05, 0.95, (2, 5))
    return np.asfortranarray(np.concatenate([xy, st], axis=1)), xy.shape[1]


@pytest.mark.parametrize("name,kw", CASES)
def test_nodes_are_the_layer_fields_and_qb(case_factory, name, kw):
    case, states, _ = stepped_states(case_factory, name, kw, 2)
    L, npoin = case.scalars["nlayers"], case.scalars["npoin"]
    e, _ = resident(case, 2)
    elem, xe = node_points(case)
    ds = S.DeviceSampler(e, elem=elem, xi_eta=xe)
    got = ds.sample()
    f5 = e.layer_fields()
    e.close()
    assert got.shape == (5 * L + 4, npoin)
    for k in range(L):
        assert np.array_equal(got[5 * k:5 * k + 5], f5[:, :, k]), (name, k)
    q, qb = states[1]
    assert np.array_equal(got[5 * L:], qb[0:4])
    assert np.array_equal(got, S.HostSampler(case, elem, xe[0], xe[1]).sample(q, qb))
    assert (got[1] != 0).any()                                  # a state that moves


@pytest.mark.parametrize("name,kw", CASES)
def test_grid_and_stations_equal_mirror(case_factory, name, kw):
    case, states, _ = stepped_states(case_factory, name, kw, 2)
    xy, ngrid = grid_and_stations(case, nx=10 if name == "dg25L3" else 8)
    e, _ = resident(case, 2)
    ds = S.DeviceSampler(e, xy=xy)
    elem, xi, eta = ds.plan()
    got = ds.sample()
    again = ds.sample()
    e.close()
    assert (elem > 0).all() and (elem <= case.scalars["nelem"]).all()      # a rectangle of elements: every point located
    assert (np.abs(xi) <= 1).all() and (np.abs(eta) <= 1).all()
    assert (np.abs(xi[:ngrid]) >= 1 - 1e-12).any()              # grid points on element edges
    want = S.HostSampler(case, elem, xi, eta).sample(*states[1])
    assert got.shape == want.shape == (5 * case.scalars["nlayers"] + 4, xy.shape[1])
    assert np.array_equal(got, want), (name, float(np.abs(got - want).max()))
    assert np.array_equal(again, got)
    assert np.isfinite(got).all() and (got[3] > 0).all()


def ref_set_equals_mirror(case, states, elem, xi, eta, nsteps=2):
    e, _ = resident(case, nsteps)
    ds = S.DeviceSampler(e, elem=elem, xi_eta=np.stack([xi, eta]))
    got = ds.sample()
    e.close()
    want = S.HostSampler(case, elem, xi, eta).sample(*states[nsteps - 1])
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    return got


def test_700_points_in_one_element(case_factory):
    """Three chunks (256 + 256 + the rest) read the same element."""
    case, states, _ = stepped_states(case_factory, *CASES[0], 2)
    rng = np.random.default_rng(7)
    elem = np.concatenate([np.full(700, 8), [1, 4, 15, 0]]).astype(np.int32)
    rng.shuffle(elem)
    M = elem.size
    got = ref_set_equals_mirror(case, states, elem, rng.uniform(-1, 1, M), rng.uniform(-1, 1, M))
    assert not got[:, elem == 0].any() and (got[3][elem > 0] > 0).all()


def test_more_elements_than_arena_slots(case_factory):
    """One point per element at N=7, L=3: 9 elements, K = 3 per chunk."""
    case, states, _ = stepped_states(case_factory, *CASES[3], 2)
    ne = case.scalars["nelem"]
    assert ne == 9 and 32768 // (8 * ((19 * 64) | 1)) == 3
    rng = np.random.default_rng(8)
    ref_set_equals_mirror(case, states, np.arange(ne, 0, -1).astype(np.int32), rng.uniform(-1, 1, ne), rng.uniform(-1, 1, ne))


@pytest.mark.parametrize("M", [1, 257])
def test_one_point_and_one_more_than_a_chunk(case_factory, M):
    case, states, _ = stepped_states(case_factory, *CASES[1], 2)
    rng = np.random.default_rng(M)
    elem = rng.integers(1, 4, M).astype(np.int32)               # few elements: the 257th point opens a chunk
    ref_set_equals_mirror(case, states, elem, rng.uniform(-1, 1, M), rng.uniform(-1, 1, M))


def test_shuffled_points_give_the_shuffled_output(case_factory):
    case, states, _ = stepped_states(case_factory, *CASES[0], 2)
    xy, _ = grid_and_stations(case, nx=10)
    rng = np.random.default_rng(9)
    p = rng.permutation(xy.shape[1])
    e, _ = resident(case, 2)
    a = S.DeviceSampler(e, xy=xy)
    b = S.DeviceSampler(e, xy=np.asfortranarray(xy[:, p]))
    ga, gb = a.sample(), b.sample()
    pa, pb = a.plan(), b.plan()
    e.close()
    assert all(np.array_equal(x[p], y) for x, y in zip(pa, pb))
    assert np.array_equal(ga[:, p], gb) and (p != np.arange(p.size)).any()


def code_of(fn, *a):
    from hnumo.engine import EngineError
    with pytest.raises(EngineError) as ei:
        fn(*a)
    assert str(ei.value).split("): ", 1)[1].strip(), "empty message"
    return ei.value.code


def test_series_every_second_step_equals_explicit_records(case_factory):
    """every=2 over 4 steps = explicit records after steps 2 and 4; both runs end on the bits of a
    run with no set."""
    from hnumo.engine import Engine
    case, states, final = stepped_states(case_factory, "bump10", {}, 4)
    xy, _ = grid_and_stations(case)
    out = {}
    for mode in ("every", "explicit"):
        e = Engine(case)
        q, qb, qp = e.state()
        e.set_resident(True)
        ds = S.DeviceSampler(e, xy=xy)
        ds.series_begin(every=2 if mode == "every" else 0, capacity=4)
        for s in range(4):
            e.ti_rk_bcl(q, qb, qp)
            if mode == "explicit" and s % 2 == 1:
                ds.record()
        out[mode] = ds.series()
        hs = ds.host_sampler()
        e.sync(q, qb, qp)
        e.close()
        for a, b in zip((q, qb, qp), final):
            assert np.array_equal(a, b), mode
    want = np.stack([hs.sample(*states[1]), hs.sample(*states[3])], axis=2)
    assert out["every"].shape == want.shape == (14, xy.shape[1], 2)
    assert np.array_equal(out["every"], want) and np.array_equal(out["explicit"], want)
    assert not np.array_equal(want[:, :, 0], want[:, :, 1])


def test_full_series_fails_the_step_call_with_the_step_done(case_factory):
    from hnumo.engine import Engine
    case, states, _ = stepped_states(case_factory, "bump10", {"nop": 2}, 3)
    e = Engine(case)
    q, qb, qp = e.state()
    e.set_resident(True)
    elem, xe = node_points(case)
    ds = S.DeviceSampler(e, elem=elem[:40], xi_eta=xe[:, :40] * 0.5)
    hs = ds.host_sampler()
    ds.series_begin(every=1, capacity=1)
    e.ti_rk_bcl(q, qb, qp)
    assert code_of(e.ti_rk_bcl, q, qb, qp) == 4                 # the second recording step: done, not recorded
    assert code_of(ds.record) == 4
    assert np.array_equal(ds.sample(), hs.sample(*states[1]))   # the state is that of step 2
    ser = ds.series(clear=True)
    assert ser.shape[2] == 1 and np.array_equal(ser[:, :, 0], hs.sample(*states[0]))
    assert ds.series().shape[2] == 0                            # clear emptied it
    e.ti_rk_bcl(q, qb, qp)                                      # room again: step 3 is recorded
    ser = ds.series()
    assert ser.shape[2] == 1 and np.array_equal(ser[:, :, 0], hs.sample(*states[2]))
    e.close()


def test_statistics_source(case_factory):
    """A STATS set with every=1 beside hnumo_stats_begin(every=1): series entry i is the mirror's
    fields after i + 1 samples, sampled by the mirror."""
    from hnumo.engine import Engine
    case, states, _ = stepped_states(case_factory, "dg25L3", {"nelx": 5, "nely": 3}, 3)
    xy, _ = grid_and_stations(case, nx=10)
    e = Engine(case)
    q, qb, qp = e.state()
    e.set_resident(True)
    ds = S.DeviceSampler(e, xy=xy, source=S.STATS)
    hs = ds.host_sampler()
    ds.series_begin(every=1, capacity=3)
    assert code_of(ds.sample) == 4                              # no state on the device yet
    assert code_of(e.ti_rk_bcl, q, qb, qp) == 4                 # before hnumo_stats_begin: the step is done, not recorded
    assert code_of(ds.sample) == 4 and code_of(ds.record) == 4
    assert ds.series().shape == (15, xy.shape[1], 0)
    e.close()

    e = Engine(case)
    q, qb, qp = e.state()
    e.set_resident(True)
    ds = S.DeviceSampler(e, xy=xy, source=S.STATS)
    e.stats_begin(every=0, series=0)
    e.ti_rk_bcl(q, qb, qp)
    assert code_of(ds.sample) == 4                              # statistics begun, but no samples
    e.close()

    e = Engine(case)
    q, qb, qp = e.state()
    e.set_resident(True)
    ds = S.DeviceSampler(e, xy=xy, source=S.STATS)
    e.stats_begin(every=1, series=0)
    ds.series_begin(every=1, capacity=3)
    for _ in range(3):
        e.ti_rk_bcl(q, qb, qp)
    ser = ds.series()
    now = ds.sample()
    dev_fields = e.stats_fields()
    e.close()
    host = F.HostFlowStats(case, series=False)
    assert ser.shape == (15, xy.shape[1], 3)
    for i in range(3):
        host.add(states[i][0])
        assert np.array_equal(ser[:, :, i], hs.sample_stats(host.fields())), i
    assert np.array_equal(now, ser[:, :, 2]) and np.array_equal(dev_fields, host.fields())
    assert np.isfinite(ser).all() and (ser[0] > 0).all()


def test_redone_step_is_recorded_once(case_factory, monkeypatch):
    """The corrector's persistent launch of the first step gives up (hnumo_debug_force_abort(1)) and
    the step is redone on per-stage launches: 3 steps record 3 samples, those of an engine on
    per-stage launches from the start."""
    from hnumo.engine import Engine
    case = case_factory("dg25L3", nelx=5, nely=3)
    xy, _ = grid_and_stations(case, nx=10)
    monkeypatch.setenv("HNUMO_PERSISTENT", "0")
    e0 = Engine(case)
    monkeypatch.delenv("HNUMO_PERSISTENT")
    e = Engine(case)
    assert e.stage_path == "persistent" and e0.stage_path == "per-stage"
    e.debug_force_abort(1)
    out = []
    for eng in (e, e0):
        st = eng.state()
        eng.set_resident(True)
        ds = S.DeviceSampler(eng, xy=xy)
        ds.series_begin(every=1, capacity=4)
        for _ in range(3):
            eng.ti_rk_bcl(*st)
        out.append(ds.series())
    assert e.persistent_stats["aborts"] == 1
    e.close()
    e0.close()
    assert out[0].shape == (19, xy.shape[1], 3)
    assert np.array_equal(out[0], out[1])
    assert not np.array_equal(out[0][:, :, 0], out[0][:, :, 1])


def group_run(parts, xy, nsteps=2):
    """The ranks `parts` as a local exchange group with a grid set each, every=1: per rank the plan,
    the series, and the mirror's samples of that rank's synced states."""
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    engines = [Engine(p) for p in parts]
    local_group(engines)
    sets = [S.DeviceSampler(e, xy=xy) for e in engines]
    for ds in sets:
        ds.series_begin(every=1, capacity=nsteps)
    states = [e.state() for e in engines]
    hosts = [ds.host_sampler() for ds in sets]
    want = [[] for _ in parts]
    for _ in range(nsteps):
        group_ti_rk_bcl(engines, states)
        for w, h, st in zip(want, hosts, states):
            w.append(h.sample(st[0], st[1]))
    plans = [ds.plan() for ds in sets]
    got = [ds.series() for ds in sets]
    for e in engines:
        e.close()
    return plans, got, [np.stack(w, axis=2) for w in want]


def check_ranks(parts, case):
    xy, _ = grid_and_stations(case)
    plans, got, want = group_run(parts, xy)
    owned = np.zeros(xy.shape[1], bool)
    for r, p in enumerate(parts):
        elem = plans[r][0]
        assert (elem >= 0).all() and (elem <= S.owned_elements(p)).all()    # never a ghost element
        assert 0 < (elem > 0).sum() < elem.size                             # the rank has part of the grid
        assert np.array_equal(got[r], want[r]), r
        assert not got[r][:, elem == 0].any() and (got[r][3][elem > 0] > 0).all()
        owned |= elem > 0
    assert owned.all()                                          # every point is some rank's


def test_two_face_ranks_in_a_local_group(case_factory):
    from hnumo.facepart import face_partition
    case = case_factory("bump10")
    check_ranks([face_partition(case, 2, r, "block") for r in range(2)], case)


def test_two_rank_ghost_layer_partition(case_factory):
    from hnumo.partition import partition
    case = case_factory("bump10")
    parts = [partition(case, 2, r) for r in range(2)]
    assert all(0 < p.nelem_owned < p.scalars["nelem"] for p in parts)      # the ranks hold ghosts
    check_ranks(parts, case)


def test_two_sets_at_once_and_id_reuse(case_factory):
    from hnumo.engine import Engine
    case, states, _ = stepped_states(case_factory, "bump10", {"nop": 2}, 3)
    xy, ngrid = grid_and_stations(case)
    e = Engine(case)
    q, qb, qp = e.state()
    e.set_resident(True)
    grid = S.DeviceSampler(e, xy=np.asfortranarray(xy[:, :ngrid]))
    stations = S.DeviceSampler(e, xy=np.asfortranarray(xy[:, ngrid:]))
    assert (grid.id, stations.id) == (0, 1)
    hg, hst = grid.host_sampler(), stations.host_sampler()
    grid.series_begin(every=2, capacity=2)
    stations.series_begin(every=1, capacity=3)
    for _ in range(2):
        e.ti_rk_bcl(q, qb, qp)
    assert np.array_equal(grid.series()[:, :, 0], hg.sample(*states[1])) and grid.series().shape[2] == 1
    grid.destroy()
    assert code_of(grid.sample) == 4                            # the id is unknown now
    e.ti_rk_bcl(q, qb, qp)
    ser = stations.series()
    assert ser.shape == (14, 5, 3)
    for i in range(3):
        assert np.array_equal(ser[:, :, i], hst.sample(*states[i])), i
    # the freed id is given out again; eight sets at most
    more = [S.DeviceSampler(e, xy=np.asfortranarray(xy[:, :3])) for _ in range(7)]
    assert [m.id for m in more] == [0, 2, 3, 4, 5, 6, 7]
    assert code_of(lambda: S.DeviceSampler(e, xy=xy)) == 4      # a ninth set
    assert np.array_equal(more[0].sample(), hg.sample(*states[2])[:, :3])
    assert np.array_equal(stations.series(), ser)
    more[3].destroy()
    assert S.DeviceSampler(e, xy=xy).id == 4
    e.close()


def test_error_paths(case_factory):
    from hnumo.engine import Engine, lib
    case, states, _ = stepped_states(case_factory, "bump10", {"nop": 2}, 3)
    L, npoin, ne, ngl = (case.scalars[k] for k in ("nlayers", "npoin", "nelem", "ngl"))
    coord = np.asfortranarray(case.arrays["coord"], dtype=np.float64)
    xgl = S.case_xgl(case)
    xy, _ = grid_and_stations(case)
    M = xy.shape[1]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    P = lambda a: a.ctypes.data_as(dp)
    big = np.zeros(14 * M * 3 + 8)
    n64, sid = C.c_int64(), C.c_int32(-7)
    e = Engine(case)

    def raw(rc):
        assert rc == 4 and lib().hnumo_last_error(e.h).decode().strip()
        assert not big.any() and sid.value == -7                # nothing written

    Lb = lib()
    # creation: NULL pointers, ldc, M, xgl, source, geometry, the caller-supplied form
    raw(Lb.hnumo_sample_create(e.h, None, 3, P(xgl), P(xy), M, 0, C.byref(sid)))
    raw(Lb.hnumo_sample_create(e.h, P(coord), 3, None, P(xy), M, 0, C.byref(sid)))
    raw(Lb.hnumo_sample_create(e.h, P(coord), 3, P(xgl), None, M, 0, C.byref(sid)))
    raw(Lb.hnumo_sample_create(e.h, P(coord), 3, P(xgl), P(xy), M, 0, None))
    raw(Lb.hnumo_sample_create(e.h, P(coord), 4, P(xgl), P(xy), M, 0, C.byref(sid)))
    raw(Lb.hnumo_sample_create(e.h, P(coord), 3, P(xgl), P(xy), 0, 0, C.byref(sid)))
    raw(Lb.hnumo_sample_create(e.h, P(coord), 3, P(xgl), P(xy), -1, 0, C.byref(sid)))
    raw(Lb.hnumo_sample_create(e.h, P(coord), 3, P(xgl), P(xy), M, 2, C.byref(sid)))
    raw(Lb.hnumo_sample_create(e.h, P(coord), 3, P(xgl), P(xy), M, -1, C.byref(sid)))
    raw(Lb.hnumo_sample_create(e.h, P(coord), 3, P(xgl[::-1].copy()), P(xy), M, 0, C.byref(sid)))
    bent = coord.copy(order="F")
    bent[1, ngl + 1] += 1e-3 * (coord[1, ngl * ngl - 1] - coord[1, 0])
    raw(Lb.hnumo_sample_create(e.h, P(bent), 3, P(xgl), P(xy), M, 0, C.byref(sid)))
    el = np.array([1, ne], np.int32)
    xe = np.zeros((2, 2), order="F")
    raw(Lb.hnumo_sample_create_ref(e.h, P(xgl), None, P(xe), 2, 0, C.byref(sid)))
    raw(Lb.hnumo_sample_create_ref(e.h, P(xgl), el.ctypes.data_as(ip), None, 2, 0, C.byref(sid)))
    raw(Lb.hnumo_sample_create_ref(e.h, None, el.ctypes.data_as(ip), P(xe), 2, 0, C.byref(sid)))
    raw(Lb.hnumo_sample_create_ref(e.h, P(xgl), el.ctypes.data_as(ip), P(xe), 0, 0, C.byref(sid)))
    raw(Lb.hnumo_sample_create_ref(e.h, P(xgl), el.ctypes.data_as(ip), P(xe), 2, 5, C.byref(sid)))
    for bad in (np.array([1, ne + 1], np.int32), np.array([-1, 1], np.int32)):
        raw(Lb.hnumo_sample_create_ref(e.h, P(xgl), bad.ctypes.data_as(ip), P(xe), 2, 0, C.byref(sid)))
    for v in (1.0 + 2.0 ** -52, -1.5, np.nan, np.inf):
        x2 = xe.copy(order="F")
        x2[1, 1] = v
        raw(Lb.hnumo_sample_create_ref(e.h, P(xgl), el.ctypes.data_as(ip), P(x2), 2, 0, C.byref(sid)))
    # no set yet: every id is unknown
    for i in (0, 7, 8, -1):
        raw(Lb.hnumo_sample(e.h, i, P(big), 14 * M))
        raw(Lb.hnumo_sample_plan(e.h, i, None, None, M))
        raw(Lb.hnumo_sample_series_begin(e.h, i, 1, 1))
        raw(Lb.hnumo_sample_record(e.h, i))
        raw(Lb.hnumo_sample_series(e.h, i, P(big), big.size, C.byref(n64), 0))
        raw(Lb.hnumo_sample_destroy(e.h, i))
    ds = S.DeviceSampler(e, xy=xy)
    hs = ds.host_sampler()
    i = ds.id
    # a set, but no state on the device yet
    assert code_of(ds.sample) == 4
    ds.series_begin(0, 2)
    assert code_of(ds.record) == 4 and ds.series().shape == (14, M, 0)
    q, qb, qp = e.state()
    e.set_resident(True)
    e.ti_rk_bcl(q, qb, qp)
    # wrong n, wrong M, negative arguments, NULL out
    raw(Lb.hnumo_sample(e.h, i, P(big), 14 * M - 1))
    raw(Lb.hnumo_sample(e.h, i, P(big), 14 * M + 14))
    raw(Lb.hnumo_sample(e.h, i, None, 14 * M))
    raw(Lb.hnumo_sample_plan(e.h, i, None, P(big), M + 1))
    raw(Lb.hnumo_sample_series_begin(e.h, i, -1, 2))
    raw(Lb.hnumo_sample_series_begin(e.h, i, 1, -2))
    ds.record()
    raw(Lb.hnumo_sample_series(e.h, i, P(big), 14 * M - 1, C.byref(n64), 0))   # out too small for one entry
    raw(Lb.hnumo_sample_series(e.h, i, P(big), -1, C.byref(n64), 0))
    assert Lb.hnumo_sample_series(e.h, i, None, 0, C.byref(n64), 1) == 0 and n64.value == 1   # count only; nothing cleared
    want = hs.sample(*states[0])
    assert np.array_equal(ds.series()[:, :, 0], want) and np.array_equal(ds.sample(), want)
    # capacity 0: no series to record into
    ds.series_begin(1, 0)
    assert code_of(ds.record) == 4
    e.ti_rk_bcl(q, qb, qp)                                      # (and every = 1 records nothing)
    assert ds.series().shape == (14, M, 0)
    e.close()
