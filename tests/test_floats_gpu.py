"""Float sets on the device (kernels_float.hip through hnumo_floats_*): positions, velocities,
elements, status and the recorded series equal -- np.array_equal, no tolerance -- the Python mirror
hnumo.floats.HostFloats fed with the per-step states of a second, non-resident engine on the same
case (whose bits equal the resident engine's: tests/test_engine_gpu.py).  The cases carry
tests/states.py's moving state; seeds and conditions are tests/float_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import float_cases as FC
from hnumo import floats as FL
from hnumo import sample as S

pytestmark = pytest.mark.gpu
_runs = {}


def stepped_states(case, key, nsteps):
    """[q_df after step 1..nsteps] and the final (q, qb, qp) from a non-resident engine (once per key)."""
    from hnumo.engine import Engine
    if (key, nsteps) not in _runs:
        e = Engine(case)
        q, qb, qp = e.state()
        out = []
        for _ in range(nsteps):
            e.ti_rk_bcl(q, qb, qp)
            out.append(q.copy(order="F"))
        e.close()
        assert all(np.isfinite(a).all() for a in out)
        _runs[(key, nsteps)] = (out, (q, qb, qp))
    return _runs[(key, nsteps)]


def record_of(g):
    return np.stack([g["x"], g["y"], g["u"], g["v"], g["elem"].astype(np.float64)])


def same(got, hf):
    want = hf.get()
    for k in ("x", "y", "u", "v", "elem", "status"):
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("name,kw", FC.CASES, ids=FC.IDS)
def test_steps_then_large_advances_equal_the_mirror(case_factory, name, kw):
    """2 steps with every = 1, then 4 explicit advances that move the fastest float 0.7 of an
    element: the get-back, the cached locations and the series are the mirror's."""
    from hnumo.engine import Engine
    case = FC.moving(case_factory, name, kw)
    states, _ = stepped_states(case, name, 2)
    xy, layer = FC.seeds(case)
    dt, big = case.scalars["dt"], FC.big_dt(case, states[1])
    hf = FL.HostFloats(case, xy, layer)
    plan = [(states[0], dt), (states[1], dt)] + [(states[1], big)] * 4
    want, stats = FC.run_mirror(hf, plan)
    # bump10's steps set the normal velocity at the wall's own nodes to 0.0 and its fastest flow is
    # over the bump: with 0.7 of an element for the fastest float no seed can reach a wall there (the
    # moving state itself does: tests/test_float_plan.py); the other three cases slide floats along walls
    FC.check_conditions(hf, stats, wall=name != "bump10")
    assert set(layer) == set(range(1, case.scalars["nlayers"] + 1))

    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    df = FL.DeviceFloats(e, xy, layer)
    df.begin(every=1, record_every=1, capacity=6)
    g0 = df.get()
    assert np.array_equal(g0["elem"], stats["elem0"]) and not g0["u"].any()
    for _ in range(2):
        e.ti_rk_bcl(*st)
    for _ in range(4):
        df.advance(dt=big)
    got, ser, (elem, xi, eta) = df.get(), df.series(), df.plan()
    e.close()
    same(got, hf)
    assert np.array_equal(elem, hf.elem) and np.array_equal(xi[elem > 0], hf.xi[elem > 0]) and np.array_equal(eta[elem > 0], hf.eta[elem > 0])
    assert ser.shape == want.shape == (5, hf.M, 6)
    assert np.array_equal(ser, want), int((ser != want).sum())
    assert np.array_equal(ser[:, :, 5], record_of(got))
    assert (got["status"] == FL.ACTIVE).sum() > hf.M // 2 and np.isfinite(ser).all()


def test_sample_set_at_the_cached_locations_reads_the_velocities(case_factory):
    """Without the mirror: a DeviceSampler(elem=, xi_eta=) at the floats' cached locations reads their
    (u, v) in rows 5(k-1)+2, 5(k-1)+3."""
    from hnumo.engine import Engine
    name, kw = FC.CASES[0]
    case = FC.moving(case_factory, name, kw)
    xy, layer = FC.seeds(case)
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    df = FL.DeviceFloats(e, xy, layer)
    df.begin(every=1)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    df.advance(dt=FC.big_dt(case, st[0]))                       # (st holds the initial state: a size, not bits)
    g = df.get()
    elem, xi, eta = df.plan()
    ds = S.DeviceSampler(e, elem=elem, xi_eta=np.stack([xi, eta]))
    v = ds.sample()
    e.close()
    m = np.arange(elem.size)
    on = elem > 0
    assert on.sum() > elem.size // 2 and (g["u"][on] != 0).sum() > on.sum() // 2
    assert np.array_equal(v[5 * (layer - 1) + 1, m], g["u"]) and np.array_equal(v[5 * (layer - 1) + 2, m], g["v"])
    assert np.array_equal(g["status"] == FL.ACTIVE, on)


@pytest.mark.parametrize("M", [1, 257, 703])
def test_tail_wave_and_shuffled_input(case_factory, M):
    """One float; one more than a workgroup; 700 floats in one element (and three elsewhere) in a
    shuffled input order: the output is in input order."""
    from hnumo.engine import Engine
    name, kw = FC.CASES[1]
    case = FC.moving(case_factory, name, kw)
    states, _ = stepped_states(case, name, 2)
    c = FC.corners_of(case)
    rng = np.random.default_rng(M)
    el = np.concatenate([np.full(M - 3, 37), [0, 5, 99]]) if M > 3 else np.array([37])
    rng.shuffle(el)
    xy = np.asfortranarray(np.array([FC.forward(c[k], *rng.uniform(-0.95, 0.95, 2)) for k in el]).T)
    layer = rng.integers(1, 3, M).astype(np.int32)
    big = FC.big_dt(case, states[1])
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    df = FL.DeviceFloats(e, xy, layer)
    hf = df.host_floats()
    assert np.array_equal(df.get()["elem"], el + 1)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    for _ in range(2):
        df.advance(dt=big)
        hf.advance(states[1], big)
    got = df.get()
    e.close()
    same(got, hf)
    assert (got["elem"] != el + 1).any() or M == 1


@pytest.mark.parametrize("which", [0, 1, 3])
def test_row_per_lane_mapping_gives_the_same_bits(case_factory, monkeypatch, which):
    """The lane mapping that was not kept (a float's NGL rows on 4 or 8 adjacent lanes, HNUMO_FLOAT_ROWS=1
    as an experiment knob) computes the mirror's bits too: every sum is still one lane's."""
    from hnumo.engine import Engine
    name, kw = FC.CASES[which]
    case = FC.moving(case_factory, name, kw)
    states, _ = stepped_states(case, name, 2)
    xy, layer = FC.seeds(case)
    big = FC.big_dt(case, states[1])
    monkeypatch.setenv("HNUMO_EXPERIMENTS", "1")
    monkeypatch.setenv("HNUMO_FLOAT_ROWS", "1")
    e = Engine(case)
    assert any("HNUMO_FLOAT_ROWS=1" in o and "ignored" not in o for o in e.overrides)
    st = e.state()
    e.set_resident(True)
    df = FL.DeviceFloats(e, xy, layer)
    hf = df.host_floats()
    df.begin(every=1)
    for i in range(2):
        e.ti_rk_bcl(*st)
        hf.advance(states[i])
    for _ in range(3):
        df.advance(dt=big)
        hf.advance(states[1], big)
    got = df.get()
    e.close()
    same(got, hf)
    assert (got["status"] == FL.ACTIVE).sum() > hf.M // 2


def test_layers_of_one_set_and_two_sets_at_once(case_factory):
    """The same seeds in layers 1, 2, 3 of one set move apart; a second set with its own series runs
    beside it; a freed id is given out again and a ninth set is refused."""
    from hnumo.engine import Engine, EngineError
    name, kw = FC.CASES[0]
    case = FC.moving(case_factory, name, kw)
    states, _ = stepped_states(case, name, 2)
    xy1 = FL.seed_grid(case, 6, 5)
    xy = np.asfortranarray(np.concatenate([xy1] * 3, axis=1))
    layer = np.repeat(np.array([1, 2, 3], np.int32), xy1.shape[1])
    ring = FL.seed_ring(xy1[:, 11], 1.0e5, 16)
    big = FC.big_dt(case, states[1])
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    a, b = FL.DeviceFloats(e, xy, layer), FL.DeviceFloats(e, ring, 2)
    assert (a.id, b.id) == (0, 1)
    ha, hb = a.host_floats(), b.host_floats()
    a.begin(every=1, record_every=2, capacity=2)
    b.begin(every=0, record_every=1, capacity=3)
    for i in range(2):
        e.ti_rk_bcl(*st)
        ha.advance(states[i])
        b.advance(dt=big)
        hb.advance(states[i], big)
        hb.record()
    ha.record()
    ga, gb, sa, sb = a.get(), b.get(), a.series(), b.series()
    same(ga, ha)
    same(gb, hb)
    assert sa.shape == (5, xy.shape[1], 1) and np.array_equal(sa, ha.series())
    assert sb.shape == (5, 16, 2) and np.array_equal(sb, hb.series())
    n = xy1.shape[1]
    assert not np.array_equal(ga["x"][:n], ga["x"][n:2 * n]) and not np.array_equal(ga["x"][n:2 * n], ga["x"][2 * n:])
    a.destroy()
    with pytest.raises(EngineError):
        a.get()
    more = [FL.DeviceFloats(e, ring, 1) for _ in range(7)]
    assert [m.id for m in more] == [0, 2, 3, 4, 5, 6, 7]
    with pytest.raises(EngineError) as ei:
        FL.DeviceFloats(e, ring, 1)
    assert ei.value.code == 4
    e.close()


def test_redone_step_advances_once_and_the_state_is_undisturbed(case_factory, monkeypatch):
    """The corrector's persistent launch of the first step gives up (hnumo_debug_force_abort(1)) and the
    step is redone on per-stage launches: the floats are those of an engine on per-stage launches from
    the start, and both runs end on the state bits of a run with no set."""
    from hnumo.engine import Engine
    name, kw = FC.CASES[0]
    case = FC.moving(case_factory, name, kw)
    states, final = stepped_states(case, name, 3)
    xy, layer = FC.seeds(case)
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
        df = FL.DeviceFloats(eng, xy, layer)
        df.begin(every=1, record_every=1, capacity=4)
        for _ in range(3):
            eng.ti_rk_bcl(*st)
        out.append((df.series(), df.get()))
        eng.sync(*st)
        for x, y in zip(st, final):
            assert np.array_equal(x, y)
    assert e.persistent_stats["aborts"] == 1
    e.close()
    e0.close()
    hf = FL.HostFloats(case, xy, layer)
    for q in states:
        hf.advance(q)
        hf.record()
    for ser, g in out:
        assert ser.shape == (5, hf.M, 3) and np.array_equal(ser, hf.series())
        same(g, hf)
    assert not np.array_equal(out[0][0][:, :, 0], out[0][0][:, :, 1])


def check_ranks(parts, case):
    """While a float is ACTIVE on a rank its record equals the single-rank run's bits (elements mapped
    through the partition; floats seeded in the same element on both); an inactive float never changes again; a float whose single-rank
    locations all stay inside one rank's owned elements is ACTIVE there to the end."""
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    nsteps, nbig = 2, 2                                        # steps with every = 1, then explicit large advances
    nrec = nsteps + nbig
    xy, layer = FC.seeds(case, max_edge_elems=24)
    states, _ = stepped_states(case, ("ranks", id(case)), nsteps)
    big = FC.big_dt(case, states[-1])
    # the single-rank run, on the device, and the mirror's account of where each float went
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    one = FL.DeviceFloats(e, xy, layer)
    one.begin(every=1, record_every=1, capacity=nrec)
    for _ in range(nsteps):
        e.ti_rk_bcl(*st)
    for _ in range(nbig):
        one.advance(dt=big)
    ref, ref_status = one.series(), one.get()["status"]
    e.close()
    hf = FL.HostFloats(case, xy, layer)
    seeded, elem0 = hf.elem > 0, hf.elem.copy()
    for q, dt in [(q, None) for q in states] + [(states[-1], big)] * nbig:
        hf.advance(q, dt)
        hf.record()
    assert np.array_equal(hf.series(), ref)

    engines = [Engine(p) for p in parts]
    local_group(engines)
    sets = [FL.DeviceFloats(g, xy, layer) for g in engines]
    for s in sets:
        s.begin(every=1, record_every=1, capacity=nrec)
    sts = [g.state() for g in engines]
    first = [s.get() for s in sets]
    plans = [s.plan() for s in sets]
    for _ in range(nsteps):
        group_ti_rk_bcl(engines, sts)
    for _ in range(nbig):
        for s in sets:
            s.advance(dt=big)
    got = [(s.series(), s.get()) for s in sets]
    for g in engines:
        g.close()
    somewhere = np.zeros(hf.M, bool)
    for r, p in enumerate(parts):
        ser, g = got[r]
        ne = S.owned_elements(p)
        glob = np.concatenate([[0], np.asarray(p.elems[:ne]) + 1]).astype(np.float64)   # local 1-based -> global 1-based
        active = np.concatenate([(first[r]["status"] == FL.ACTIVE)[:, None], ser[4] > 0], axis=1)   # (M, nrec + 1)
        assert 0 < active[:, 0].sum() < hf.M                    # the rank has part of the seeds
        # a seed on an edge the rank shares with another rank lies in the lower element of the two on one
        # rank alone; here it lies in the rank's own: another float of the discontinuous field from the start
        el0, xi0, eta0 = plans[r]
        other = active[:, 0] & (glob[el0] != elem0)
        assert other.sum() < 0.05 * hf.M and (np.maximum(np.abs(xi0[other]), np.abs(eta0[other])) == 1.0).all()
        assert (ser[4] <= ne).all()
        for i in range(nrec):
            on = active[:, i + 1]
            assert active[on, i].all()                          # no float comes back
            mapped = ser[:, :, i].copy()
            mapped[4] = glob[ser[4, :, i].astype(np.int64)]
            assert np.array_equal(mapped[:, on & ~other], ref[:, on & ~other, i]), (r, i)
            off = ~active[:, i]
            if i > 0:
                assert np.array_equal(ser[:, off, i], ser[:, off, i - 1])   # inactive: never touched again
        owned = set((np.asarray(p.elems[:ne]) + 1).tolist())
        stay = np.array([bool(v) and v <= owned for v in hf.visited]) & (ref_status == FL.ACTIVE) & ~other
        assert stay.any() and (g["status"][stay] == FL.ACTIVE).all()
        assert ((g["status"] == FL.LEFT) & active[:, 0]).any() and not (g["status"] == FL.LOST).any()
        somewhere |= active[:, 0]
    assert np.array_equal(somewhere, seeded)


def test_two_face_ranks_in_a_local_group(case_factory):
    from hnumo.facepart import face_partition
    case = FC.moving(case_factory, *FC.CASES[1])
    check_ranks([face_partition(case, 2, r, "block") for r in range(2)], case)


def test_group_step_runs_every_observer_after_a_refused_recording(case_factory):
    """Two ranks in a local group, each with flow statistics (every = 1, a series of one sample) and a
    float set (every = 1).  The second group step is refused by the full statistics series (code 4: the
    step itself succeeded), and the floats of both ranks have advanced on it all the same: they are
    those of two steps with a series that is large enough."""
    from hnumo.engine import Engine, EngineError, group_ti_rk_bcl, local_group
    from hnumo.facepart import face_partition
    case = FC.moving(case_factory, *FC.CASES[1])
    parts = [face_partition(case, 2, r, "block") for r in range(2)]
    xy, layer = FC.seeds(case, max_edge_elems=24)

    def two_steps(capacity):
        engines = [Engine(p) for p in parts]
        local_group(engines)
        sets = [FL.DeviceFloats(g, xy, layer) for g in engines]
        for g, s in zip(engines, sets):
            g.stats_begin(every=1, series=capacity)
            s.begin(every=1)
        sts = [g.state() for g in engines]
        group_ti_rk_bcl(engines, sts)
        if capacity >= 2:
            group_ti_rk_bcl(engines, sts)
        else:
            with pytest.raises(EngineError) as ei:
                group_ti_rk_bcl(engines, sts)
            assert ei.value.code == 4 and "flow statistics after the step" in str(ei.value)
        got = [s.get() for s in sets]
        for g in engines:
            g.close()
        return got

    want, got = two_steps(2), two_steps(1)
    for r in range(2):
        assert (want[r]["status"] == FL.ACTIVE).any() and want[r]["u"].any()
        for k in ("x", "y", "u", "v", "elem", "status"):
            assert np.array_equal(got[r][k], want[r][k]), (r, k, int((got[r][k] != want[r][k]).sum()))


def test_two_rank_ghost_layer_partition(case_factory):
    from hnumo.partition import partition
    case = FC.moving(case_factory, *FC.CASES[1])
    parts = [partition(case, 2, r) for r in range(2)]
    assert all(0 < p.nelem_owned < p.scalars["nelem"] for p in parts)      # the ranks hold ghosts
    check_ranks(parts, case)


def test_error_paths_and_reseeding(case_factory):
    from hnumo.engine import Engine, EngineError, lib
    name, kw = FC.CASES[1]
    case = FC.moving(case_factory, name, kw)
    states, _ = stepped_states(case, name, 2)
    coord = np.asfortranarray(case.arrays["coord"], dtype=np.float64)
    xgl = S.case_xgl(case)
    ngl = case.scalars["ngl"]
    xy = FL.seed_grid(case, 7, 5)
    M = xy.shape[1]
    layer = np.ones(M, np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    P = lambda a: a.ctypes.data_as(dp)
    I = lambda a: a.ctypes.data_as(ip)
    big = np.zeros(5 * M * 2 + 8)
    ibuf = np.zeros(M, np.int32)
    n64, fid = C.c_int64(), C.c_int32(-7)
    e = Engine(case)
    Lb = lib()

    def raw(rc):
        assert rc == 4 and Lb.hnumo_last_error(e.h).decode().strip()
        assert not big.any() and not ibuf.any() and fid.value == -7            # nothing written

    # creation: NULL pointers, ldc, M, xgl, layers, geometry
    raw(Lb.hnumo_floats_create(e.h, None, 3, P(xgl), P(xy), I(layer), M, C.byref(fid)))
    raw(Lb.hnumo_floats_create(e.h, P(coord), 3, None, P(xy), I(layer), M, C.byref(fid)))
    raw(Lb.hnumo_floats_create(e.h, P(coord), 3, P(xgl), None, I(layer), M, C.byref(fid)))
    raw(Lb.hnumo_floats_create(e.h, P(coord), 3, P(xgl), P(xy), None, M, C.byref(fid)))
    raw(Lb.hnumo_floats_create(e.h, P(coord), 3, P(xgl), P(xy), I(layer), M, None))
    raw(Lb.hnumo_floats_create(e.h, P(coord), 4, P(xgl), P(xy), I(layer), M, C.byref(fid)))
    raw(Lb.hnumo_floats_create(e.h, P(coord), 3, P(xgl), P(xy), I(layer), 0, C.byref(fid)))
    raw(Lb.hnumo_floats_create(e.h, P(coord), 3, P(xgl), P(xy), I(layer), -1, C.byref(fid)))
    raw(Lb.hnumo_floats_create(e.h, P(coord), 3, P(xgl[::-1].copy()), P(xy), I(layer), M, C.byref(fid)))
    for bad in (0, 3, -1):
        l2 = layer.copy()
        l2[M // 2] = bad
        raw(Lb.hnumo_floats_create(e.h, P(coord), 3, P(xgl), P(xy), I(l2), M, C.byref(fid)))
    bent = coord.copy(order="F")
    bent[1, ngl + 1] += 1e-3 * (coord[1, ngl * ngl - 1] - coord[1, 0])
    raw(Lb.hnumo_floats_create(e.h, P(bent), 3, P(xgl), P(xy), I(layer), M, C.byref(fid)))
    nan = coord.copy(order="F")
    nan[0, 5] = np.nan
    raw(Lb.hnumo_floats_create(e.h, P(nan), 3, P(xgl), P(xy), I(layer), M, C.byref(fid)))
    # no set yet: every id is unknown
    for i in (0, 7, 8, -1):
        raw(Lb.hnumo_floats_get(e.h, i, P(big), None, None, None, I(ibuf), None, M))
        raw(Lb.hnumo_floats_plan(e.h, i, I(ibuf), P(big), M))
        raw(Lb.hnumo_floats_set(e.h, i, P(xy), I(layer), M))
        raw(Lb.hnumo_floats_advance(e.h, i, 1.0))
        raw(Lb.hnumo_floats_begin(e.h, i, 1, 1, 1))
        raw(Lb.hnumo_floats_record(e.h, i))
        raw(Lb.hnumo_floats_series(e.h, i, P(big), big.size, C.byref(n64), 0))
        raw(Lb.hnumo_floats_destroy(e.h, i))
    df = FL.DeviceFloats(e, xy, layer)
    i = df.id
    # a set, but no state on the device yet
    raw(Lb.hnumo_floats_advance(e.h, i, 1.0))
    st = e.state()
    e.set_resident(True)
    e.ti_rk_bcl(*st)
    # wrong M, every other than 0 or 1, negative arguments, a dt that is not finite, no series
    raw(Lb.hnumo_floats_get(e.h, i, P(big), None, None, None, I(ibuf), None, M + 1))
    raw(Lb.hnumo_floats_plan(e.h, i, I(ibuf), P(big), M - 1))
    raw(Lb.hnumo_floats_set(e.h, i, P(xy), I(layer), M - 1))
    l2 = layer.copy()
    l2[0] = 3
    raw(Lb.hnumo_floats_set(e.h, i, P(xy), I(l2), M))
    raw(Lb.hnumo_floats_set(e.h, i, None, I(layer), M))
    for ev in (2, -1, 5):
        raw(Lb.hnumo_floats_begin(e.h, i, ev, 1, 1))
    raw(Lb.hnumo_floats_begin(e.h, i, 1, -1, 1))
    raw(Lb.hnumo_floats_begin(e.h, i, 1, 1, -1))
    raw(Lb.hnumo_floats_advance(e.h, i, float("nan")))
    raw(Lb.hnumo_floats_advance(e.h, i, float("inf")))
    raw(Lb.hnumo_floats_record(e.h, i))                                     # no series
    df.begin(every=1, record_every=1, capacity=1)
    e.ti_rk_bcl(*st)
    with pytest.raises(EngineError) as ei:                                  # the series is full: step and advance are done
        e.ti_rk_bcl(*st)
    assert ei.value.code == 4
    raw(Lb.hnumo_floats_series(e.h, i, P(big), 5 * M - 1, C.byref(n64), 0))
    raw(Lb.hnumo_floats_series(e.h, i, P(big), -1, C.byref(n64), 0))
    assert Lb.hnumo_floats_series(e.h, i, None, 0, C.byref(n64), 1) == 0 and n64.value == 1
    hf = df.host_floats()
    hf.advance(states[1])
    hf.record()
    assert np.array_equal(df.series(clear=True), hf.series()) and df.series().shape == (5, M, 0)
    e.close()
    hf2 = FL.HostFloats(case, xy, layer)
    # (the engine above took a third step; its floats advanced on it: a fresh engine for the re-seed)
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    a = FL.DeviceFloats(e, xy, layer)
    a.begin(every=1)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    xy2 = np.asfortranarray(xy[:, ::-1] * (1 + 1e-3))
    a.set(xy2, 2)
    b = FL.DeviceFloats(e, xy2, 2)
    big_dt = FC.big_dt(case, states[1])
    a.advance(dt=big_dt)
    b.advance(dt=big_dt)
    ga, gb = a.get(), b.get()
    e.close()
    hf2.set(xy2, 2)
    hf2.advance(states[1], big_dt)
    same(ga, hf2)
    same(gb, hf2)
