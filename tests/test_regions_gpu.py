"""Region sets on the device (kernels_region.hip through hnumo_regions_*): series and areas equal --
np.array_equal, no tolerance -- the numpy mirror hnumo.regions.HostRegions fed with the per-step states of a
second, non-resident engine on the same moving case (whose bits equal the resident engine's:
tests/test_engine_gpu.py), after 2 steps.  The resident engine is read before any sync.

Shapes: the smallest at which the member groups of the 256-lane workgroup (EPB = 256 // P members, a ragged
last group, members that are not consecutive elements) and the segmented tree can go wrong:

    bump10 nop=4 4x4          P = 25, L = 2: three uneven regions (3, 5, 6 members) plus unlabelled elements
    lake10 nop=2 4x4 L=1      P = 9,  one layer, 28 members per group
    dg25N7L3 3x3              P = 64, L = 3: 4 members per group, the padded product rows
    qmbump8 nop=5 4x4         P = 36, warped quadrilaterals: the metric rows differ between elements
    dg25L3 nop=2 37x37        1369 elements, regions of 1100, 268, 1 and 0: two tree passes for the first (its
                              second chunk ragged, 76), one for the others, a zero write for the last
"""
import ctypes as C

import numpy as np
import pytest

import states
from hnumo import covariance as CV
from hnumo import regions as RG
from hnumo import sample as S
from hnumo import vorticity as V

pytestmark = pytest.mark.gpu
_moving, _runs = {}, {}

SHAPES = [("bump10", {"nop": 4, "nelx": 4, "nely": 4}), ("lake10", {"nop": 2, "nelx": 4, "nely": 4, "nlayers": 1}),
          ("dg25N7L3", {"nelx": 3, "nely": 3}), ("qmbump8", {"nop": 5, "nelx": 4, "nely": 4})]
STATE = {"qmbump8": dict(amp=0.005, fr=0.001, jump=0.005)}
SMALL = SHAPES[0]
BETA = ("dg25L3", {"nelx": 4, "nely": 4})
BIG = ("dg25L3", {"nelx": 37, "nely": 37, "nop": 2})
BOTH = RG.FLOW | RG.VORT


def moving(case_factory, name, kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _moving:
        _moving[key] = states.moving_case(case_factory(name, **kw), **STATE.get(name, {}))
    return _moving[key]


def stepped_states(case_factory, name, kw, nsteps=2):
    """(case, [q_df after step 1..nsteps], final (q, qb, qp)) from a non-resident engine that never created a
    region set (once per case)."""
    from hnumo.engine import Engine
    key = (name, tuple(sorted(kw.items())), nsteps)
    if key not in _runs:
        case = moving(case_factory, name, kw)
        e = Engine(case)
        q, qb, qp = e.state()
        out = []
        for _ in range(nsteps):
            e.ti_rk_bcl(q, qb, qp)
            out.append(q.copy(order="F"))
        e.close()
        assert all(np.isfinite(x).all() for x in out)
        _runs[key] = (case, out, (q, qb, qp))
    return _runs[key]


def uneven(ne):
    """three uneven regions whose members are scattered over the elements, plus unlabelled elements"""
    e = np.arange(ne)
    lab = np.where(e % 7 == 3, 0, np.where(e % 5 < 1, 1, np.where(e % 5 < 3, 2, 3))).astype(np.int32)
    return lab, 3


def mirror(case, lab, R, rows, qs, coriolis=None):
    hr = RG.HostRegions(case, lab, R, rows, coriolis=coriolis)
    for q in qs:
        hr.add(q)
    return hr


def resident_run(case, sets, nsteps=2):
    """nsteps resident steps with an explicit sample of every set after each; [(series, area)] read BEFORE any
    sync.  sets: [(labels, R, rows, coriolis)]"""
    from hnumo.engine import Engine
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    drs = [RG.DeviceRegions(e, lab, R, rows, coriolis=cor, every=0, series=nsteps) for lab, R, rows, cor in sets]
    for _ in range(nsteps):
        e.ti_rk_bcl(*st)
        for d in drs:
            d.add()
    got = [(d.series, d.area) for d in drs]
    e.close()
    return got


def assert_equal_mirror(got, hr, what=""):
    ser, area = got
    want = hr.series
    assert ser.shape == want.shape and np.isfinite(ser).all(), (what, ser.shape, want.shape)
    names = RG.row_names(hr.L, hr.mask)
    for v in range(hr.V):
        assert np.array_equal(ser[v], want[v]), (what, names[v], ser[v], want[v])
    assert np.array_equal(area, hr.area), (what, area, hr.area)


@pytest.mark.parametrize("rows", [RG.FLOW, RG.VORT, BOTH])
@pytest.mark.parametrize("name,kw", SHAPES)
def test_series_and_area_equal_mirror(case_factory, name, kw, rows):
    case, qs, _ = stepped_states(case_factory, name, kw)
    lab, R = uneven(case.scalars["nelem"])
    sizes = [int((lab == r).sum()) for r in range(R + 1)]
    assert min(sizes) > 0 and len(set(sizes[1:])) > 1, sizes        # uneven, with unlabelled elements
    if (name, kw) == SMALL:
        assert sorted(sizes[1:]) == [3, 5, 6] and sizes[0] == 2
    if name == "qmbump8":
        P = case.scalars["ngl"] ** 2
        m = np.asarray(case.arrays["ksi_x"]).reshape(P, -1, order="F")
        assert np.ptp(m[0]) > 0.01 * np.abs(m[0]).max()               # the metric rows differ between elements
    got = resident_run(case, [(lab, R, rows, None)])[0]
    hr = mirror(case, lab, R, rows, qs)
    assert_equal_mirror(got, hr, name)
    assert got[0].shape == (RG.region_rows(case.scalars["nlayers"], rows), R, 2) and (got[1] > 0).all()
    assert np.abs(got[0]).max() > 0 and not np.array_equal(got[0][:, :, 0], got[0][:, :, 1])


def test_two_tree_passes_with_a_ragged_chunk_and_an_empty_region(case_factory):
    """1369 elements at N=2: regions of 1100 (chunks of 1024 and 76, then a pass over the two results), 268, 1
    and 0 members."""
    case, qs, _ = stepped_states(case_factory, *BIG)
    ne = case.scalars["nelem"]
    assert ne == 1369
    lab = np.zeros(ne, np.int32)
    order = np.random.default_rng(5).permutation(ne)
    lab[order[:1100]], lab[order[1100:1368]], lab[order[1368:]] = 1, 2, 3
    R = 4
    assert [int((lab == r).sum()) for r in (1, 2, 3, 4)] == [1100, 268, 1, 0]
    got = resident_run(case, [(lab, R, BOTH, True)])[0]
    assert_equal_mirror(got, mirror(case, lab, R, BOTH, qs, coriolis=True), "37x37")
    ser, area = got
    assert not ser[:, 3].any() and not np.signbit(ser[:, 3]).any() and area[3] == 0 and not np.signbit(area[3])
    assert (np.abs(ser[:, :3]) > 0).all()


def test_coriolis_given_against_null(case_factory):
    """On the beta plane PZ differs with f given; Z and G do not."""
    case, qs, _ = stepped_states(case_factory, *BETA)
    assert case.cfg["beta"] != 0 and np.ptp(V.coriolis_of(case)) > 0
    lab, R = uneven(case.scalars["nelem"])
    (sa, _), (sb, _) = resident_run(case, [(lab, R, RG.VORT, True), (lab, R, RG.VORT, None)])
    assert np.array_equal(sa, mirror(case, lab, R, RG.VORT, qs, coriolis=True).series)
    assert np.array_equal(sb, mirror(case, lab, R, RG.VORT, qs, coriolis=None).series)
    assert np.array_equal(sa[0::3], sb[0::3]) and np.array_equal(sa[2::3], sb[2::3]) and (sa[1::3] != sb[1::3]).all()


@pytest.mark.parametrize("name,kw", [SMALL, BIG])
def test_one_region_of_all_elements_has_the_bits_of_the_whole_domain_series(case_factory, name, kw):
    """The anchor that does not go through the mirror: hnumo_stats_series and hnumo_vort_series of the same run."""
    from hnumo.engine import Engine
    case = moving(case_factory, name, kw)
    L, ne = case.scalars["nlayers"], case.scalars["nelem"]
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    e.stats_begin(1, 2)
    e.vort_begin(V.coriolis_of(case), 1, 2)
    dr = RG.DeviceRegions(e, np.ones(ne, np.int32), 1, BOTH, coriolis=True, every=1, series=2)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    ser, ss, vs = dr.series, e.stats_series(), e.vort_series()
    e.close()
    assert ser.shape == (7 * L, 1, 2) and ss.shape == (2, L, 2) and vs.shape == (3, L, 2)
    for k in range(L):
        assert np.array_equal(ser[4 * k + 3, 0], ss[0, k]) and np.array_equal(ser[4 * k, 0], ss[1, k]), k
        for c in range(3):
            assert np.array_equal(ser[4 * L + 3 * k + c, 0], vs[c, k]), (k, c)
    assert (ss > 0).all() and np.abs(vs).min() > 0


# ---------------------------------------------------------------- the observer contract
def test_every_second_step_equals_explicit_samples_and_the_step_is_unchanged(case_factory):
    from hnumo.engine import Engine
    case, qs, final = stepped_states(case_factory, *SMALL, 4)
    lab, R = uneven(case.scalars["nelem"])
    want = mirror(case, lab, R, BOTH, [qs[1], qs[3]]).series
    for mode in ("every", "explicit"):
        e = Engine(case)
        q, qb, qp = e.state()
        e.set_resident(True)
        sid = e.regions_create(lab, R, BOTH, None, 2 if mode == "every" else 0, 4)
        for s in range(4):
            e.ti_rk_bcl(q, qb, qp)
            if mode == "explicit" and s % 2 == 1:
                e.regions_sample(sid)
        ser = e.regions_series(sid)
        e.sync(q, qb, qp)
        e.close()
        assert ser.shape == want.shape and np.array_equal(ser, want), mode
        for a, b in zip((q, qb, qp), final):                          # the bits of an engine without region sets
            assert np.array_equal(a, b), mode


def test_redone_step_is_sampled_once(case_factory, monkeypatch):
    """The corrector's persistent launch of the first step gives up (hnumo_debug_force_abort(1)) and the step is
    redone on per-stage launches: 3 steps give 3 samples, those of an engine on per-stage launches from the
    start."""
    from hnumo.engine import Engine
    case = moving(case_factory, *BETA)
    lab, R = uneven(case.scalars["nelem"])
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
        dr = RG.DeviceRegions(eng, lab, R, BOTH, coriolis=True, every=1, series=4)
        for _ in range(3):
            eng.ti_rk_bcl(*st)
        out.append(dr.series)
    assert e.persistent_stats["aborts"] == 1
    e.close()
    e0.close()
    assert out[0].shape[2] == 3 and np.array_equal(out[0], out[1])
    assert not np.array_equal(out[0][:, :, 0], out[0][:, :, 1])


def test_non_resident_engine_samples_its_last_output(case_factory):
    from hnumo.engine import Engine
    case = moving(case_factory, *SMALL)
    lab, R = uneven(case.scalars["nelem"])
    e = Engine(case)
    q, qb, qp = e.state()
    dr = RG.DeviceRegions(e, lab, R, BOTH, every=1, series=3)
    hr = RG.HostRegions(case, lab, R, BOTH)
    for _ in range(2):
        e.ti_rk_bcl(q, qb, qp)
        hr.add(q)
    dr.add()                                                           # the output of the last call, once more
    hr.add(q)
    got = dr.series, dr.area
    e.close()
    assert_equal_mirror(got, hr, "non-resident")
    assert got[0].shape[2] == 3


def test_two_processor_face_ranks_each_against_its_own_mirror(case_factory):
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    from hnumo.facepart import face_partition
    case = moving(case_factory, "dg25L3", {"nelx": 4, "nely": 2})
    parts = [face_partition(case, 2, r, "block") for r in range(2)]
    engines = [Engine(p) for p in parts]
    local_group(engines)
    labs = [uneven(p.nelem_owned) for p in parts]
    drs = [RG.DeviceRegions(e, lab, R, BOTH, coriolis=True, every=1, series=2) for e, (lab, R) in zip(engines, labs)]
    hosts = [RG.HostRegions(p, lab, R, BOTH, coriolis=True) for p, (lab, R) in zip(parts, labs)]
    sts = [e.state() for e in engines]
    for _ in range(2):
        group_ti_rk_bcl(engines, sts)
        for h, st in zip(hosts, sts):
            h.add(st[0])
    devs = [(d.series, d.area) for d in drs]
    for e in engines:
        e.close()
    for r in range(2):
        assert 0 < parts[r].nelem_owned < case.scalars["nelem"]
        assert_equal_mirror(devs[r], hosts[r], f"rank {r}")
        assert np.abs(devs[r][0]).max() > 0


def test_four_sets_at_once_with_the_other_observers_on(case_factory):
    """Four overlapping partitions beside the statistics, the vorticity, the covariances, the energy budget and a
    sample set, all on every = 1: every set has its mirror's bits, and the others' series are those of a run
    without region sets."""
    from hnumo.engine import Engine
    case, qs, final = stepped_states(case_factory, *BETA)
    ne, L = case.scalars["nelem"], case.scalars["nlayers"]
    cfg = case.cfg
    lab_u, R_u = uneven(ne)
    lab_s, R_s = RG.strips(case, 1, np.linspace(cfg["ydims"][0], cfg["ydims"][1], 5))
    xm = cfg["xdims"][0] + 0.25 * (cfg["xdims"][1] - cfg["xdims"][0])
    lab_b, R_b = RG.boxes(case, [(cfg["xdims"][0], xm, cfg["ydims"][0], 2 * cfg["ydims"][1]),
                                 (xm, 2 * cfg["xdims"][1], cfg["ydims"][0], 2 * cfg["ydims"][1])])
    assert [int((lab_s == r).sum()) for r in range(1, 5)] == [4, 4, 4, 4] and int((lab_b == 1).sum()) == 4
    sets = [(lab_u, R_u, BOTH, True), (lab_s, R_s, RG.FLOW, None), (lab_b, R_b, RG.VORT, None), (np.ones(ne, np.int32), 1, BOTH, True)]
    zref = CV.rest_elevations(case_factory(*BETA[:1], **BETA[1]))
    xgl = S.case_xgl(case)
    series = {}
    for with_regions in (True, False):
        e = Engine(case)
        q, qb, qp = e.state()
        e.set_resident(True)
        e.stats_begin(1, 2)
        e.vort_begin(V.coriolis_of(case), 1, 2)
        e.cov_begin(V.coriolis_of(case), zref, 1)
        e.energy_begin(zref, 1, 2)
        sid = e.sample_create_ref(xgl, [1, ne], np.zeros((2, 2)), S.STATE)
        e.sample_series_begin(sid, 1, 2)
        drs = [RG.DeviceRegions(e, lab, R, rows, coriolis=cor, every=1, series=2) for lab, R, rows, cor in sets] if with_regions else []
        for _ in range(2):
            e.ti_rk_bcl(q, qb, qp)
        got = [(d.series, d.area) for d in drs]
        series[with_regions] = (e.stats_series(), e.vort_series(), e.energy_series(), e.sample_series(sid), e.cov_sums()[0])
        if with_regions:
            from hnumo.engine import EngineError
            with pytest.raises(EngineError) as ei:                     # a fifth set
                e.regions_create(lab_u, R_u, RG.FLOW, None, 0, 1)
            assert ei.value.code == 4 and "hnumo_regions_create" in str(ei.value) and "4 region sets already" in str(ei.value)
            drs[1].end()                                               # destroy frees a slot; the others stay
            sid5 = e.regions_create(lab_u, R_u, RG.FLOW, None, 0, 1)
            assert sid5 == drs[1].id
            e.regions_sample(sid5)
            assert np.array_equal(e.regions_series(sid5)[:, :, 0], mirror(case, lab_u, R_u, RG.FLOW, [qs[1]]).series[:, :, 0])
            assert np.array_equal(drs[0].series, got[0][0])
        e.sync(q, qb, qp)
        e.close()
        for a, b in zip((q, qb, qp), final):
            assert np.array_equal(a, b), with_regions
        if with_regions:
            for g, (lab, R, rows, cor) in zip(got, sets):
                assert_equal_mirror(g, mirror(case, lab, R, rows, qs, coriolis=cor), f"set R={R} rows={rows}")
    for a, b in zip(series[True], series[False]):
        assert np.array_equal(a, b) and np.abs(a).max() > 0


# ---------------------------------------------------------------- the code-4 paths
def refused(fn, *a, has=()):
    """fn(*a) raises code 4 with a message that holds every text of `has`."""
    from hnumo.engine import EngineError
    with pytest.raises(EngineError) as ei:
        fn(*a)
    msg = str(ei.value).split("): ", 1)[1].strip()
    assert ei.value.code == 4 and msg, msg
    for h in (has,) if isinstance(has, str) else has:
        assert h in msg, (h, msg)
    return msg


@pytest.fixture
def small(case_factory):
    from hnumo.engine import Engine
    e = Engine(moving(case_factory, *SMALL))
    yield e
    e.close()


def raw(e, call, *a):
    """(return code, message) of a call on the library itself"""
    from hnumo.engine import lib
    rc = getattr(lib(), call)(e.h, *a)
    return rc, lib().hnumo_last_error(e.h).decode()


def test_code4_unknown_id(small):
    e = small
    n64 = C.c_int64()
    buf = np.zeros(4)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    for call, a in (("hnumo_regions_sample", (0,)), ("hnumo_regions_series", (2, None, 0, C.byref(n64), 0)),
                    ("hnumo_regions_area", (3, p, 4)), ("hnumo_regions_destroy", (-1,)), ("hnumo_regions_sample", (4,))):
        rc, msg = raw(e, call, *a)
        assert rc == 4 and msg == f"{call}: no region set with id {a[0]}", msg
    assert not buf.any()


def test_code4_create_arguments(small):
    e = small
    ne = e.dims["nelem"]
    lab, R = uneven(ne)
    refused(e.regions_create, lab, R, RG.FLOW, None, -1, 0, has=("hnumo_regions_create", "must be >= 0, got -1, 0"))
    refused(e.regions_create, lab, R, RG.FLOW, None, 0, -2, has=("hnumo_regions_create", "must be >= 0, got 0, -2"))
    refused(e.regions_create, lab[:-1], R, RG.FLOW, None, 0, 1, has=("hnumo_regions_create", f"n must be nelem_owned = {ne}, got {ne - 1}"))
    refused(e.regions_create, lab, 0, RG.FLOW, None, 0, 1, has=("hnumo_regions_create", "nregions must be >= 1, got 0"))
    refused(e.regions_create, lab, R, 0, None, 0, 1, has=("hnumo_regions_create", "rows_mask", "got 0"))
    refused(e.regions_create, lab, R, 4, None, 0, 1, has=("hnumo_regions_create", "rows_mask", "got 4"))
    refused(e.regions_create, lab, 2, RG.FLOW, None, 0, 1, has=("hnumo_regions_create", "= 3 is outside 0..2"))
    from hnumo.engine import lib
    sid = C.c_int32(-7)
    assert lib().hnumo_regions_create(e.h, None, ne, R, 1, None, 0, 1, C.byref(sid)) == 4 and sid.value == -7
    assert "region_of_elem is NULL" in lib().hnumo_last_error(e.h).decode()
    assert lib().hnumo_regions_create(e.h, lab.ctypes.data_as(C.POINTER(C.c_int32)), ne, R, 1, None, 0, 1, None) == 4
    assert "id is NULL" in lib().hnumo_last_error(e.h).decode()
    # nothing was created
    rc, msg = raw(e, "hnumo_regions_sample", 0)
    assert rc == 4 and "no region set with id 0" in msg


def test_code4_before_any_state_and_without_a_series(small):
    e = small
    lab, R = uneven(e.dims["nelem"])
    sid = e.regions_create(lab, R, RG.FLOW, None, 0, 2)
    refused(e.regions_sample, sid, has=("hnumo_regions_sample", "no state on the device"))
    assert e.regions_series(sid).shape == (4 * e.dims["nlayers"], R, 0)
    assert np.array_equal(e.regions_area(sid), RG.HostRegions(e.case, lab, R).area)     # the areas need no state
    q, qb, qp = e.state()
    e.ti_rk_bcl(q, qb, qp)
    none = e.regions_create(lab, R, RG.FLOW, None, 1, 0)             # capacity 0: nothing to record into
    e.ti_rk_bcl(q, qb, qp)                                           # ... so nothing is due after a step either
    refused(e.regions_sample, none, has=("hnumo_regions_sample", f"region set {none} has no series"))
    refused(e.regions_series, none, has=("hnumo_regions_series", f"region set {none} has no series"))


def test_code4_wrong_n_and_a_full_series(small, case_factory):
    e = small
    case = e.case
    L = e.dims["nlayers"]
    lab, R = uneven(e.dims["nelem"])
    q, qb, qp = e.state()
    e.set_resident(True)
    sid = e.regions_create(lab, R, BOTH, None, 1, 1)
    e.ti_rk_bcl(q, qb, qp)
    V_ = 7 * L
    big = np.zeros(V_ * R * 2 + 8)
    p = big.ctypes.data_as(C.POINTER(C.c_double))
    n64 = C.c_int64()
    for call, a, text in (("hnumo_regions_series", (sid, p, V_ * R - 1, C.byref(n64), 0), f"n = {V_ * R - 1}"),
                          ("hnumo_regions_series", (sid, p, -1, C.byref(n64), 0), "n = -1"),
                          ("hnumo_regions_area", (sid, p, R + 1), f"nregions = {R}, got {R + 1}"),
                          ("hnumo_regions_area", (sid, None, R), "out is NULL")):
        rc, msg = raw(e, call, *a)
        assert rc == 4 and msg.startswith(call + ": ") and text in msg and not big.any(), msg
    rc, _ = raw(e, "hnumo_regions_series", sid, None, 0, C.byref(n64), 0)
    assert rc == 0 and n64.value == 1                                # (NULL, 0): the count
    refused(e.regions_sample, sid, has=("hnumo_regions_sample", f"the series of region set {sid} is full (1 samples)"))
    # the every hook on a full series: the step call returns 4 with the step done
    refused(e.ti_rk_bcl, q, qb, qp, has="the step itself succeeded")
    qs = stepped_states(case_factory, *SMALL, 4)[1]
    ser = e.regions_series(sid, clear=True)
    assert np.array_equal(ser, mirror(case, lab, R, BOTH, [qs[0]]).series) and e.regions_series(sid).shape[2] == 0
    e.regions_sample(sid)                                            # room again: the state after step 2
    assert np.array_equal(e.regions_series(sid), mirror(case, lab, R, BOTH, [qs[1]]).series)
    e.regions_destroy(sid)
    rc, msg = raw(e, "hnumo_regions_series", sid, None, 0, C.byref(n64), 0)
    assert rc == 4 and "no region set with id" in msg
