"""Vorticity products on the device (kernels_vort.hip through hnumo_vort_*, and the sample sets' VORT
source): fields and series equal -- np.array_equal, no tolerance -- the numpy mirror
hnumo.vorticity.HostVorticity fed with the per-step states of a second, non-resident engine on the
same moving case (whose bits equal the resident engine's: tests/test_engine_gpu.py).  The resident
engine is read before any sync."""
import ctypes as C

import numpy as np
import pytest

import states
from hnumo import sample as S
from hnumo import vorticity as V

pytestmark = pytest.mark.gpu
_moving, _runs = {}, {}

# dg25L3 5x3: P = 25, the last element group (10 per group) ragged, L = 3; bump10 at N=2: P = 9, 28
# elements per group, L = 2; qmbump8: warped quadrilaterals, the metric rows differ between elements;
# dg25N7L3 3x3: P = 64, 4 elements per group
CASES = [("dg25L3", {"nelx": 5, "nely": 3}), ("bump10", {"nop": 2}), ("qmbump8", {}), ("dg25N7L3", {"nelx": 3, "nely": 3})]


def moving(case_factory, name, kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _moving:
        _moving[key] = states.moving_case(case_factory(name, **kw))
    return _moving[key]


def stepped_states(case_factory, name, kw, nsteps=2):
    """(case, [q_df after step 1..nsteps], final (q, qb, qp)) from a non-resident engine (once per case)."""
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


def mirror_series(case, qs, coriolis=True):
    hv = V.HostVorticity(case, coriolis=coriolis)
    for q in qs:
        hv.add(q)
    return hv.series


def resident_recorded(case, nsteps):
    """nsteps resident steps with an explicit record after each; (fields, series) read BEFORE any sync."""
    from hnumo.engine import Engine
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    dv = V.DeviceVorticity(e, every=0, series=nsteps)
    for _ in range(nsteps):
        e.ti_rk_bcl(*st)
        dv.add()
    got = dv.fields(), dv.series
    e.close()
    return got


def assert_fields_and_series(case, qs, got, what=""):
    fields, series = got
    want = V.HostVorticity(case).fields(qs[-1])
    assert np.isfinite(fields).all() and np.abs(fields[0]).max() > 0, what
    assert np.array_equal(fields, want), (what, "fields", float(np.abs(fields - want).max()))
    ms = mirror_series(case, qs)
    assert series.shape == ms.shape, (what, series.shape, ms.shape)
    assert np.array_equal(series, ms), (what, "series", series, ms)


@pytest.mark.parametrize("name,kw", CASES)
def test_fields_and_series_equal_mirror(case_factory, name, kw):
    case, qs, _ = stepped_states(case_factory, name, kw)
    if name == "qmbump8":
        P = case.scalars["ngl"] ** 2
        for k in ("ksi_x", "ksi_y", "eta_x", "eta_y"):
            m = np.asarray(case.arrays[k]).reshape(P, -1, order="F")
            assert np.ptp(m[0]) > 0.01 * np.abs(m[0]).max(), k      # the metric rows differ between elements
    assert_fields_and_series(case, qs, resident_recorded(case, 2), name)


def test_more_elements_than_one_reduction_chunk(case_factory):
    """E = 37*37 = 1369 elements: two chunks of the tree kernel, the second one ragged (345)."""
    case, qs, _ = stepped_states(case_factory, "dg25L3", {"nelx": 37, "nely": 37, "nop": 2})
    assert case.scalars["nelem"] == 1369
    assert_fields_and_series(case, qs, resident_recorded(case, 2), "dg25L3 37x37")


def test_coriolis_given_against_null(case_factory):
    """On the beta plane pv differs with f given, zeta, delta and ow do not."""
    from hnumo.engine import Engine
    case, qs, _ = stepped_states(case_factory, *CASES[0])
    assert case.cfg["beta"] != 0 and np.ptp(V.coriolis_of(case)) > 0
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    out = {}
    for cor in (True, False):
        dv = V.DeviceVorticity(e, every=0, series=1, coriolis=cor)
        dv.add()
        out[cor] = dv.fields(), dv.series
        assert np.array_equal(out[cor][0], V.HostVorticity(case, coriolis=cor).fields(qs[1])), cor
        assert np.array_equal(out[cor][1], mirror_series(case, qs[1:], coriolis=cor)), cor
    e.close()
    (fa, sa), (fb, sb) = out[True], out[False]
    for c in (0, 1, 3):
        assert np.array_equal(fa[c], fb[c])
    assert (fa[2] != fb[2]).all()
    assert np.array_equal(sa[[0, 2]], sb[[0, 2]]) and (sa[1] != sb[1]).all()


def test_every_second_step_equals_explicit_records(case_factory):
    """every=2 over 4 steps = explicit records after steps 2 and 4; both runs end on the bits of a run
    that never began."""
    from hnumo.engine import Engine
    case, qs, final = stepped_states(case_factory, "bump10", {"nop": 2}, 4)
    want = mirror_series(case, [qs[1], qs[3]])
    for mode in ("every", "explicit"):
        e = Engine(case)
        q, qb, qp = e.state()
        e.set_resident(True)
        e.vort_begin(V.coriolis_of(case), every=2 if mode == "every" else 0, series=4)
        for s in range(4):
            e.ti_rk_bcl(q, qb, qp)
            if mode == "explicit" and s % 2 == 1:
                e.vort_record()
        ser = e.vort_series()
        e.sync(q, qb, qp)
        e.close()
        assert ser.shape == want.shape == (3, 2, 2) and np.array_equal(ser, want), mode
        for a, b in zip((q, qb, qp), final):
            assert np.array_equal(a, b), mode


def test_redone_step_is_sampled_once(case_factory, monkeypatch):
    """The corrector's persistent launch of the first step gives up (hnumo_debug_force_abort(1)) and the
    step is redone on per-stage launches: 3 steps give 3 samples, those of an engine on per-stage
    launches from the start."""
    from hnumo.engine import Engine
    case = moving(case_factory, *CASES[0])
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
        dv = V.DeviceVorticity(eng, every=1, series=4)
        for _ in range(3):
            eng.ti_rk_bcl(*st)
        out.append(dv.series)
    assert e.persistent_stats["aborts"] == 1
    e.close()
    e0.close()
    assert out[0].shape == (3, 3, 3) and np.array_equal(out[0], out[1])
    assert not np.array_equal(out[0][:, :, 0], out[0][:, :, 1])


def test_non_resident_engine_samples_its_last_output(case_factory):
    from hnumo.engine import Engine
    case = moving(case_factory, "bump10", {"nop": 2})
    e = Engine(case)
    q, qb, qp = e.state()
    dv = V.DeviceVorticity(e, every=1, series=3)
    hv = V.HostVorticity(case)
    for _ in range(2):
        e.ti_rk_bcl(q, qb, qp)
        hv.add(q)
    dv.add()                                  # the output of the last call, once more
    hv.add(q)
    got = dv.fields(), dv.series
    e.close()
    assert np.array_equal(got[0], hv.fields(q)) and np.array_equal(got[1], hv.series)
    assert got[1].shape == (3, 2, 3) and np.abs(got[0][0]).max() > 0


def group_run(parts, nsteps):
    """The ranks `parts` as a local exchange group, every=1: per rank (fields, series) of the engine
    and of the mirror on that rank's own states."""
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    engines = [Engine(p) for p in parts]
    local_group(engines)
    dvs = [V.DeviceVorticity(e, every=1, series=nsteps) for e in engines]
    sts = [e.state() for e in engines]
    hosts = [V.HostVorticity(p) for p in parts]
    for _ in range(nsteps):
        group_ti_rk_bcl(engines, sts)
        for h, st in zip(hosts, sts):
            h.add(st[0])
    devs = [(d.fields(), d.series) for d in dvs]
    for e in engines:
        e.close()
    return devs, [(h.fields(st[0]), h.series) for h, st in zip(hosts, sts)]


@pytest.mark.parametrize("kind", ["face", "ghost"])
def test_two_ranks_in_a_local_group(case_factory, kind):
    case = moving(case_factory, "dg25L3", {"nelx": 4, "nely": 2})
    if kind == "face":
        from hnumo.facepart import face_partition
        parts = [face_partition(case, 2, r, "block") for r in range(2)]
    else:
        from hnumo.partition import partition
        parts = [partition(case, 2, r) for r in range(2)]
    devs, hosts = group_run(parts, 2)
    for r, p in enumerate(parts):
        (df, ds), (hf, hs) = devs[r], hosts[r]
        assert np.array_equal(df, hf) and np.array_equal(ds, hs), (kind, r)
        assert ds.shape == (3, 3, 2) and np.abs(df[0]).max() > 0 and np.isfinite(df).all()
        nown = p.nelem_owned * p.scalars["ngl"] ** 2
        if kind == "ghost":
            assert nown < p.scalars["npoin"] and not df[:, nown:].any()      # ghost nodes read 0


def node_points(case):
    ngl, ne = case.scalars["ngl"], S.owned_elements(case)
    P = ngl * ngl
    xgl = S.case_xgl(case)
    e = np.repeat(np.arange(ne), P)
    ln = np.tile(np.arange(P), ne)
    return (e + 1).astype(np.int32), np.stack([xgl[ln % ngl], xgl[ln // ngl]])


@pytest.mark.parametrize("name,kw", CASES)
def test_vort_sample_set(case_factory, name, kw):
    """At the nodes the set equals hnumo_vort_fields; at off-node points (two in one element, one with
    elem = 0, every element once in reverse order: more elements than arena slots at N=7) it equals
    HostSampler on the mirror's fields; an every=1 series has one entry per step with their bits."""
    from hnumo.engine import Engine
    case, qs, _ = stepped_states(case_factory, name, kw)
    L, npoin, ne = case.scalars["nlayers"], case.scalars["npoin"], case.scalars["nelem"]
    rng = np.random.default_rng(11)
    elem = np.concatenate([[3, 3, 0], np.arange(ne, 0, -1)]).astype(np.int32)
    xe = rng.uniform(-1, 1, (2, elem.size))
    hs = S.HostSampler(case, elem, xe[0], xe[1], source=S.VORT)
    hv = V.HostVorticity(case)
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    dv = V.DeviceVorticity(e)
    ds = S.DeviceSampler(e, elem=elem, xi_eta=xe, source=S.VORT)
    ds.series_begin(every=1, capacity=2)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    nelem, nxe = node_points(case)
    dn = S.DeviceSampler(e, elem=nelem, xi_eta=nxe, source=S.VORT)
    at_nodes, fields, off, ser = dn.sample(), dv.fields(), ds.sample(), ds.series()
    e.close()
    assert at_nodes.shape == (4 * L, npoin)
    for k in range(L):
        assert np.array_equal(at_nodes[4 * k:4 * k + 4], fields[:, :, k]), (name, k)
    want = [hs.sample_vort(hv.fields(q)) for q in qs]
    assert np.array_equal(off, want[1]), (name, float(np.abs(off - want[1]).max()))
    assert not off[:, 2].any() and np.abs(off[0]).max() > 0 and np.isfinite(off).all()
    assert ser.shape == (4 * L, elem.size, 2)
    assert np.array_equal(ser[:, :, 0], want[0]) and np.array_equal(ser[:, :, 1], want[1])


# ---------------------------------------------------------------- the code-4 paths
def refused(e, fn, *a, has=""):
    """fn(*a) raises code 4 with a message that names `has`."""
    from hnumo.engine import EngineError
    with pytest.raises(EngineError) as ei:
        fn(*a)
    msg = str(ei.value).split("): ", 1)[1].strip()
    assert ei.value.code == 4 and msg and has in msg, msg
    return msg


@pytest.fixture
def small(case_factory):
    from hnumo.engine import Engine
    e = Engine(moving(case_factory, "bump10", {"nop": 2}))
    yield e
    e.close()


def test_code4_before_begin(small):
    e = small
    from hnumo.engine import lib
    assert lib().hnumo_vort_end(e.h) == 0                       # a no-op
    for fn in (e.vort_record, e.vort_fields, e.vort_series):
        refused(e, fn, has="hnumo_vort_begin")


def test_code4_negative_arguments(small):
    refused(small, small.vort_begin, None, -1, 0, has="must be >= 0")
    refused(small, small.vort_begin, None, 0, -1, has="must be >= 0")


def test_code4_before_any_state(small):
    small.vort_begin(None, 0, 2)
    refused(small, small.vort_record, has="no state on the device")
    refused(small, small.vort_fields, has="no state on the device")
    assert small.vort_series().shape == (3, 2, 0)


def test_code4_wrong_n(small):
    from hnumo.engine import lib
    e = small
    L, npoin = e.dims["nlayers"], e.dims["npoin"]
    q, qb, qp = e.state()
    e.vort_begin(None, 0, 2)
    e.ti_rk_bcl(q, qb, qp)
    e.vort_record()
    big = np.zeros(4 * npoin * (L + 1) + 8)
    ptr = big.ctypes.data_as(C.POINTER(C.c_double))
    n64 = C.c_int64()
    for rc in (lib().hnumo_vort_fields(e.h, ptr, 4 * npoin * L - 1), lib().hnumo_vort_fields(e.h, ptr, 4 * npoin * (L + 1)),
               lib().hnumo_vort_series(e.h, ptr, 3 * L - 1, C.byref(n64), 0), lib().hnumo_vort_series(e.h, ptr, -1, C.byref(n64), 0)):
        assert rc == 4 and not big.any()                        # nothing written
        assert "n" in lib().hnumo_last_error(e.h).decode() and "hnumo_vort_" in lib().hnumo_last_error(e.h).decode()
    assert lib().hnumo_vort_series(e.h, None, 0, C.byref(n64), 0) == 0 and n64.value == 1      # (NULL, 0): the count


def test_code4_series_full_or_absent(small, case_factory):
    e = small
    case = e.case
    q, qb, qp = e.state()
    e.set_resident(True)
    e.vort_begin(V.coriolis_of(case), 0, 0)
    e.ti_rk_bcl(q, qb, qp)
    refused(e, e.vort_record, has="no series")
    assert np.abs(e.vort_fields()[0]).max() > 0                 # the fields need no series
    e.vort_begin(V.coriolis_of(case), 1, 1)                     # a second begin resets
    assert e.vort_series().shape[2] == 0
    e.ti_rk_bcl(q, qb, qp)
    refused(e, e.vort_record, has="full")
    # the every hook on a full series: the step call returns 4 with the step done
    refused(e, e.ti_rk_bcl, q, qb, qp, has="the step itself succeeded")
    qs = stepped_states(case_factory, "bump10", {"nop": 2}, 4)[1]
    ser = e.vort_series(clear=True)
    assert np.array_equal(ser, mirror_series(case, [qs[1]])) and e.vort_series().shape[2] == 0
    e.vort_record()                                             # room again: the state after step 3
    assert np.array_equal(e.vort_series(), mirror_series(case, [qs[2]]))
    e.vort_end()
    refused(e, e.vort_series, has="hnumo_vort_begin")


def test_code4_vort_sample_set_before_begin(small):
    e = small
    q, qb, qp = e.state()
    e.ti_rk_bcl(q, qb, qp)
    xgl = S.case_xgl(e.case)
    # before hnumo_vort_begin the set cannot be created (it needs f) ...
    refused(e, e.sample_create_ref, xgl, [1, 2], np.zeros((2, 2)), S.VORT, has="hnumo_vort_begin")
    refused(e, e.sample_create, e.case.arrays["coord"], xgl, np.full((2, 1), 1000.0), S.VORT, has="hnumo_vort_begin")
    e.vort_begin(None, 0, 0)
    sid = e.sample_create_ref(xgl, [1, 2], np.zeros((2, 2)), S.VORT)
    assert e.sample(sid).shape == (8, 2)
    e.sample_series_begin(sid, every=0, capacity=1)
    e.vort_end()
    # ... and after hnumo_vort_end it cannot be sampled
    refused(e, e.sample, sid, has="hnumo_vort_begin")
    refused(e, e.sample_record, sid, has="hnumo_vort_begin")
    assert e.sample_series(sid).shape == (8, 2, 0)


def test_overrides_short_buffer_leaves_a_message(case_factory, monkeypatch):
    from hnumo.engine import Engine, lib
    monkeypatch.setenv("HNUMO_PERSISTENT", "0")
    e = Engine(case_factory("bump10", nop=2))
    monkeypatch.delenv("HNUMO_PERSISTENT")
    text = "HNUMO_PERSISTENT=0"
    assert e.overrides == [text]
    refused(e, e.vort_record, has="hnumo_vort_begin")            # a message of another call, to be replaced
    buf = C.create_string_buffer(8)
    assert lib().hnumo_overrides(e.h, buf, len(buf)) == 4
    msg = lib().hnumo_last_error(e.h).decode()
    assert "hnumo_overrides" in msg and str(len(text) + 1) in msg, msg
    assert buf.value.decode() == text[:7]
    e.close()
