"""Eddy covariances on the device (kernels_cov.hip through hnumo_cov_*, and the sample sets' COV source):
sums, fields and integrals equal -- np.array_equal, no tolerance -- the numpy mirror
hnumo.covariance.HostEddyCov fed with the per-step states of a second, non-resident engine on the same
moving case (whose bits equal the resident engine's: tests/test_engine_gpu.py), after at least 3 samples.
The resident engine is read before any sync.  Shapes: the smallest at which the element groups of the
256-lane workgroup (whole elements, a ragged last group), the banking cases of the LDS tiles and the
pairwise tree can go wrong."""
import ctypes as C

import numpy as np
import pytest

import states
from hnumo import covariance as CV
from hnumo import flowstats as F
from hnumo import floats as FL
from hnumo import sample as S
from hnumo import vorticity as V

pytestmark = pytest.mark.gpu
_moving, _runs = {}, {}

# N=2 on 6x6: P = 9, 28 elements per group and a ragged 8, L = 2; N=3 on 4x4: P = 16, one full group;
# N=4 on 4x4: P = 25, 10 per group and a ragged 6, L = 3; N=5 on 3x3: P = 36, 7 per group and a ragged 2
# (ngl = 6: the column read of a half straddles two elements); N=7 on 3x3: P = 64, groups of 4, 4, 1;
# qmbump8: warped quadrilaterals, all four metric terms non-zero and different between elements
SHAPES = [("bump10", {"nop": 2, "nelx": 6, "nely": 6}), ("bump10", {"nop": 3, "nelx": 4, "nely": 4}),
          ("dg25L3", {"nelx": 4, "nely": 4}), ("dg25L3", {"nop": 5, "nelx": 3, "nely": 3}),
          ("dg25N7L3", {"nelx": 3, "nely": 3}), ("qmbump8", {})]
SMALL2 = SHAPES[0]            # L = 2
# the warped grid keeps its thicknesses positive over these steps with tests/states.py's amplitudes halved
STATE = {"qmbump8": dict(amp=0.005, fr=0.001, jump=0.005)}
SMALL3 = SHAPES[2]            # L = 3, on the beta plane


def moving(case_factory, name, kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _moving:
        rest = case_factory(name, **kw)
        _moving[key] = (states.moving_case(rest, **STATE.get(name, {})), CV.rest_elevations(rest))
    return _moving[key]


def stepped_states(case_factory, name, kw, nsteps=3):
    """(case, zref, [q_df after step 1..nsteps], final (q, qb, qp)) from a non-resident engine that never
    began covariances (once per case)."""
    from hnumo.engine import Engine
    key = (name, tuple(sorted(kw.items())), nsteps)
    if key not in _runs:
        case, zref = moving(case_factory, name, kw)
        e = Engine(case)
        q, qb, qp = e.state()
        out = []
        for _ in range(nsteps):
            e.ti_rk_bcl(q, qb, qp)
            out.append(q.copy(order="F"))
        e.close()
        assert all(np.isfinite(x).all() for x in out)
        _runs[key] = (case, zref, out, (q, qb, qp))
    return _runs[key]


def mirror(case, qs, **kw):
    cv = CV.HostEddyCov(case, **kw)
    for q in qs:
        cv.add(q)
    return cv


def read(dc):
    """(sums, nsamples, fields, integrals) of a device object"""
    s, n = dc.sums()
    return s, n, dc.fields(), dc.integrals()


def assert_equal_mirror(got, hc, what=""):
    s, n, f, ig = got
    hs, hn = hc.sums()
    assert n == hn, (what, n, hn)
    assert np.isfinite(s).all() and np.isfinite(f).all() and np.isfinite(ig).all(), what
    for c, name in enumerate(CV.SUM_NAMES):
        assert np.array_equal(s[c], hs[c]), (what, "sums", name, float(np.abs(s[c] - hs[c]).max()))
    hf = hc.fields()
    for c, name in enumerate(CV.FIELD_NAMES):
        assert np.array_equal(f[c], hf[c]), (what, "fields", name, float(np.abs(f[c] - hf[c]).max()))
    hi = hc.integrals()
    assert ig.shape == hi.shape and np.array_equal(ig, hi), (what, "integrals", ig, hi)


def resident_run(case, nsteps, **kw):
    """nsteps resident steps with an explicit sample after each; everything read BEFORE any sync."""
    from hnumo.engine import Engine
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    dc = CV.DeviceEddyCov(e, every=0, **kw)
    for _ in range(nsteps):
        e.ti_rk_bcl(*st)
        dc.add()
    got = read(dc)
    e.close()
    return got


@pytest.mark.parametrize("name,kw", SHAPES)
def test_sums_fields_and_integrals_equal_mirror(case_factory, name, kw):
    case, zref, qs, _ = stepped_states(case_factory, name, kw)
    if name == "qmbump8":
        P = case.scalars["ngl"] ** 2
        for k in ("ksi_x", "ksi_y", "eta_x", "eta_y"):
            m = np.asarray(case.arrays[k]).reshape(P, -1, order="F")
            # (non-zero at all but a few nodes, and different between elements)
            assert np.count_nonzero(m) > 0.9 * m.size and np.ptp(m[0]) > 0.01 * np.abs(m[0]).max(), k
    got = resident_run(case, 3, zref=zref)
    assert_equal_mirror(got, mirror(case, qs, zref=zref), name)
    f = got[2]
    assert np.abs(f[5]).max() > 0 and np.abs(f[6]).max() > 0 and np.abs(f[13]).max() > 0 and np.abs(f[11]).max() > 0, name


@pytest.mark.parametrize("cor,ref", [(True, False), (False, True), (False, False)])
def test_coriolis_and_zref_given_or_null(case_factory, cor, ref):
    """(both given: the test above.)  On the beta plane f changes the PV sums and nothing else; zref
    changes S_d, S_dd and nothing else."""
    case, zref, qs, _ = stepped_states(case_factory, *SMALL3)
    assert case.cfg["beta"] != 0 and np.ptp(V.coriolis_of(case)) > 0
    kw = {"coriolis": cor, "zref": zref if ref else None}
    got = resident_run(case, 3, **kw)
    assert_equal_mirror(got, mirror(case, qs, **kw), str(kw))
    full = mirror(case, qs, zref=zref).sums()[0]
    same = [c for c in range(14) if np.array_equal(got[0][c], full[c])]
    assert same == [c for c in range(14) if not ((not cor and c >= 10) or (not ref and c in (8, 9)))]


def test_more_elements_than_one_reduction_chunk(case_factory):
    """E = 37*37 = 1369 elements at N=2: two chunks of the tree kernel, the second one ragged (345)."""
    case, zref, qs, _ = stepped_states(case_factory, "dg25L3", {"nelx": 37, "nely": 37, "nop": 2})
    assert case.scalars["nelem"] == 1369
    assert_equal_mirror(resident_run(case, 3, zref=zref), mirror(case, qs, zref=zref), "dg25L3 37x37")


def test_non_resident_engine_samples_its_last_output(case_factory):
    from hnumo.engine import Engine
    case, zref = moving(case_factory, *SMALL2)
    e = Engine(case)
    q, qb, qp = e.state()
    dc = CV.DeviceEddyCov(e, every=1, zref=zref)
    hc = CV.HostEddyCov(case, zref=zref)
    for _ in range(3):
        e.ti_rk_bcl(q, qb, qp)
        hc.add(q)
    dc.add()                                  # the output of the last call, once more
    hc.add(q)
    got = read(dc)
    e.close()
    assert got[1] == 4
    assert_equal_mirror(got, hc, "non-resident")


@pytest.mark.parametrize("kind", ["face", "ghost"])
def test_two_ranks_in_a_local_group(case_factory, kind):
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    case, _ = moving(case_factory, "dg25L3", {"nelx": 4, "nely": 2})
    if kind == "face":
        from hnumo.facepart import face_partition
        parts = [face_partition(case, 2, r, "block") for r in range(2)]
    else:
        from hnumo.partition import partition
        parts = [partition(case, 2, r) for r in range(2)]
    engines = [Engine(p) for p in parts]
    local_group(engines)
    dcs = [CV.DeviceEddyCov(e, every=1) for e in engines]
    sts = [e.state() for e in engines]
    hosts = [CV.HostEddyCov(p) for p in parts]
    for _ in range(3):
        group_ti_rk_bcl(engines, sts)
        for h, st in zip(hosts, sts):
            h.add(st[0])
    devs = [read(d) for d in dcs]
    for e in engines:
        e.close()
    for r, p in enumerate(parts):
        assert_equal_mirror(devs[r], hosts[r], (kind, r))
        nown = p.nelem_owned * p.scalars["ngl"] ** 2 if kind == "ghost" else p.scalars["npoin"]
        assert np.abs(devs[r][2][5, :nown]).max() > 0
        if kind == "ghost":
            assert nown < p.scalars["npoin"]
            assert not devs[r][0][:, nown:].any() and not devs[r][2][:, nown:].any()      # ghost nodes read 0


def test_every_second_step_leaves_the_step_alone(case_factory):
    """every=2 over 6 steps: 3 samples, those of steps 2, 4, 6; q, qb, qprime end on the bits of a run that
    never began covariances."""
    from hnumo.engine import Engine
    case, zref, qs, final = stepped_states(case_factory, *SMALL2, 6)
    e = Engine(case)
    q, qb, qp = e.state()
    e.set_resident(True)
    dc = CV.DeviceEddyCov(e, every=2, zref=zref)
    for _ in range(6):
        e.ti_rk_bcl(q, qb, qp)
    got = read(dc)
    e.sync(q, qb, qp)
    e.close()
    assert got[1] == 3
    assert_equal_mirror(got, mirror(case, [qs[1], qs[3], qs[5]], zref=zref), "every=2")
    for a, b in zip((q, qb, qp), final):
        assert np.array_equal(a, b)


def test_saved_sums_restored_after_end_continue_on_the_same_bits(case_factory):
    from hnumo.engine import Engine
    case, zref, qs, _ = stepped_states(case_factory, *SMALL3, 4)
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    dc = CV.DeviceEddyCov(e, every=1, zref=zref)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    saved, n = dc.sums()
    dc.end()
    dc = CV.DeviceEddyCov(e, every=1, zref=zref)        # a second begin: from zero
    assert dc.nsamples == 0 and not dc.sums()[0].any()
    dc.set_sums(saved, n)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    got = read(dc)
    e.close()
    assert n == 2 and got[1] == 4
    assert_equal_mirror(got, mirror(case, qs, zref=zref), "restored")


def node_points(case):
    ngl, ne = case.scalars["ngl"], S.owned_elements(case)
    P = ngl * ngl
    xgl = S.case_xgl(case)
    e = np.repeat(np.arange(ne), P)
    ln = np.tile(np.arange(P), ne)
    return (e + 1).astype(np.int32), np.stack([xgl[ln % ngl], xgl[ln // ngl]])


@pytest.mark.parametrize("name,kw", [SHAPES[0], SHAPES[3], SHAPES[4]])
def test_cov_sample_set(case_factory, name, kw):
    """At the nodes the set equals hnumo_cov_fields exactly; at off-node points (two in one element, one
    with elem = 0, every element once in reverse order: more elements than arena slots) it equals
    HostSampler fed the mirror's fields; an every=1 series sees the sums of its own step."""
    from hnumo.engine import Engine
    case, zref, qs, _ = stepped_states(case_factory, name, kw)
    L, npoin, ne = case.scalars["nlayers"], case.scalars["npoin"], case.scalars["nelem"]
    rng = np.random.default_rng(17)
    elem = np.concatenate([[3, 3, 0], np.arange(ne, 0, -1)]).astype(np.int32)
    xe = rng.uniform(-1, 1, (2, elem.size))
    hs = S.HostSampler(case, elem, xe[0], xe[1], source="cov")
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    dc = CV.DeviceEddyCov(e, every=1, zref=zref)
    ds = S.DeviceSampler(e, elem=elem, xi_eta=xe, source="cov")
    ds.series_begin(every=1, capacity=3)
    for _ in range(3):
        e.ti_rk_bcl(*st)
    nelem, nxe = node_points(case)
    dn = S.DeviceSampler(e, elem=nelem, xi_eta=nxe, source=S.COV)
    at_nodes, fields, off, ser = dn.sample(), dc.fields(), ds.sample(), ds.series()
    e.close()
    assert at_nodes.shape == (16 * L, npoin)
    for k in range(L):
        assert np.array_equal(at_nodes[16 * k:16 * k + 16], fields[:, :, k]), (name, k)
    want = [hs.sample_cov(mirror(case, qs[:i + 1], zref=zref).fields()) for i in range(3)]
    assert np.array_equal(off, want[2]), (name, float(np.abs(off - want[2]).max()))
    assert not off[:, 2].any() and np.abs(off[5]).max() > 0 and np.isfinite(off).all()
    assert ser.shape == (16 * L, elem.size, 3)
    for i in range(3):
        assert np.array_equal(ser[:, :, i], want[i]), (name, i)


def test_other_observers_record_what_they_record_without_covariances(case_factory):
    """Statistics, vorticity, a STATE sample set and a float set beside the covariances: each of them
    records the bits it records on an engine that never began covariances."""
    from hnumo.engine import Engine
    case, zref, qs, final = stepped_states(case_factory, *SMALL2)
    xy = FL.seed_grid(case, 3, 2)
    out = {}
    for with_cov in (False, True):
        e = Engine(case)
        q, qb, qp = e.state()
        e.set_resident(True)
        e.stats_begin(1, 3)
        e.vort_begin(V.coriolis_of(case), 1, 3)
        dc = CV.DeviceEddyCov(e, every=1, zref=zref) if with_cov else None
        ds = S.DeviceSampler(e, xy=xy)
        ds.series_begin(every=1, capacity=3)
        df = FL.DeviceFloats(e, xy, 1)
        df.begin(every=1, record_every=1, capacity=3)
        for _ in range(3):
            e.ti_rk_bcl(q, qb, qp)
        out[with_cov] = (e.stats_sums()[0], e.stats_series(), e.vort_series(), e.vort_fields(), ds.series(), df.series())
        if with_cov:
            cov = read(dc)
        e.sync(q, qb, qp)
        e.close()
        for a, b in zip((q, qb, qp), final):
            assert np.array_equal(a, b), with_cov
    for a, b in zip(out[False], out[True]):
        assert a.shape == b.shape
        assert a.any() and np.array_equal(a, b)
    assert_equal_mirror(cov, mirror(case, qs, zref=zref), "all observers on")
    # the statistics on the same samples: hbar, um, vm are the same statements
    st = F.HostFlowStats(case, series=False)
    for x in qs:
        st.add(x)
    assert np.array_equal(out[True][0], st.sums)
    for c, d in ((0, 0), (3, 1), (4, 2)):
        assert np.array_equal(cov[2][c], st.fields()[d])


# ---------------------------------------------------------------- the code-4 paths
def refused(fn, *a, has=""):
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
    e = Engine(moving(case_factory, *SMALL2)[0])
    yield e
    e.close()


def test_code4_before_begin(small):
    from hnumo.engine import lib
    e = small
    assert lib().hnumo_cov_end(e.h) == 0                        # a no-op
    for fn in (e.cov_accumulate, e.cov_sums, e.cov_fields, e.cov_integrals):
        assert refused(fn, has="hnumo_cov_begin").startswith("hnumo_cov_")
    refused(e.cov_set_sums, np.zeros((14, e.dims["npoin"], e.dims["nlayers"]), order="F"), 1, has="call hnumo_cov_begin first")


def test_code4_negative_every(small):
    assert refused(small.cov_begin, None, None, -1, has="every must be >= 0, got -1").startswith("hnumo_cov_begin")


def test_code4_before_any_state_and_no_samples(small):
    e = small
    e.cov_begin(None, None, 0)
    refused(e.cov_accumulate, has="hnumo_cov_accumulate: no state on the device yet")
    refused(e.cov_fields, has="hnumo_cov_fields: no samples yet")
    refused(e.cov_integrals, has="hnumo_cov_integrals: no samples yet")
    s, n = e.cov_sums()
    assert n == 0 and not s.any()
    e.ti_rk_bcl(*e.state())
    refused(e.cov_fields, has="no samples yet")                  # a state, still no sample
    e.cov_accumulate()
    assert e.cov_sums()[1] == 1 and np.isfinite(e.cov_fields()).all()
    e.cov_begin(None, None, 0)                                   # a second begin resets
    assert e.cov_sums()[1] == 0
    refused(e.cov_integrals, has="no samples yet")
    refused(e.cov_set_sums, s, -1, has="nsamples must be >= 0")


def test_code4_wrong_n(small):
    from hnumo.engine import lib
    e = small
    L, npoin = e.dims["nlayers"], e.dims["npoin"]
    q, qb, qp = e.state()
    e.cov_begin(None, None, 1)
    e.ti_rk_bcl(q, qb, qp)
    big = np.zeros(16 * npoin * (L + 1) + 8)
    ptr = big.ctypes.data_as(C.POINTER(C.c_double))
    n64 = C.c_int64(-7)
    Lb = lib()
    calls = ((lambda: Lb.hnumo_cov_sums(e.h, ptr, 14 * npoin * L - 1, C.byref(n64)), "hnumo_cov_sums: n must be 14*npoin*nlayers"),
             (lambda: Lb.hnumo_cov_sums(e.h, ptr, 16 * npoin * L, C.byref(n64)), "hnumo_cov_sums: n must be 14*npoin*nlayers"),
             (lambda: Lb.hnumo_cov_set_sums(e.h, ptr, 14 * npoin * L + 1, 1), "hnumo_cov_set_sums: n must be 14*npoin*nlayers"),
             (lambda: Lb.hnumo_cov_fields(e.h, ptr, 14 * npoin * L), "hnumo_cov_fields: n must be 16*npoin*nlayers"),
             (lambda: Lb.hnumo_cov_fields(e.h, ptr, -1), "hnumo_cov_fields: n must be 16*npoin*nlayers"),
             (lambda: Lb.hnumo_cov_integrals(e.h, ptr, 3 * L + 1), "hnumo_cov_integrals: n must be 3*nlayers"),
             (lambda: Lb.hnumo_cov_integrals(e.h, ptr, 0), "hnumo_cov_integrals: n must be 3*nlayers"))
    for call, who in calls:
        assert call() == 4 and not big.any() and n64.value == -7    # nothing written
        assert who in Lb.hnumo_last_error(e.h).decode(), Lb.hnumo_last_error(e.h).decode()
    assert e.cov_sums()[1] == 1                                  # the sample the step took is still there


def test_code4_unsupported_layers_or_ngl(case_factory):
    """Every ngl an engine can be created with (3, 4, 5, 6, 8) has its kernels, so the refusal is reached
    through the layer count: one layer has no instantiation."""
    from hnumo.engine import Engine
    e = Engine(case_factory("lake10", nop=2, nelx=4, nely=4, nlayers=1))
    assert e.dims["nlayers"] == 1
    refused(e.cov_begin, None, None, 0, has="hnumo_cov_begin: unsupported nlayers or ngl")
    refused(e.cov_accumulate, has="hnumo_cov_begin")
    e.close()


def test_code4_cov_sample_set_before_begin_or_without_samples(small):
    e = small
    q, qb, qp = e.state()
    e.ti_rk_bcl(q, qb, qp)
    xgl = S.case_xgl(e.case)
    # before hnumo_cov_begin the set cannot be created ...
    refused(e.sample_create_ref, xgl, [1, 2], np.zeros((2, 2)), S.COV, has="hnumo_cov_begin")
    refused(e.sample_create, e.case.arrays["coord"], xgl, np.full((2, 1), 1000.0), S.COV, has="hnumo_cov_begin")
    e.cov_begin(None, None, 0)
    sid = e.sample_create_ref(xgl, [1, 2], np.zeros((2, 2)), S.COV)
    e.sample_series_begin(sid, every=0, capacity=1)
    # ... with no samples it cannot be sampled ...
    refused(e.sample, sid, has="the eddy covariances have no samples yet")
    refused(e.sample_record, sid, has="the eddy covariances have no samples yet")
    e.cov_accumulate()
    assert e.sample(sid).shape == (32, 2)
    e.cov_end()
    # ... and neither after hnumo_cov_end
    refused(e.sample, sid, has="hnumo_cov_begin")
    refused(e.sample_record, sid, has="hnumo_cov_begin")
    assert e.sample_series(sid).shape == (32, 2, 0)
