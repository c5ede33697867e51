"""Energy budget on the device (kernels_energy.hip through hnumo_energy_*): series, sums and means equal --
np.array_equal, no tolerance -- the numpy mirror hnumo.energy.HostEnergy fed with the per-step states of a
second, non-resident engine on the same moving case (whose bits equal the resident engine's:
tests/test_engine_gpu.py) and with the wind of each step, after 3 samples.  The resident engine is read before
any sync.

Shapes: the smallest at which the element groups of the 256-lane workgroup (EPG = 256 // Q whole elements, one
lane per quad point, a ragged last group) can go wrong:

    bump10 nop=2 6x6, botfr=2, cd=1e-3   P = 9,  Q = 25:  10 per group, 3 full groups + a ragged 6; L = 2
    bump10 nop=3 4x4                     P = 16, Q = 49:  5 per group, 3 full + a ragged 1 (padded t stride)
    dg25L3 4x4                           P = 25, Q = 81:  3 per group, 5 full + a ragged 1; L = 3, botfr = 1, wind
                                                          and viscosity on
    dg25L3 nop=5 3x3                     P = 36, Q = 121: 2 per group, 4 full + a ragged 1; 242 of 256 lanes
                                                          (padded t stride)
    dg25N7L3 3x3                         P = 64, Q = 225: 1 per group, 9 groups
    qmbump8                              warped quadrilaterals (amplitudes halved as tests/test_cov_gpu.py does)
    dg25L3 nop=2 37x37                   1369 elements: the tree across a chunk of 1024
    lake10 nop=2 4x4, nlayers=1          one layer: top and bottom layer are the same
"""
import ctypes as C

import numpy as np
import pytest

import states
import wind_cases as WC
from hnumo import covariance as CV
from hnumo import energy as EN
from hnumo import flowstats as F
from hnumo import floats as FL
from hnumo import sample as S
from hnumo import vorticity as V
from hnumo import wind as W

pytestmark = pytest.mark.gpu
_moving, _runs = {}, {}

SHAPES = [("bump10", {"nop": 2, "nelx": 6, "nely": 6, "botfr": 2, "cd": 1e-3}), ("bump10", {"nop": 3, "nelx": 4, "nely": 4}),
          ("dg25L3", {"nelx": 4, "nely": 4}), ("dg25L3", {"nop": 5, "nelx": 3, "nely": 3}),
          ("dg25N7L3", {"nelx": 3, "nely": 3}), ("qmbump8", {})]
GROUPS = [(10, 3, 6), (5, 3, 1), (3, 5, 1), (2, 4, 1), (1, 9, 0), None]     # (per group, full groups, ragged rest)
STATE = {"qmbump8": dict(amp=0.005, fr=0.001, jump=0.005)}
SMALL2 = SHAPES[0]            # L = 2, quadratic drag, no wind, no viscosity
SMALL3 = SHAPES[2]            # L = 3, wind, linear drag, viscosity
ONE = ("lake10", {"nop": 2, "nelx": 4, "nely": 4, "nlayers": 1})


def moving(case_factory, name, kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _moving:
        rest = case_factory(name, **kw)
        _moving[key] = (states.moving_case(rest, **STATE.get(name, {})), CV.rest_elevations(rest))
    return _moving[key]


def stepped_states(case_factory, name, kw, nsteps=3):
    """(case, zref, [q_df after step 1..nsteps], final (q, qb, qp)) from a non-resident engine that never began
    the observer (once per case)."""
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


def mirror(case, qs, taus=None, **kw):
    he = EN.HostEnergy(case, **kw)
    for i, q in enumerate(qs):
        he.add(q, None if taus is None else taus[i])
    return he


def read(de, series=True):
    """(series or None, quad, nodal, nsamples, mean quad, mean nodal) of a device object"""
    quad, nodal, n = de.sums()
    mq, mn = de.means()
    return (de.series() if series else None), quad, nodal, n, mq, mn


def assert_equal_mirror(got, he, what=""):
    ser, quad, nodal, n, mq, mn = got
    hq, hn, hcount = he.sums()
    assert n == hcount, (what, n, hcount)
    for nm, a, b in (("S_W", quad[0], hq[0]), ("S_D", quad[1], hq[1]), ("S_V", nodal, hn)):
        assert np.isfinite(a).all() and np.array_equal(a, b), (what, nm, float(np.abs(a - b).max()))
    hmq, hmn = he.means()
    assert np.array_equal(mq, hmq) and np.array_equal(mn, hmn), (what, "means")
    if ser is not None:
        want = he.series()
        assert ser.shape == want.shape and np.isfinite(ser).all(), (what, ser.shape, want.shape)
        for r, nm in enumerate(EN.series_names(he.L)):
            assert np.array_equal(ser[r], want[r]), (what, "series", nm, ser[r], want[r])


def resident_run(case, nsteps, series=True, **kw):
    """nsteps resident steps with an explicit sample after each; everything read BEFORE any sync."""
    from hnumo.engine import Engine
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    de = EN.DeviceEnergy(e, every=0, series=nsteps if series else 0, **kw)
    for _ in range(nsteps):
        e.ti_rk_bcl(*st)
        de.add()
    got = read(de, series)
    e.close()
    return got


@pytest.mark.parametrize("name,kw,groups", [s + (g,) for s, g in zip(SHAPES, GROUPS)])
def test_series_sums_and_means_equal_mirror(case_factory, name, kw, groups):
    case, zref, qs, _ = stepped_states(case_factory, name, kw)
    Sc = case.scalars
    if groups:
        per, full, rest = groups
        assert 256 // Sc["nq"] ** 2 == per and divmod(Sc["nelem"], per) == (full, rest), (name, Sc["nq"], Sc["nelem"])
    got = resident_run(case, 3, zref=zref)
    assert_equal_mirror(got, mirror(case, qs, zref=zref), name)
    ser, quad, nodal = got[:3]
    L = Sc["nlayers"]
    assert (ser[:2 * L] > 0).all()
    # the terms the case has are non-zero somewhere, the others +0.0 everywhere
    wind, drag, visc = bool(np.asarray(case.arrays["tau_wind"]).any()), Sc["botfr"] != 0 and Sc["cd"] != 0, Sc["visc"] != 0
    for on, a, row in ((wind, quad[0], ser[3 * L]), (drag, quad[1], ser[3 * L + 1]), (visc, nodal, ser[2 * L:3 * L])):
        assert bool(a.any()) == on and bool(row.any()) == on, name
        assert on or not (np.signbit(a).any() or np.signbit(row).any()), name
    assert (quad[1] >= 0).all() and (nodal >= 0).all()
    if name == "dg25L3" and "nop" not in kw:
        assert wind and drag and visc
    if name == "bump10" and kw["nop"] == 2:
        assert drag and Sc["botfr"] == 2


def test_more_elements_than_one_reduction_chunk(case_factory):
    """E = 37*37 = 1369 elements at N=2: two chunks of the tree kernel, the second one ragged (345)."""
    case, zref, qs, _ = stepped_states(case_factory, "dg25L3", {"nelx": 37, "nely": 37, "nop": 2})
    assert case.scalars["nelem"] == 1369
    assert_equal_mirror(resident_run(case, 3, zref=zref), mirror(case, qs, zref=zref), "dg25L3 37x37")


def test_one_layer(case_factory):
    case, zref, qs, _ = stepped_states(case_factory, *ONE)
    assert case.scalars["nlayers"] == 1
    got = resident_run(case, 3, zref=zref)
    assert got[0].shape == (5, 3)
    assert_equal_mirror(got, mirror(case, qs, zref=zref), "one layer")


# ---------------------------------------------------------------- the wind the observer reads
def test_uniform_wind_installed_by_wind_set(case_factory):
    """A uniform wind, which no symmetry of the double gyre's own pattern can cancel, blended from two patterns
    by hnumo_wind_set.  The states come from an engine created with the blended wind, W from the mirror fed
    wind.blend(...)."""
    from hnumo.engine import Engine
    case, zref = moving(case_factory, *SMALL3)
    pat = np.zeros((2, case.scalars["npoin_q"], 2), order="F")
    pat[0, :, 0], pat[1, :, 0], pat[0, :, 1], pat[1, :, 1] = 0.08, -0.03, 0.01, 0.02
    coef = (0.5, 2.0)
    tau = W.blend(pat, coef)
    assert np.ptp(tau[0]) == 0 and np.ptp(tau[1]) == 0 and not np.array_equal(tau, case.arrays["tau_wind"])
    e0 = Engine(WC.with_wind(case, tau))
    q, qb, qp = e0.state()
    qs = []
    for _ in range(3):
        e0.ti_rk_bcl(q, qb, qp)
        qs.append(q.copy(order="F"))
    e0.close()
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    e.wind_begin(pat)
    e.wind_set(coef)
    de = EN.DeviceEnergy(e, zref=zref, every=1, series=3)
    for _ in range(3):
        e.ti_rk_bcl(*st)
    got = read(de)
    e.close()
    he = mirror(case, qs, [tau] * 3, zref=zref)
    assert_equal_mirror(got, he, "uniform wind")
    L = case.scalars["nlayers"]
    Wrow = got[0][3 * L]
    own = mirror(case, qs, zref=zref).series()[3 * L]
    assert Wrow.all() and not (Wrow == own).any(), (Wrow, own)             # the wind that was set, not the case's own
    assert not np.array_equal(got[1][0], mirror(case, qs, zref=zref).sums()[0][0])


@pytest.mark.parametrize("resident", [True, False])
def test_wind_schedule_row_k_is_under_the_row_step_k_used(case_factory, resident):
    """REPEAT over 3 steps, every = 1: the observer reads the resident wind, not the create-time one."""
    from hnumo.engine import Engine
    case = WC.case_of("N4", case_factory)
    pat = WC.patterns(case, 2)
    table = np.asfortranarray([[1.0, 0.25], [0.5, -1.0]])                     # coef(M = 2, nrows = 2): rows 0, 1, 0
    taus = [W.blend(pat, table[:, W.row_for(k, 2, 0, "repeat")]) for k in range(3)]
    assert np.array_equal(taus[0], taus[2]) and not np.array_equal(taus[0], taus[1])
    e0 = Engine(case)                                                          # the states: the same schedule, no observer
    e0.wind_begin(pat)
    e0.wind_schedule(table, mode="repeat")
    q, qb, qp = e0.state()
    qs = []
    for _ in range(3):
        e0.ti_rk_bcl(q, qb, qp)
        qs.append(q.copy(order="F"))
    e0.close()
    e = Engine(case)
    st = e.state()
    e.set_resident(resident)
    e.wind_begin(pat)
    e.wind_schedule(table, mode="repeat")
    de = EN.DeviceEnergy(e, every=1, series=3)
    for _ in range(3):
        e.ti_rk_bcl(*st)
    got = read(de)
    e.close()
    assert_equal_mirror(got, mirror(case, qs, taus), "schedule")
    L = case.scalars["nlayers"]
    created = mirror(case, qs).series()[3 * L]
    assert got[0][3 * L].all() and not (got[0][3 * L] == created).any()


# ---------------------------------------------------------------- observer variants
def test_zref_null(case_factory):
    """(zref given: the tests above.)  zref changes the APE rows and nothing else."""
    case, zref, qs, _ = stepped_states(case_factory, *SMALL3)
    got = resident_run(case, 3)
    assert_equal_mirror(got, mirror(case, qs), "zref NULL")
    full = mirror(case, qs, zref=zref).series()
    L = case.scalars["nlayers"]
    same = [r for r in range(3 * L + 2) if np.array_equal(got[0][r], full[r])]
    assert same == [r for r in range(3 * L + 2) if not L <= r < 2 * L]


def test_non_resident_engine_samples_its_last_output(case_factory):
    from hnumo.engine import Engine
    case, zref = moving(case_factory, *SMALL3)
    e = Engine(case)
    q, qb, qp = e.state()
    de = EN.DeviceEnergy(e, zref=zref, every=1, series=4)
    he = EN.HostEnergy(case, zref=zref)
    for _ in range(3):
        e.ti_rk_bcl(q, qb, qp)
        he.add(q)
    de.add()                                  # the output of the last call, once more
    he.add(q)
    got = read(de)
    e.close()
    assert got[3] == 4
    assert_equal_mirror(got, he, "non-resident")


def test_every_second_step_leaves_the_step_alone(case_factory):
    """every=2 over 6 steps: 3 samples, those of steps 2, 4, 6; q, qb, qprime end on the bits of a run that never
    began the observer."""
    from hnumo.engine import Engine
    case, zref, qs, final = stepped_states(case_factory, *SMALL3, 6)
    e = Engine(case)
    q, qb, qp = e.state()
    e.set_resident(True)
    de = EN.DeviceEnergy(e, zref=zref, every=2, series=3)
    for _ in range(6):
        e.ti_rk_bcl(q, qb, qp)
    got = read(de)
    e.sync(q, qb, qp)
    e.close()
    assert got[3] == 3
    assert_equal_mirror(got, mirror(case, [qs[1], qs[3], qs[5]], zref=zref), "every=2")
    for a, b in zip((q, qb, qp), final):
        assert np.array_equal(a, b)


def test_series_off_keeps_the_sums(case_factory):
    case, zref, qs, _ = stepped_states(case_factory, *SMALL3)
    got = resident_run(case, 3, series=False, zref=zref)
    assert got[0] is None
    assert_equal_mirror(got, mirror(case, qs, zref=zref, series=False), "series off")


def test_saved_sums_restored_after_end_continue_on_the_same_bits(case_factory):
    from hnumo.engine import Engine
    case, zref, qs, _ = stepped_states(case_factory, *SMALL3, 4)
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    de = EN.DeviceEnergy(e, zref=zref, every=1, series=4)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    quad, nodal, n = de.sums()
    first = de.series()
    de.end()
    de = EN.DeviceEnergy(e, zref=zref, every=1, series=4)        # a second begin: from zero
    assert de.nsamples == 0 and not de.sums()[0].any() and not de.sums()[1].any() and de.series().shape[1] == 0
    de.set_sums(quad, nodal, n)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    got = read(de)
    e.close()
    he = mirror(case, qs, zref=zref)
    assert n == 2 and got[3] == 4
    assert np.array_equal(np.concatenate([first, got[0]], axis=1), he.series())
    assert_equal_mirror((None,) + got[1:], he, "restored")


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
    des = [EN.DeviceEnergy(e, every=1, series=3) for e in engines]
    sts = [e.state() for e in engines]
    hosts = [EN.HostEnergy(p) for p in parts]
    for _ in range(3):
        group_ti_rk_bcl(engines, sts)
        for h, st in zip(hosts, sts):
            h.add(st[0])
    devs = [read(d) for d in des]
    for e in engines:
        e.close()
    for r, p in enumerate(parts):
        assert_equal_mirror(devs[r], hosts[r], (kind, r))
        Sc = p.scalars
        nown = p.nelem_owned * Sc["ngl"] ** 2 if kind == "ghost" else Sc["npoin"]
        nqown = p.nelem_owned * Sc["nq"] ** 2 if kind == "ghost" else Sc["npoin_q"]
        assert devs[r][1][:, :nqown].any() and devs[r][2][:nown].any()
        if kind == "ghost":
            assert nown < Sc["npoin"] and nqown < Sc["npoin_q"]
            assert not devs[r][1][:, nqown:].any() and not devs[r][2][nown:].any()       # ghost points read 0


def test_every_observer_on_at_once(case_factory):
    """Statistics, vorticity, covariances, a STATE sample set and a float set beside the energy budget: each of
    them records the bits it records on an engine that never began it, and the step's state is the same."""
    from hnumo.engine import Engine
    case, zref, qs, final = stepped_states(case_factory, *SMALL3)
    xy = FL.seed_grid(case, 3, 2)
    out = {}
    for with_energy in (False, True):
        e = Engine(case)
        q, qb, qp = e.state()
        e.set_resident(True)
        e.stats_begin(1, 3)
        e.vort_begin(V.coriolis_of(case), 1, 3)
        dc = CV.DeviceEddyCov(e, every=1, zref=zref)
        de = EN.DeviceEnergy(e, zref=zref, every=1, series=3) if with_energy else None
        ds = S.DeviceSampler(e, xy=xy)
        ds.series_begin(every=1, capacity=3)
        df = FL.DeviceFloats(e, xy, 1)
        df.begin(every=1, record_every=1, capacity=3)
        for _ in range(3):
            e.ti_rk_bcl(q, qb, qp)
        out[with_energy] = (e.stats_sums()[0], e.stats_series(), e.vort_series(), e.vort_fields(), dc.sums()[0], ds.series(),
                            df.series())
        if with_energy:
            got = read(de)
        e.sync(q, qb, qp)
        e.close()
        for a, b in zip((q, qb, qp), final):
            assert np.array_equal(a, b), with_energy
    for a, b in zip(out[False], out[True]):
        assert a.shape == b.shape
        assert a.any() and np.array_equal(a, b)
    he = mirror(case, qs, zref=zref)
    assert_equal_mirror(got, he, "all observers on")
    # the statistics' KE series on the same samples: KE_k here is theirs over alpha_k, to rounding
    L = case.scalars["nlayers"]
    for k in range(L):
        assert np.allclose(got[0][k], out[True][1][0, k] / he.alpha[k], rtol=1e-13, atol=0)


def test_redone_step_is_sampled_once(case_factory, monkeypatch):
    """The corrector's persistent launch of the first step gives up (hnumo_debug_force_abort(1)) and the step is
    redone on per-stage launches: 3 steps give 3 samples, those of an engine on per-stage launches from the start."""
    from hnumo.engine import Engine
    case, zref = moving(case_factory, *SMALL3)
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
        de = EN.DeviceEnergy(eng, zref=zref, every=1, series=4)
        for _ in range(3):
            eng.ti_rk_bcl(*st)
        out.append(read(de))
    assert e.persistent_stats["aborts"] == 1
    e.close()
    e0.close()
    assert out[0][3] == out[1][3] == 3 and out[0][0].shape == (11, 3)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    assert not np.array_equal(out[0][0][:, 0], out[0][0][:, 1])


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


def test_full_series_returns_4_with_the_step_done(small, case_factory):
    """capacity 2, every = 1: the third step returns 4, is done all the same and adds nothing; a read with
    clear makes room again."""
    from hnumo.engine import EngineError
    e = small
    case, _, qs, _ = stepped_states(case_factory, *SMALL2, 4)
    q, qb, qp = e.state()
    e.energy_begin(None, 1, 2)
    e.ti_rk_bcl(q, qb, qp)
    e.ti_rk_bcl(q, qb, qp)
    with pytest.raises(EngineError) as ei:
        e.ti_rk_bcl(q, qb, qp)
    assert ei.value.code == 4 and "energy budget after the step" in str(ei.value) and "the series is full (2 samples)" in str(ei.value)
    assert np.array_equal(q, qs[2])                                            # the step itself is done
    quad, nodal, n = e.energy_sums()
    he = mirror(case, qs[:2])
    assert n == 2 and np.array_equal(quad, he.sums()[0]) and np.array_equal(nodal, he.sums()[1])   # nothing accumulated
    refused(e.energy_sample, has="hnumo_energy_sample: the series is full")
    assert np.array_equal(e.energy_series(clear=True), he.series())
    e.ti_rk_bcl(q, qb, qp)
    assert np.array_equal(q, qs[3]) and e.energy_sums()[2] == 3
    he.add(qs[3])
    assert np.array_equal(e.energy_series(), he.series()[:, 2:])


def test_code4_before_begin(small):
    from hnumo.engine import lib
    e = small
    assert lib().hnumo_energy_end(e.h) == 0                      # a no-op
    for fn in (e.energy_sample, e.energy_sums, e.energy_means, e.energy_series):
        assert refused(fn, has="hnumo_energy_begin").startswith("hnumo_energy_")
    d = e.dims
    refused(e.energy_set_sums, np.zeros((2, d["npoin_q"]), order="F"), np.zeros((d["npoin"], d["nlayers"]), order="F"), 1,
            has="call hnumo_energy_begin first")


def test_code4_negative_every_or_capacity(small):
    assert refused(small.energy_begin, None, -1, 0, has="must be >= 0, got -1, 0").startswith("hnumo_energy_begin")
    assert refused(small.energy_begin, None, 0, -3, has="must be >= 0, got 0, -3").startswith("hnumo_energy_begin")
    refused(small.energy_sample, has="hnumo_energy_begin")       # still not begun


def test_code4_before_any_state_no_samples_no_series(small):
    e = small
    e.energy_begin(None, 0, 0)
    refused(e.energy_sample, has="hnumo_energy_sample: no state on the device yet")
    refused(e.energy_means, has="hnumo_energy_means: no samples yet")
    refused(e.energy_series, has="hnumo_energy_series: no series")
    quad, nodal, n = e.energy_sums()
    assert n == 0 and not quad.any() and not nodal.any()
    e.ti_rk_bcl(*e.state())
    refused(e.energy_means, has="no samples yet")                # a state, still no sample
    e.energy_sample()
    assert e.energy_sums()[2] == 1 and np.isfinite(e.energy_means()[0]).all()
    e.energy_begin(None, 0, 1)                                   # a second begin resets
    assert e.energy_sums()[2] == 0 and e.energy_series().shape == (8, 0)
    refused(e.energy_means, has="no samples yet")
    refused(e.energy_set_sums, quad, nodal, -1, has="nsamples must be >= 0")


def test_code4_wrong_n(small):
    from hnumo.engine import lib
    e = small
    d = e.dims
    L, npoin, npq = d["nlayers"], d["npoin"], d["npoin_q"]
    q, qb, qp = e.state()
    e.energy_begin(None, 1, 2)
    e.ti_rk_bcl(q, qb, qp)
    big = np.zeros(2 * npq + npoin * (L + 1) + 64)
    ptr = big.ctypes.data_as(C.POINTER(C.c_double))
    n64 = C.c_int64(-7)
    Lb = lib()
    calls = ((lambda: Lb.hnumo_energy_sums(e.h, ptr, 2 * npq - 1, ptr, npoin * L, C.byref(n64)), "hnumo_energy_sums: nq2 must be 2*npoin_q"),
             (lambda: Lb.hnumo_energy_sums(e.h, ptr, 2 * npq, ptr, npoin * L + 1, C.byref(n64)), "hnumo_energy_sums: nn must be npoin*nlayers"),
             (lambda: Lb.hnumo_energy_set_sums(e.h, ptr, npq, ptr, npoin * L, 1), "hnumo_energy_set_sums: nq2 must be 2*npoin_q"),
             (lambda: Lb.hnumo_energy_set_sums(e.h, ptr, 2 * npq, ptr, npoin, 1), "hnumo_energy_set_sums: nn must be npoin*nlayers"),
             (lambda: Lb.hnumo_energy_means(e.h, ptr, -1, ptr, npoin * L), "hnumo_energy_means: nq2 must be 2*npoin_q"),
             (lambda: Lb.hnumo_energy_means(e.h, ptr, 2 * npq, ptr, 0), "hnumo_energy_means: nn must be npoin*nlayers"),
             (lambda: Lb.hnumo_energy_series(e.h, ptr, 3 * L + 1, C.byref(n64), 1), "hnumo_energy_series: out holds n = "),
             (lambda: Lb.hnumo_energy_series(e.h, None, -1, C.byref(n64), 0), "hnumo_energy_series: out holds n = -1"))
    for call, who in calls:
        assert call() == 4 and not big.any() and n64.value == -7    # nothing written
        assert who in Lb.hnumo_last_error(e.h).decode(), Lb.hnumo_last_error(e.h).decode()
    assert e.energy_sums()[2] == 1 and e.energy_series().shape == (3 * L + 2, 1)   # the step's sample is still there


def test_failed_step_is_not_sampled(case_factory):
    """A step that returns code 1 or 2 (bump10 at time steps far beyond its stability limit) takes no sample."""
    from hnumo.engine import Engine, EngineError
    e = Engine(case_factory("bump10", dt=5.0e4, dt_btp=1.0e4))
    try:
        e.energy_begin(None, 1, 8)
        q, qb, qp = e.state()
        done = 0
        with pytest.raises(EngineError) as ei:
            for _ in range(3):
                e.ti_rk_bcl(q, qb, qp)
                done += 1
        assert ei.value.code in (1, 2)
        assert e.energy_sums()[2] == done and e.energy_series().shape[1] == done
    finally:
        e.close()
