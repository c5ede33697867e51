"""The float sets' sensors on the device (kernels_float.hip: float_sense_kernel, through hnumo_floats_sensors /
_sense / _sense_info and the widened records): every comparison is np.array_equal, no tolerance -- with sample
sets at the floats' cached locations (no mirror involved), and with the Python mirror hnumo.floats.HostFloats
fed with the per-step states of a second, non-resident engine.  Cases and seeds are tests/float_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import float_cases as FC
import float_migrate_cases as MC
from hnumo import floats as FL
from hnumo import sample as S
from hnumo import vorticity as V
from test_floats_gpu import stepped_states

pytestmark = pytest.mark.gpu
STATE, VORT, ALL = FL.SENSE_STATE, FL.SENSE_VORT, FL.SENSE_STATE | FL.SENSE_VORT
KEYS = ("x", "y", "u", "v", "elem", "status")


def engine_with_floats(case, xy, layer, mask, resident=True, vort=True):
    """(engine, its state arrays, the set): vort_begin with the case's f before the sensors, as VORT needs."""
    from hnumo.engine import Engine
    e = Engine(case)
    st = e.state()
    if resident:
        e.set_resident(True)
    if vort:
        e.vort_begin(V.coriolis_of(case))
    return e, st, FL.DeviceFloats(e, xy, layer, sensors=mask)


def same(got, hf):
    want = hf.get()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


def slot_order(elem0):
    return np.argsort(elem0, kind="stable")


def blocks(elem_sorted):
    return [elem_sorted[b:b + 256] for b in range(0, elem_sorted.size, 256)]


# ------------------------------------------------------------------ 1. without the mirror
def test_sample_sets_at_the_cached_locations_read_the_sensor_rows(case_factory):
    """After 2 steps and 4 large advances a DeviceSampler(elem=, xi_eta=) of source STATE and one of source VORT
    at df.plan() read, for every float, its sensor rows: those of hnumo_floats_sense and of the last record."""
    name, kw = FC.CASES[0]
    case = FC.moving(case_factory, name, kw)
    xy, layer = FC.seeds(case)
    e, st, df = engine_with_floats(case, xy, layer, ALL)
    df.begin(every=1, record_every=1, capacity=6)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    big = FC.big_dt(case, st[0])                                # (st holds the initial state: a size, not bits)
    for _ in range(4):
        df.advance(dt=big)
    sense, ser, g = df.sense(), df.series(), df.get()
    elem, xi, eta = df.plan()
    xe = np.stack([xi, eta])
    vs = S.DeviceSampler(e, elem=elem, xi_eta=xe, source=S.STATE).sample()
    vv = S.DeviceSampler(e, elem=elem, xi_eta=xe, source=S.VORT).sample()
    info = df.sense_info()
    e.close()
    m, k = np.arange(elem.size), np.asarray(layer) - 1
    want = np.stack([vs[5 * k + v, m] for v in range(5)] + [vv[4 * k + v, m] for v in range(4)])
    assert sense.shape == (9, elem.size) and info[0] == 9 and info[1] >= 1
    assert np.array_equal(sense, want), int((sense != want).sum())
    assert ser.shape == (14, elem.size, 6) and np.array_equal(ser[5:, :, -1], want)
    assert np.array_equal(ser[6], ser[2]) and np.array_equal(ser[7], ser[3])      # the record's own u, v
    on = elem > 0
    assert on.sum() > elem.size // 2 and (~on).any() and not sense[:, ~on].any()
    assert (sense[:, on] != 0).any(axis=1).all() and np.isfinite(ser).all()
    assert np.array_equal(g["u"], sense[1]) and np.array_equal(g["v"], sense[2])


# ------------------------------------------------------------------ 2. against the mirror
@pytest.mark.parametrize("mask", [1, 2, 3])
@pytest.mark.parametrize("name,kw", FC.CASES, ids=FC.IDS)
def test_steps_then_large_advances_equal_the_mirror(case_factory, name, kw, mask):
    case = FC.moving(case_factory, name, kw)
    states, _ = stepped_states(case, name, 2)
    xy, layer = FC.seeds(case)
    dt, big = case.scalars["dt"], FC.big_dt(case, states[1])
    hf = FL.HostFloats(case, xy, layer, sensors=mask)
    for q, d in [(states[0], dt), (states[1], dt)] + [(states[1], big)] * 4:
        hf.advance(q, d)
        hf.record()
    want = hf.series()
    e, st, df = engine_with_floats(case, xy, layer, mask, vort=bool(mask & VORT))
    df.begin(every=1, record_every=1, capacity=6)
    for _ in range(2):
        e.ti_rk_bcl(*st)
    for _ in range(4):
        df.advance(dt=big)
    got, ser, sense = df.get(), df.series(), df.sense()
    e.close()
    same(got, hf)
    nS = FL.sense_rows(mask)
    assert ser.shape == want.shape == (5 + nS, hf.M, 6)
    assert np.array_equal(ser, want), [int((ser[r] != want[r]).sum()) for r in range(5 + nS)]
    assert np.array_equal(sense, want[5:, :, -1]) and np.isfinite(want).all()
    assert (want[5:, want[4, :, -1] > 0, -1] != 0).any(axis=1).all()


# ------------------------------------------------------------------ 3. the shapes at which the grouping can go wrong
def grouping_seeds(case):
    """700 floats in one element, tests/float_cases.py's seeds, and 520 points outside the domain (they sort first:
    two blocks wholly inactive), in a shuffled input order."""
    rng = np.random.default_rng(11)
    c = FC.corners_of(case)
    xy0, _ = FC.seeds(case)
    inside = np.array([FC.forward(c[37], *rng.uniform(-0.95, 0.95, 2)) for _ in range(700)]).T
    lo, hi = c.reshape(-1, 2).min(axis=0), c.reshape(-1, 2).max(axis=0)
    outside = np.stack([hi[0] + (hi[0] - lo[0]) * rng.uniform(0.1, 1.0, 520), rng.uniform(lo[1], hi[1], 520)])
    xy = np.concatenate([inside, xy0, outside], axis=1)
    xy = np.asfortranarray(xy[:, rng.permutation(xy.shape[1])])
    layer = rng.integers(1, case.scalars["nlayers"] + 1, xy.shape[1]).astype(np.int32)
    return xy, layer


def test_blocks_with_many_runs_repeats_gaps_and_no_active_float(case_factory):
    """bump10 at N = 2: two large advances, one of 8 x 0.7 element that loses the fast floats (a fifth hop),
    one more.  The mirror's elements in slot order are asserted to hold every shape named below, so the case
    cannot stop covering them silently."""
    name, kw = FC.CASES[1]
    case = FC.moving(case_factory, name, kw)
    states, _ = stepped_states(case, name, 2)
    xy, layer = grouping_seeds(case)
    big = FC.big_dt(case, states[1])
    hf = FL.HostFloats(case, xy, layer, sensors=ALL)
    e0 = hf.elem.copy()
    order = slot_order(e0)
    plan = [(states[0], None), (states[1], None), (states[1], big), (states[1], big), (states[1], 8 * big), (states[1], big)]
    for q, d in plan:
        hf.advance(q, d)
        hf.record()
    want = hf.series()
    e, st, df = engine_with_floats(case, xy, layer, ALL)
    K = df.sense_info()[1]
    df.begin(every=1, record_every=1, capacity=len(plan))
    for _ in range(2):
        e.ti_rk_bcl(*st)
    for _, d in plan[2:]:
        df.advance(dt=d)
    got, ser, sense = df.get(), df.series(), df.sense()
    e.close()
    # the shapes, on the mirror's elements in slot order at the last record (and at the one before the loss)
    assert (e0 == 38).sum() >= 700 and (e0 == 0).sum() >= 520
    many = repeat = gap = dead = False
    for rec in (3, len(plan) - 1):
        for b in blocks(want[4, order, rec].astype(np.int64)):
            slot, lst = FL.sense_slots(b)
            many |= lst.size > K
            repeat |= np.unique(lst).size < lst.size
            act = np.nonzero(b > 0)[0]
            gap |= act.size > 0 and (b[act[0]:act[-1] + 1] <= 0).any()
            dead |= not (b > 0).any()
    assert many and repeat and gap and dead, (many, repeat, gap, dead, K)
    assert (hf.status == FL.LOST).any() and (hf.status == FL.ACTIVE).sum() > 500
    same(got, hf)
    assert ser.shape == want.shape == (14, hf.M, len(plan))
    assert np.array_equal(ser, want), [int((ser[r] != want[r]).sum()) for r in range(14)]
    assert np.array_equal(sense, want[5:, :, -1])


@pytest.mark.parametrize("M", [1, 257])
def test_one_float_and_one_more_than_a_workgroup(case_factory, M):
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
    e, st, df = engine_with_floats(case, xy, layer, ALL)
    hf = df.host_floats()
    for _ in range(2):
        e.ti_rk_bcl(*st)
    assert np.array_equal(df.sense(), hf.sense(states[1]))        # before any advance: at the seeds
    for _ in range(2):
        df.advance(dt=big)
        hf.advance(states[1], big)
    got, sense = df.get(), df.sense()
    e.close()
    same(got, hf)
    want = hf.sense(states[1])
    assert sense.shape == (9, M) and np.array_equal(sense, want) and (want != 0).all()


# ------------------------------------------------------------------ 4. engine states and partitions
def test_record_every_two_two_sets_with_different_masks_and_the_state_bits(case_factory):
    name, kw = FC.CASES[0]
    case = FC.moving(case_factory, name, kw)
    states, final = stepped_states(case, name, 4)
    xy, layer = FC.seeds(case)
    ring = FL.seed_ring(FL.seed_grid(case, 6, 5)[:, 11], 1.0e5, 16)
    e, st, a = engine_with_floats(case, xy, layer, ALL)
    b, c = FL.DeviceFloats(e, ring, 2, sensors=STATE), FL.DeviceFloats(e, ring, 3)
    ha, hb, hc = a.host_floats(), b.host_floats(), c.host_floats()
    a.begin(every=1, record_every=2, capacity=2)
    b.begin(every=1, record_every=1, capacity=4)
    c.begin(every=1, record_every=1, capacity=4)
    for i in range(4):
        e.ti_rk_bcl(*st)
        for h in (ha, hb, hc):
            h.advance(states[i])
        hb.record(), hc.record()
        if i % 2:
            ha.record()
    sa, sb, sc = a.series(), b.series(), c.series()
    assert [a.sense_info()[0], b.sense_info()[0], c.sense_info()[0]] == [9, 5, 0]
    e.sync(*st)
    e.close()
    assert sa.shape == (14, ha.M, 2) and np.array_equal(sa, ha.series())
    assert sb.shape == (10, 16, 4) and np.array_equal(sb, hb.series())
    assert sc.shape == (5, 16, 4) and np.array_equal(sc, hc.series())
    assert not np.array_equal(sa[5:, :, 0], sa[5:, :, 1])
    for x, y in zip(st, final):                                  # the state's bits are those of a run with no set
        assert np.array_equal(x, y)


def test_redone_step_is_sensed_once(case_factory):
    """The corrector's persistent launch of the first step gives up (hnumo_debug_force_abort(1)) and the step is
    redone on per-stage launches: one record per step, on the state the step ended on."""
    from hnumo.engine import Engine
    name, kw = FC.CASES[0]
    case = FC.moving(case_factory, name, kw)
    states, final = stepped_states(case, name, 3)
    xy, layer = FC.seeds(case)
    e = Engine(case)
    assert e.stage_path == "persistent"
    e.debug_force_abort(1)
    st = e.state()
    e.set_resident(True)
    e.vort_begin(V.coriolis_of(case))
    df = FL.DeviceFloats(e, xy, layer, sensors=ALL)
    df.begin(every=1, record_every=1, capacity=3)
    for _ in range(3):
        e.ti_rk_bcl(*st)
    ser = df.series()
    aborts = e.persistent_stats["aborts"]
    e.sync(*st)
    e.close()
    assert aborts == 1
    hf = FL.HostFloats(case, xy, layer, sensors=ALL)
    for q in states:
        hf.advance(q)
        hf.record()
    assert ser.shape == (14, hf.M, 3) and np.array_equal(ser, hf.series())
    for x, y in zip(st, final):
        assert np.array_equal(x, y)


def test_non_resident_engine(case_factory):
    name, kw = FC.CASES[2]
    case = FC.moving(case_factory, name, kw)
    xy, layer = FC.seeds(case)
    e, st, df = engine_with_floats(case, xy, layer, ALL, resident=False)
    hf = df.host_floats()
    df.begin(every=1, record_every=1, capacity=2)
    for _ in range(2):
        e.ti_rk_bcl(*st)                                        # (st holds the state after the step)
        hf.advance(st[0])
        hf.record()
    ser, sense = df.series(), df.sense()
    e.close()
    assert np.array_equal(ser, hf.series()) and np.array_equal(sense, hf.sense(st[0]))


def test_two_rank_ghost_layer_partition(case_factory):
    """Each rank's set senses its owned elements from the rank's own state: the mirror on the rank's case."""
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    from hnumo.partition import partition
    case = FC.moving(case_factory, *FC.CASES[1])
    parts = [partition(case, 2, r) for r in range(2)]
    assert all(0 < p.nelem_owned < p.scalars["nelem"] for p in parts)
    xy, layer = FC.seeds(case, max_edge_elems=24)
    engines = [Engine(p) for p in parts]
    local_group(engines)
    for g, p in zip(engines, parts):
        g.vort_begin(V.coriolis_of(p))
    sets = [FL.DeviceFloats(g, xy, layer, sensors=ALL) for g in engines]
    mirrors = [FL.HostFloats(p, xy, layer, sensors=ALL) for p in parts]
    for s in sets:
        s.begin(every=1, record_every=1, capacity=2)
    sts = [g.state() for g in engines]
    for _ in range(2):
        group_ti_rk_bcl(engines, sts)
        for hf, stt in zip(mirrors, sts):
            hf.advance(stt[0])
            hf.record()
    got = [s.series() for s in sets]
    for g in engines:
        g.close()
    for r in range(2):
        want = mirrors[r].series()
        assert got[r].shape == want.shape == (14, xy.shape[1], 2)
        assert np.array_equal(got[r], want), (r, int((got[r] != want).sum()))
        assert 0 < (want[4, :, -1] > 0).sum() < xy.shape[1] and (want[5:, want[4, :, -1] > 0, -1] != 0).any()


def test_two_face_ranks_merged_series_is_the_single_rank_engines(case_factory):
    """bump10 on 2 block ranks with a migrating GroupFloats: the merged (5 + S) series equals the series of a
    single-rank engine on the whole mesh (whose state bits the two ranks carry: tests/test_float_migrate_gpu.py)."""
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    case, parts = MC.partition(case_factory, MC.ROWS[0])
    xy, layer = MC.seeds(case, parts)
    scale = float(np.abs(np.asarray(case.arrays["coord"])[0:2]).max())
    nstep, nbig = 2, 3
    engines = [Engine(p) for p in parts]
    local_group(engines)
    for g, p in zip(engines, parts):
        g.vort_begin(V.coriolis_of(p))
    gf = FL.GroupFloats(engines, xy, layer, coord_scale=scale, sensors=ALL)
    gf.begin(every=1, record_every=1, capacity=nstep + nbig)
    sts = [g.state() for g in engines]
    for _ in range(nstep):
        group_ti_rk_bcl(engines, sts)
    from hnumo.facepart import gather_faces_state
    big = FC.big_dt(case, gather_faces_state(list(zip(parts, [s[0] for s in sts])), "q_df", case))
    for _ in range(nbig):
        gf.advance(dt=big)
    sers = gf.series()
    for g in engines:
        g.close()
    e, st, one = engine_with_floats(case, xy, layer, ALL)
    one.begin(every=1, record_every=1, capacity=nstep + nbig)
    for _ in range(nstep):
        e.ti_rk_bcl(*st)
    for _ in range(nbig):
        one.advance(dt=big)
    ref = one.series()
    e.close()
    merged = FL.merge_series(sers, parts)
    assert merged.shape == ref.shape == (14, xy.shape[1], nstep + nbig)
    assert np.array_equal(merged, ref), int((merged != ref).any(axis=(0, 2)).sum())
    assert sum((s[4] > 0).astype(int) for s in sers).max() == 1
    crossed = sum(((s[4, :, 0] > 0) != (s[4, :, -1] > 0)).sum() for s in sers)
    assert crossed > 0 and (ref[4] > 0).sum() > 0.5 * ref[4].size


# ------------------------------------------------------------------ 5. a set with mask 0
def test_mask_zero_is_the_set_that_never_heard_of_sensors(case_factory):
    from hnumo.engine import EngineError
    name, kw = FC.CASES[1]
    case = FC.moving(case_factory, name, kw)
    xy, layer = FC.seeds(case)
    e, st, a = engine_with_floats(case, xy, layer, 0, vort=False)
    b = FL.DeviceFloats(e, xy, layer)
    e.floats_sensors(b.id, 0)
    msgs = []
    for df in (a, b):
        with pytest.raises(EngineError) as ei:
            df.record()                                           # no series
        msgs.append(str(ei.value).replace(f"set {df.id}", "set N"))
        df.begin(every=1, record_every=1, capacity=1)
    for _ in range(1):
        e.ti_rk_bcl(*st)
    with pytest.raises(EngineError) as ei:
        e.ti_rk_bcl(*st)                                          # both series are full
    assert ei.value.code == 4 and str(ei.value).endswith("float set after the step (the step itself succeeded): the series of float set "
                                                         f"{b.id} is full (1 records): nothing recorded; read it with clear = 1")
    n64 = C.c_int64()
    from hnumo.engine import lib
    buf = np.zeros(5 * a.engine._set_sizes("float", a.id))
    for df in (a, b):
        assert lib().hnumo_floats_series(e.h, df.id, buf.ctypes.data_as(C.POINTER(C.c_double)), buf.size - 1, C.byref(n64), 0) == 4
        msgs.append(lib().hnumo_last_error(e.h).decode())
        assert msgs[-1] == f"hnumo_floats_series: out holds n = {buf.size - 1} values, the series has 5*M*count = {buf.size}"
        assert df.sense_info() == (0, 0)
    sa, sb = a.series(), b.series()
    e.close()
    assert msgs[0] == msgs[1] and "is full (0 records)" in msgs[0]
    assert sa.shape == (5, xy.shape[1], 1) and np.array_equal(sa, sb) and sa.tobytes() == sb.tobytes()


# ------------------------------------------------------------------ 6. refusals
@pytest.fixture()
def small(case_factory):
    """(engine, state, xy, layer) of bump10 at N = 2 with no state on the device yet."""
    from hnumo.engine import Engine
    case = FC.moving(case_factory, *FC.CASES[1])
    e = Engine(case)
    yield e, e.state(), FL.seed_grid(case, 7, 5), 1
    e.close()


def refused(fn, text):
    from hnumo.engine import EngineError
    with pytest.raises(EngineError) as ei:
        fn()
    assert ei.value.code == 4 and text in str(ei.value), str(ei.value)


def test_refused_unknown_id(small):
    from hnumo.engine import lib
    e = small[0]
    for i in (0, 7, 8, -1):
        refused(lambda: e.floats_sensors(i, 1), f"hnumo_floats_sensors: no float set with id {i}")
        refused(lambda: e.floats_sense_info(i), f"hnumo_floats_sense_info: no float set with id {i}")
        out = np.zeros(5)
        assert lib().hnumo_floats_sense(e.h, i, out.ctypes.data_as(C.POINTER(C.c_double)), 5) == 4
        assert f"hnumo_floats_sense: no float set with id {i}" in lib().hnumo_last_error(e.h).decode() and not out.any()


def test_refused_unknown_bit(small):
    e, st, xy, layer = small
    df = FL.DeviceFloats(e, xy, layer)
    for bad in (4, 5, 8, -1):
        refused(lambda: e.floats_sensors(df.id, bad), "mask must be a sum of HNUMO_FLOAT_SENSE_STATE (1) and HNUMO_FLOAT_SENSE_VORT (2)")
    assert df.sense_info() == (0, 0)


def test_refused_vort_bit_before_vort_begin(small):
    e, st, xy, layer = small
    df = FL.DeviceFloats(e, xy, layer)
    for mask in (VORT, ALL):
        refused(lambda: e.floats_sensors(df.id, mask), "HNUMO_FLOAT_SENSE_VORT needs f: call hnumo_vort_begin first")
    e.floats_sensors(df.id, STATE)
    e.vort_begin(None)
    e.floats_sensors(df.id, ALL)
    assert df.sense_info()[0] == 9


def test_refused_mask_that_changes_the_width_of_a_series(small):
    e, st, xy, layer = small
    df = FL.DeviceFloats(e, xy, layer, sensors=STATE)
    df.begin(every=0, record_every=0, capacity=2)
    refused(lambda: e.floats_sensors(df.id, 0), "holds records of 10 rows, the mask asks for 5")
    e.vort_begin(None)
    refused(lambda: e.floats_sensors(df.id, ALL), "holds records of 10 rows, the mask asks for 14")
    e.floats_sensors(df.id, STATE)                                # (the same width)
    df.begin(every=0, record_every=0, capacity=0)                 # capacity 0 first, then the mask, then begin
    e.floats_sensors(df.id, ALL)
    df.begin(every=0, record_every=0, capacity=2)
    e.set_resident(True)
    e.ti_rk_bcl(*st)
    df.record()
    assert df.series().shape == (14, xy.shape[1], 1)
    n64 = C.c_int64()
    from hnumo.engine import lib
    buf = np.zeros(14 * xy.shape[1])
    assert lib().hnumo_floats_series(e.h, df.id, buf.ctypes.data_as(C.POINTER(C.c_double)), buf.size - 1, C.byref(n64), 0) == 4
    assert lib().hnumo_last_error(e.h).decode() == \
        f"hnumo_floats_series: out holds n = {buf.size - 1} values, the series has (5+S)*M*count = {buf.size}"
    assert not buf.any()


def test_refused_sense_without_sensors_and_with_a_wrong_n(small):
    e, st, xy, layer = small
    df = FL.DeviceFloats(e, xy, layer)
    refused(lambda: df.sense(), f"hnumo_floats_sense: float set {df.id} has no sensors")
    e.floats_sensors(df.id, STATE)
    from hnumo.engine import lib
    out = np.zeros(5 * xy.shape[1] + 1)
    assert lib().hnumo_floats_sense(e.h, df.id, out.ctypes.data_as(C.POINTER(C.c_double)), out.size) == 4
    assert "n must be S*M" in lib().hnumo_last_error(e.h).decode() and not out.any()
    assert lib().hnumo_floats_sense(e.h, df.id, None, out.size - 1) == 4


def test_refused_sense_and_record_before_any_state(small):
    e, st, xy, layer = small
    df = FL.DeviceFloats(e, xy, layer, sensors=STATE)
    df.begin(every=0, record_every=0, capacity=1)
    refused(lambda: df.sense(), "there is none on the device yet (run a step first)")
    refused(lambda: df.record(), "there is none on the device yet (run a step first)")
    assert df.series().shape == (10, xy.shape[1], 0)              # nothing was recorded
    e.set_resident(True)
    e.ti_rk_bcl(*st)
    df.record()
    assert np.array_equal(df.series()[5:, :, 0], df.sense())


def test_refused_vort_sensors_after_vort_end_and_the_due_record(small):
    """The due record of a step is refused like a full series: the step and the advance are done."""
    e, st, xy, layer = small
    e.set_resident(True)
    e.vort_begin(None)
    a, b = FL.DeviceFloats(e, xy, layer, sensors=ALL), FL.DeviceFloats(e, xy, layer, sensors=STATE)
    for df in (a, b):
        df.begin(every=1, record_every=1, capacity=2)
    e.ti_rk_bcl(*st)
    e.vort_end()
    refused(lambda: a.sense(), "hnumo_vort_end has been called")
    refused(lambda: a.record(), "hnumo_vort_end has been called")
    refused(lambda: e.ti_rk_bcl(*st), "float set after the step (the step itself succeeded)")
    ga, gb = a.get(), b.get()
    assert a.series().shape == (14, xy.shape[1], 1) and b.series().shape == (10, xy.shape[1], 2)   # b still recorded
    for k in KEYS:
        assert np.array_equal(ga[k], gb[k])                       # a advanced on the second step all the same
    assert not np.array_equal(b.series()[0, :, 0], b.series()[0, :, 1])
    assert b.sense().shape == (5, xy.shape[1])


# ------------------------------------------------------------------ 7. a group step after a refused recording
def test_group_step_runs_every_observer_after_a_refused_sensor_record(case_factory):
    """Two processor-face ranks, each with flow statistics (every = 1) and a migrating set whose VORT sensors
    lost their f (hnumo_vort_end): the group step returns 4 for the refused record, and the statistics of both
    ranks have their sample and the floats have advanced and migrated as in a run whose records are taken."""
    from hnumo.engine import Engine, EngineError, group_ti_rk_bcl, local_group
    case, parts = MC.partition(case_factory, MC.ROWS[0])
    xy, layer = MC.seeds(case, parts)
    scale = float(np.abs(np.asarray(case.arrays["coord"])[0:2]).max())

    def two_steps(end_vort):
        engines = [Engine(p) for p in parts]
        local_group(engines)
        for g, p in zip(engines, parts):
            g.vort_begin(V.coriolis_of(p))
            g.stats_begin(every=1, series=2)
        gf = FL.GroupFloats(engines, xy, layer, coord_scale=scale, sensors=ALL)
        gf.begin(every=1, record_every=1, capacity=2)
        sts = [g.state() for g in engines]
        group_ti_rk_bcl(engines, sts)
        if end_vort:
            for g in engines:
                g.vort_end()
            with pytest.raises(EngineError) as ei:
                group_ti_rk_bcl(engines, sts)
            assert ei.value.code == 4 and "hnumo_vort_end has been called" in str(ei.value)
        else:
            group_ti_rk_bcl(engines, sts)
        out = gf.get(), [g.stats_sums()[1] for g in engines], [s.shape[2] for s in gf.series()]
        for g in engines:
            g.close()
        return out

    (want, n_want, rec_want), (got, n_got, rec_got) = two_steps(False), two_steps(True)
    assert n_want == n_got == [2, 2] and rec_want == [2, 2] and rec_got == [1, 1]
    for r in range(2):
        assert (want[r]["status"] == FL.ACTIVE).any() and want[r]["u"].any()
        for k in KEYS:
            assert np.array_equal(got[r][k], want[r][k]), (r, k)
