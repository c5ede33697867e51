"""Online flow statistics on the device (kernels_stats.hip through hnumo_stats_*): sums, fields and
series equal -- np.array_equal, no tolerance -- the numpy mirror hnumo.flowstats.HostFlowStats fed
with the per-step states of a second, non-resident engine on the same case (whose bits equal the
resident engine's: tests/test_engine_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

from hnumo import flowstats as F

pytestmark = pytest.mark.gpu
_runs = {}


def stepped_states(case_factory, name, kw, nsteps):
    """(case, [q_df after step 1..nsteps]) from a non-resident engine (computed once per case)."""
    from hnumo.engine import Engine
    key = (name, tuple(sorted(kw.items())), nsteps)
    if key not in _runs:
        case = case_factory(name, **kw)
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


def mirror(case, states):
    st = F.HostFlowStats(case)
    for q in states:
        st.add(q)
    return st


def assert_equal_mirror(dev, host, what=""):
    """dev: (sums, nsamples, fields, series) read from an engine."""
    sums, n, fields, series = dev
    assert n == host.nsamples, what
    assert np.array_equal(sums, host.sums), (what, "sums", float(np.abs(sums - host.sums).max()))
    hf = host.fields()
    assert np.array_equal(fields, hf), (what, "fields", float(np.abs(fields - hf).max()))
    assert series.shape == host.series.shape, (what, series.shape, host.series.shape)
    assert np.array_equal(series, host.series), (what, "series", series, host.series)


def read_all(e):
    s, n = e.stats_sums()
    return s, n, e.stats_fields(), e.stats_series()


def resident_sampled(case, nsteps, series=None):
    """nsteps resident steps with an explicit sample after each; everything read BEFORE any sync."""
    from hnumo.engine import Engine
    e = Engine(case)
    q, qb, qp = e.state()
    e.set_resident(True)
    st = F.DeviceFlowStats(e, every=0, series=nsteps if series is None else series)
    for _ in range(nsteps):
        e.ti_rk_bcl(q, qb, qp)
        st.add()
    got = (st.sums, st.nsamples, st.fields(), st.series)
    ken = st.ke_normalised()
    e.close()
    return got, ken


# dg25L3 5x3: E = 15 is odd and the last element group (10 per group at N=4) is ragged, L=3;
# bump10 at N=2: P = 9, 28 elements per group, L=2; qmbump8: warped quadrilaterals with a non-uniform
# jac, E = 64 a power of two; dg25N7L3 3x3: P = 64 (4 elements per group) and E = 9
@pytest.mark.parametrize("name,kw,nsteps", [("dg25L3", {"nelx": 5, "nely": 3}, 4), ("bump10", {"nop": 2}, 3),
                                            ("qmbump8", {}, 3), ("dg25N7L3", {"nelx": 3, "nely": 3}, 3)])
def test_resident_statistics_equal_mirror(case_factory, name, kw, nsteps):
    case, states, _ = stepped_states(case_factory, name, kw, nsteps)
    if name == "qmbump8":
        jac = np.asarray(case.arrays["jac"]).reshape(case.scalars["ngl"] ** 2, -1, order="F")
        assert (jac.max(axis=1) > 1.01 * jac.min(axis=1)).all()      # the weights differ between elements
    got, ken = resident_sampled(case, nsteps)
    host = mirror(case, states)
    assert_equal_mirror(got, host, name)
    assert np.array_equal(ken, host.ke_normalised())
    assert np.isfinite(got[2]).all()


def test_more_elements_than_one_reduction_chunk(case_factory):
    """E = 37*37 = 1369 elements (odd, no power of two): two chunks of the tree kernel (1024
    elements each), the second one ragged (345), then the pass over the two chunk results."""
    case, states, _ = stepped_states(case_factory, "dg25L3", {"nelx": 37, "nely": 37, "nop": 2}, 2)
    assert case.scalars["nelem"] == 1369
    got, _ = resident_sampled(case, 2)
    assert_equal_mirror(got, mirror(case, states), "dg25L3 37x37")


def test_every_second_step_equals_explicit_samples(case_factory):
    """every=2 over 4 steps = explicit samples after steps 2 and 4; both runs end on the bits of a
    run that never began statistics."""
    from hnumo.engine import Engine
    case, states, final = stepped_states(case_factory, "bump10", {}, 4)
    out = {}
    for mode in ("every", "explicit"):
        e = Engine(case)
        q, qb, qp = e.state()
        e.set_resident(True)
        e.stats_begin(every=2 if mode == "every" else 0, series=4)
        for s in range(4):
            e.ti_rk_bcl(q, qb, qp)
            if mode == "explicit" and s % 2 == 1:
                e.stats_accumulate()
        got = read_all(e)
        e.sync(q, qb, qp)
        e.close()
        out[mode] = got
        for a, b in zip((q, qb, qp), final):
            assert np.array_equal(a, b), mode
    host = mirror(case, [states[1], states[3]])
    assert_equal_mirror(out["every"], host, "every=2")
    assert_equal_mirror(out["explicit"], host, "explicit")


def test_non_resident_engine_samples_its_last_output(case_factory):
    from hnumo.engine import Engine
    case = case_factory("bump10", nop=2)
    e = Engine(case)
    q, qb, qp = e.state()
    e.stats_begin(every=1, series=3)
    host = F.HostFlowStats(case)
    for _ in range(2):
        e.ti_rk_bcl(q, qb, qp)
        host.add(q)
    e.stats_accumulate()                      # the output of the last call, once more
    host.add(q)
    got = read_all(e)
    e.close()
    assert_equal_mirror(got, host)


def group_run(parts, nsteps):
    """The ranks `parts` as a local exchange group, every=1: per rank what the engine holds and the
    mirror on that rank's own states."""
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    engines = [Engine(p) for p in parts]
    local_group(engines)
    for e in engines:
        e.stats_begin(every=1, series=nsteps)
    states = [e.state() for e in engines]
    hosts = [F.HostFlowStats(p) for p in parts]
    for _ in range(nsteps):
        group_ti_rk_bcl(engines, states)
        for h, st in zip(hosts, states):
            h.add(st[0])
    devs = [read_all(e) for e in engines]
    for e in engines:
        e.close()
    return devs, hosts


def test_two_face_ranks_in_a_local_group(case_factory):
    from hnumo.engine import Engine
    from hnumo.facepart import face_partition
    case = case_factory("bump10")
    devs, hosts = group_run([face_partition(case, 2, r, "block") for r in range(2)], 2)
    for r in range(2):
        assert_equal_mirror(devs[r], hosts[r], f"rank {r}")
    one = Engine(case)
    q, qb, qp = one.state()
    one.stats_begin(every=1, series=2)
    for _ in range(2):
        one.ti_rk_bcl(q, qb, qp)
    single = one.stats_series()
    one.close()
    # two summation orders of npoin non-negative terms, each within npoin * 2**-53 relative of
    # the exact sum
    total = devs[0][3][0] + devs[1][3][0]
    bound = 2 * case.scalars["npoin"] * 2.0 ** -53
    assert (single[0] > 0).all()
    assert np.all(np.abs(total - single[0]) <= bound * single[0]), (total, single[0])


def test_two_rank_ghost_layer_partition(case_factory):
    from hnumo.partition import partition
    case = case_factory("bump10")
    parts = [partition(case, 2, r) for r in range(2)]
    devs, hosts = group_run(parts, 2)
    for r, p in enumerate(parts):
        assert 0 < p.nelem_owned < p.scalars["nelem"]          # the rank holds ghosts
        assert_equal_mirror(devs[r], hosts[r], f"rank {r}")
        nown = p.nelem_owned * p.scalars["ngl"] ** 2
        sums, _, fields, _ = devs[r]
        assert not sums[:, nown:].any() and not fields[:, nown:].any()
        assert (sums[0, :nown] > 0).all()


def code_of(fn, *a):
    from hnumo.engine import EngineError
    with pytest.raises(EngineError) as ei:
        fn(*a)
    assert str(ei.value).split("): ", 1)[1].strip(), "empty message"
    return ei.value.code


def test_full_series_refuses_the_sample(case_factory):
    from hnumo.engine import Engine
    case, states, _ = stepped_states(case_factory, "bump10", {"nop": 2}, 3)
    e = Engine(case)
    q, qb, qp = e.state()
    e.set_resident(True)
    e.stats_begin(every=0, series=2)
    for s in range(3):
        e.ti_rk_bcl(q, qb, qp)
        if s < 2:
            e.stats_accumulate()
    assert code_of(e.stats_accumulate) == 4
    assert_equal_mirror(read_all(e), mirror(case, states[:2]), "after the refused sample")
    ser = e.stats_series(clear=True)
    assert ser.shape[2] == 2 and e.stats_series().shape[2] == 0
    e.stats_accumulate()                                        # room again: the state after step 3
    host = mirror(case, states)
    s, n = e.stats_sums()
    assert n == 3 and np.array_equal(s, host.sums)
    assert np.array_equal(e.stats_series(), host.series[:, :, 2:])
    e.close()


def test_restore_reset_and_error_paths(case_factory):
    from hnumo.engine import Engine, lib
    case, states, _ = stepped_states(case_factory, "bump10", {"nop": 2}, 3)
    host = mirror(case, states)
    L, npoin = case.scalars["nlayers"], case.scalars["npoin"]
    dp = C.POINTER(C.c_double)
    big = np.zeros(5 * npoin * (L + 1) + 8)
    ptr = big.ctypes.data_as(dp)
    n64 = C.c_int64()

    def raw(rc):
        assert rc == 4 and lib().hnumo_last_error(e.h).decode().strip()
        assert not big.any()                                    # nothing written

    e = Engine(case)
    # before hnumo_stats_begin: every call but end is refused
    assert lib().hnumo_stats_end(e.h) == 0
    assert code_of(e.stats_accumulate) == 4
    assert code_of(e.stats_sums) == 4
    assert code_of(e.stats_fields) == 4
    assert code_of(e.stats_series) == 4
    assert code_of(e.stats_set_sums, host.sums, 1) == 4
    # negative arguments
    assert code_of(e.stats_begin, -1, 0) == 4
    assert code_of(e.stats_begin, 0, -1) == 4
    # begun, but no state on the device yet
    e.stats_begin(every=0, series=0)
    assert code_of(e.stats_accumulate) == 4
    assert code_of(e.stats_fields) == 4                         # no samples
    q, qb, qp = e.state()
    e.set_resident(True)
    e.ti_rk_bcl(q, qb, qp)
    e.stats_accumulate()
    # series_capacity = 0: no series, the same sums
    assert e.stats_series().shape == (2, L, 0)
    s1, n1 = e.stats_sums()
    assert n1 == 1 and np.array_equal(s1, mirror(case, states[:1]).sums)
    # wrong n
    raw(lib().hnumo_stats_sums(e.h, ptr, 4 * npoin * L - 1, C.byref(n64)))
    raw(lib().hnumo_stats_sums(e.h, ptr, 4 * npoin * (L + 1), C.byref(n64)))
    raw(lib().hnumo_stats_fields(e.h, ptr, 5 * npoin * L + 1))
    raw(lib().hnumo_stats_set_sums(e.h, ptr, 4 * npoin * L + 4, 1))
    raw(lib().hnumo_stats_set_sums(e.h, ptr, 4 * npoin * L, -1))
    # hnumo_stats_begin twice resets; restore the first sample and go on: the uninterrupted run
    e.stats_begin(every=0, series=3)
    s0, n0 = e.stats_sums()
    assert n0 == 0 and not s0.any() and e.stats_series().shape[2] == 0
    e.stats_accumulate()
    raw(lib().hnumo_stats_series(e.h, ptr, 2 * L - 1, C.byref(n64), 0))      # out too small for one entry
    raw(lib().hnumo_stats_series(e.h, ptr, -1, C.byref(n64), 0))
    e.stats_begin(every=1, series=3)
    e.stats_set_sums(s1, n1)
    for _ in range(2):
        e.ti_rk_bcl(q, qb, qp)
    s, n = e.stats_sums()
    assert n == 3 and np.array_equal(s, host.sums)
    assert np.array_equal(e.stats_fields(), host.fields())
    assert np.array_equal(e.stats_series(), host.series[:, :, 1:])
    e.stats_end()
    assert code_of(e.stats_sums) == 4
    e.stats_end()                                               # a no-op again
    e.close()
