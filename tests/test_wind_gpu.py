"""The time-dependent wind on the device (hnumo_wind_*, csrc/kernels_wind.hip) against the CPU oracle, bit for bit:
an engine whose wind was set to tau must be an engine -- and an oracle -- created with tau.

The cases, the patterns and the oracle runs are tests/wind_cases.py's: the dg3 family with a moving state at
N = 2, 4, 7 and on a warped mesh, pattern 0 the case's own wind and the others random at every quad point.  Every
comparison is np.array_equal; the oracle results are computed once per (case, winds) and shared."""
import ctypes as C

import numpy as np
import pytest

import matrix as M
import wind_cases as W
from hnumo import wind
from test_matrix_gpu import first_difference, variant_engines

pytestmark = pytest.mark.gpu

_runs = {}


def oracle_run(name, case, taus):
    """(states after every step, the parity fields after the last) of the case's own state under taus[i]."""
    from hnumo import bundle as B
    key = (name, tuple(np.ascontiguousarray(t).tobytes() for t in taus))
    if key not in _runs:
        sts, o = W.Oracles(case).run(taus)
        assert all(np.isfinite(a).all() for a in sts[-1])
        _runs[key] = (sts, {f: o.field(f) for f, _ in B.FIELDS})
    return _runs[key]


def fields_of(e):
    from hnumo import bundle as B
    return {f: e.field(f) for f, _ in B.FIELDS}


def make_engine(case, path, monkeypatch):
    """An engine on a stage path ("default", "per-stage", "resident": the default path, resident) or under a
    kernel variant of tests/matrix.py."""
    from hnumo.engine import Engine
    if path in M.VARIANTS:
        e, = variant_engines(path, [case], monkeypatch)
        return e
    if path == "per-stage":
        monkeypatch.setenv("HNUMO_PERSISTENT", "0")
    e = Engine(case)
    monkeypatch.delenv("HNUMO_PERSISTENT", raising=False)
    assert e.stage_path == ("per-stage" if path == "per-stage" else "persistent")
    if path == "resident":
        e.set_resident(True)
    return e


SET_RUNS = [(c, p) for c in W.CELLS for p in ("default", "per-stage")] + \
           [("N4", "resident"), ("N4", "large"), ("N4", "large-nb4")]
COEF2 = (0.5, 0.25)


@pytest.mark.parametrize("name,path", SET_RUNS, ids=["-".join(r) for r in SET_RUNS])
def test_set_equals_create(name, path, case_factory, monkeypatch):
    """set c = (0.5, 0.25), two steps: the state and every parity field, tau_wind_ave among them (which the
    persistent path forms at create only), are the oracle's created with blend(patterns, c)."""
    case = W.case_of(name, case_factory)
    assert case.scalars["npoin_q"] == W.NPQ[name] and case.scalars["npoin_q"] % 256
    pat = W.patterns(case, 2)
    tau = wind.blend(pat, COEF2)
    so, ofields = oracle_run(name, case, [tau, tau])
    assert np.array_equal(ofields["tau_wind_ave"], wind.ave(tau, case.scalars["N_btp"]))
    e = make_engine(case, path, monkeypatch)
    try:
        e.wind_begin(pat)
        got, row = e.wind_get()
        assert row == -1 and np.array_equal(got, case.arrays["tau_wind"])      # unchanged until a set
        e.wind_set(COEF2)
        got, row = e.wind_get()
        assert row == -1 and np.array_equal(got, tau)
        st = e.state()
        for _ in range(2):
            e.ti_rk_bcl(*st)
        if path == "resident":
            e.sync(*st)
        fields = fields_of(e)
    finally:
        e.close()
    assert first_difference(st, so[-1], fields, ofields) is None


TABLE3 = np.asfortranarray([[1.0, 0.5, 0.25], [0.0, 0.5, -1.0], [0.75, -0.25, 0.125]])   # coef(M = 3, nrows = 3)
ROWS5 = {"repeat": [0, 1, 2, 0, 1], "hold": [0, 1, 2, 2, 2]}


def schedule_taus(case, mode):
    pat = W.patterns(case, 3)
    return pat, [wind.blend(pat, TABLE3[:, r]) for r in ROWS5[mode]]


@pytest.mark.parametrize("mode,resident", [("repeat", False), ("hold", False), ("repeat", True), ("hold", True)])
def test_schedule(mode, resident, case_factory):
    """Three rows over five steps against per-step oracles, next_row after every step; then first = 2 from the
    state after step 2 reproduces the tail of the same run."""
    from hnumo.engine import Engine
    case = W.case_of("N4", case_factory)
    pat, taus = schedule_taus(case, mode)
    so, _ = oracle_run("N4", case, taus)
    nxt = [wind.row_for(k, 3, 0, mode) for k in range(1, 6)]
    e = Engine(case)
    try:
        e.wind_begin(pat)
        e.wind_schedule(TABLE3, first=0, mode=mode)
        assert e.wind_get()[1] == 0
        st = e.state()
        e.set_resident(resident)
        for k in range(5):
            e.ti_rk_bcl(*st)
            if resident:
                e.sync(*st)
            tau, row = e.wind_get()
            assert row == nxt[k], (k, row)
            assert np.array_equal(tau, taus[k]), k
            assert W.same_state(st, so[k]), (k, first_difference(st, so[k], {}, {}))
        assert np.array_equal(e.field("tau_wind_ave"), wind.ave(taus[4], case.scalars["N_btp"]))
        # the tail: steps 2, 3, 4 of the table from the state after step 1
        e.wind_schedule(TABLE3, first=2, mode=mode)
        assert e.wind_get()[1] == 2
        st = tuple(a.copy(order="F") for a in so[1])
        e.set_resident(resident)                                              # (the next step uploads st)
        for k in range(2, 5):
            e.ti_rk_bcl(*st)
            if resident:
                e.sync(*st)
            assert e.wind_get()[1] == nxt[k]
            assert W.same_state(st, so[k]), (k, first_difference(st, so[k], {}, {}))
        # no rows: the schedule is gone, the wind stays
        e.wind_schedule(np.zeros((3, 0)))
        tau, row = e.wind_get()
        assert row == -1 and np.array_equal(tau, taus[4])
    finally:
        e.close()


@pytest.mark.parametrize("name", ["N2", "N7"])
def test_identity_table_is_a_never_begun_engine(name, case_factory):
    """M = 1, the pattern the create-time wind, rows (1.0,): every bit of the state and of the parity fields is
    that of an engine that never began."""
    from hnumo.engine import Engine
    case = W.case_of(name, case_factory)
    outs = []
    for begun in (False, True):
        e = Engine(case)
        try:
            if begun:
                e.wind_begin(W.patterns(case, 1))
                e.wind_schedule(np.ones((1, 2)), mode="repeat")
            st = e.state()
            for _ in range(2):
                e.ti_rk_bcl(*st)
            if begun:
                tau, row = e.wind_get()
                assert row == 0 and np.array_equal(tau, case.arrays["tau_wind"])
            outs.append((st, fields_of(e)))
        finally:
            e.close()
    (s0, f0), (s1, f1) = outs
    assert first_difference(s1, s0, f1, f0) is None


def test_redone_step_consumes_one_row(case_factory):
    """The corrector's persistent launch gives up (hnumo_debug_force_abort(1)) under a schedule: the step is redone
    inside the same call with the same row -- the undisturbed run's bits -- and next_row advances once."""
    from hnumo.engine import Engine
    case = W.case_of("N4", case_factory)
    pat, taus = schedule_taus(case, "repeat")
    so, _ = oracle_run("N4", case, taus)
    e = Engine(case)
    try:
        assert e.stage_path == "persistent"
        e.wind_begin(pat)
        e.wind_schedule(TABLE3, mode="repeat")
        e.debug_force_abort(1)
        st = e.state()
        e.ti_rk_bcl(*st)
        assert e.persistent_stats["aborts"] == 1 and e.stage_path == "per-stage"
        assert e.wind_get()[1] == 1
        assert W.same_state(st, so[0]), first_difference(st, so[0], {}, {})
        e.ti_rk_bcl(*st)
        assert e.wind_get()[1] == 2
        assert W.same_state(st, so[1]), first_difference(st, so[1], {}, {})
    finally:
        e.close()


def test_failed_step_does_not_advance(case_factory):
    """A step that returns code 1 or 2 (bump10 at time steps far beyond its stability limit) leaves next_row where
    it was: the rows taken are the successful steps."""
    from hnumo.engine import Engine, EngineError
    case = case_factory("bump10", dt=5.0e4, dt_btp=1.0e4)
    e = Engine(case)
    try:
        e.wind_begin(W.patterns(case, 2))
        e.wind_schedule(np.asfortranarray([[1.0] * 8, [0.0] * 8]), mode="hold")
        q, qb, qp = e.state()
        done = 0
        with pytest.raises(EngineError) as ei:
            for _ in range(3):
                assert e.wind_get()[1] == done
                e.ti_rk_bcl(q, qb, qp)
                done += 1
        assert ei.value.code in (1, 2)
        assert e.wind_get()[1] == done
    finally:
        e.close()


def test_end_restores_the_create_time_wind(case_factory):
    """After end: tau_wind, tau_wind_ave and the next two steps are those of a never-begun engine (the oracle of
    the case itself); a second begin after end works."""
    from hnumo.engine import Engine, EngineError
    case = W.case_of("N4warp", case_factory)
    pat = W.patterns(case, 3)
    tau0 = np.asarray(case.arrays["tau_wind"])
    so, ofields = oracle_run("N4warp", case, [tau0, tau0])
    e = Engine(case)
    try:
        e.wind_begin(pat)
        e.wind_set((0.1, 1.0, -1.0))
        st = e.state()
        e.ti_rk_bcl(*st)
        assert not W.same_state(st, so[0])                                    # the other wind was felt
        e.wind_end()
        with pytest.raises(EngineError) as ei:
            e.wind_get()
        assert ei.value.code == 4
        st = e.state()
        for _ in range(2):
            e.ti_rk_bcl(*st)
        fields = fields_of(e)
        assert first_difference(st, so[-1], fields, ofields) is None
        assert np.array_equal(fields["tau_wind_ave"], wind.ave(tau0, case.scalars["N_btp"]))
        e.wind_begin(pat[:, :, :2])
        tau, row = e.wind_get()
        assert row == -1 and np.array_equal(tau, tau0)
        e.wind_set(COEF2)
        assert np.array_equal(e.wind_get()[0], wind.blend(pat[:, :, :2], COEF2))
        e.wind_end()
        assert np.array_equal(e.field("tau_wind_ave"), ofields["tau_wind_ave"])
    finally:
        e.close()


def test_second_begin_replaces_patterns_and_clears_the_schedule(case_factory):
    from hnumo.engine import Engine
    case = W.case_of("N2", case_factory)
    pat = W.patterns(case, 3)
    e = Engine(case)
    try:
        e.wind_begin(pat)
        e.wind_schedule(TABLE3, first=1, mode="hold")
        e.wind_set((0.0, 1.0, 0.0))
        assert e.wind_get()[1] == 1
        e.wind_begin(pat[:, :, 2])
        tau, row = e.wind_get()
        assert row == -1 and np.array_equal(tau, pat[:, :, 1])                # the current wind is unchanged
        e.wind_set((2.0,))
        assert np.array_equal(e.wind_get()[0], 2.0 * pat[:, :, 2])
        e.wind_end()
        assert np.array_equal(e.field("tau_wind_ave"), wind.ave(case.arrays["tau_wind"], case.scalars["N_btp"]))
    finally:
        e.close()


def local_patterns(pc, pat, Q):
    quads = (np.asarray(pc.elems)[:, None] * Q + np.arange(Q)[None, :]).ravel()
    return np.asfortranarray(pat[:, quads, :])


@pytest.mark.parametrize("kind", ["face", "ghost"])
def test_scheduled_partitions_equal_the_single_rank_oracle(kind, case_factory):
    """Two ranks in a local group, every engine with its own schedule on its own elements' patterns (the ghost
    elements of a ghost-layer rank included), three steps: the gathered state is the single-rank oracle's."""
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    from hnumo.facepart import face_partition, gather_faces_state
    from hnumo.partition import gather_owned, partition
    case = W.case_of("N4", case_factory)
    pat, taus = schedule_taus(case, "repeat")
    so, _ = oracle_run("N4", case, taus)
    Q = case.scalars["nq"] ** 2
    parts = [face_partition(case, 2, r, "block") if kind == "face" else partition(case, 2, r) for r in range(2)]
    engines = [Engine(p) for p in parts]
    try:
        local_group(engines)
        for e, p in zip(engines, parts):
            e.wind_begin(local_patterns(p, pat, Q))
            e.wind_schedule(TABLE3, mode="repeat")
        sts = [e.state() for e in engines]
        for k in range(3):
            group_ti_rk_bcl(engines, sts)
            for e, p in zip(engines, parts):
                tau, row = e.wind_get()
                assert row == (k + 1) % 3
                assert np.array_equal(tau, local_patterns(p, taus[k][:, :, None], Q)[:, :, 0])
            for j, nm in enumerate(("q_df", "qb_df", "qprime_df")):
                loc = [(p, s[j]) for p, s in zip(parts, sts)]
                got = gather_faces_state(loc, nm, case) if kind == "face" else gather_owned(loc, nm, case)
                assert np.array_equal(got, so[k][j]), (kind, k, nm, float(np.abs(got - so[k][j]).max()))
    finally:
        for e in engines:
            e.close()


def test_wind_begun_on_a_zero_wind_case(case_factory):
    """A lake cell, created with a wind of zeros, at N = 3 with two layers."""
    from hnumo.engine import Engine
    case = W.case_of(W.LAKE, case_factory)
    assert case.scalars["ngl"] == 4 and not np.asarray(case.arrays["tau_wind"]).any()
    pat = W.patterns(case, 2)
    tau = wind.blend(pat, (1.0, 0.5))
    assert np.array_equal(tau, 0.5 * pat[:, :, 1]) and np.abs(tau).max() > 0.01
    so, ofields = oracle_run(W.LAKE, case, [tau, tau])
    e = Engine(case)
    try:
        e.wind_begin(pat)
        e.wind_set((1.0, 0.5))
        st = e.state()
        for _ in range(2):
            e.ti_rk_bcl(*st)
        fields = fields_of(e)
    finally:
        e.close()
    assert first_difference(st, so[-1], fields, ofields) is None
    # and the wind is felt: the case's own oracle ends elsewhere
    s0, _ = oracle_run(W.LAKE, case, [np.asarray(case.arrays["tau_wind"])] * 2)
    assert not np.array_equal(s0[-1][1], so[-1][1])


def test_hooks_and_bench_steps_use_the_wind_in_place(case_factory):
    """predict under a set wind equals the oracle's created with it; neither it nor bench_steps advances the schedule."""
    import oracle as O
    from hnumo.engine import Engine
    case = W.case_of("N2", case_factory)
    pat = W.patterns(case, 2)
    tau = wind.blend(pat, COEF2)
    o = O.Oracle(W.with_wind(case, tau))
    so = o.state()
    o.predict(*so)
    e = Engine(case)
    try:
        e.wind_begin(pat)
        e.wind_schedule(np.asfortranarray([[0.5, 1.0], [0.25, 0.0]]), mode="hold")
        st = e.state()
        e.ti_rk_bcl(*st)                                                      # row 0 = COEF2
        assert e.wind_get()[1] == 1
        se = e.state()
        e.predict(*se)
        assert first_difference(se, so, {}, {}) is None
        e.set_resident(True)
        e.ti_rk_bcl(*e.state())
        assert e.wind_get()[1] == 1                                           # two rows, held
        e.bench_steps(2)
        tau1, row = e.wind_get()
        assert row == 1 and np.array_equal(tau1, pat[:, :, 0])                # row 1 = (1.0, 0.0), held
    finally:
        e.close()


def _refusals():
    """name -> (call on (lib, handle, case), the words its message must hold); every call but the first four
    comes after a begin with M = 2."""
    dp = C.POINTER(C.c_double)

    def ptr(a):
        return a.ctypes.data_as(dp)

    def pats(case, m):
        return np.zeros((2, case.scalars["npoin_q"], m), order="F")

    c2, tab, r = np.ones(2), np.ones((2, 3), order="F"), C.c_int32()
    return {
        "begin-M0": (False, lambda L, h, c: L.hnumo_wind_begin(h, ptr(pats(c, 1)), 2 * c.scalars["npoin_q"], 0),
                     ("hnumo_wind_begin", "M must be 1..4, got 0")),
        "begin-M5": (False, lambda L, h, c: L.hnumo_wind_begin(h, ptr(pats(c, 5)), 10 * c.scalars["npoin_q"], 5),
                     ("hnumo_wind_begin", "M must be 1..4, got 5")),
        "begin-null": (False, lambda L, h, c: L.hnumo_wind_begin(h, None, 4 * c.scalars["npoin_q"], 2),
                       ("hnumo_wind_begin", "patterns is NULL")),
        "begin-n": (False, lambda L, h, c: L.hnumo_wind_begin(h, ptr(pats(c, 2)), 4 * c.scalars["npoin_q"] - 1, 2),
                    ("hnumo_wind_begin", "n must be 2*npoin_q*M = %d, got %d")),
        "set-before-begin": (False, lambda L, h, c: L.hnumo_wind_set(h, ptr(c2), 2), ("hnumo_wind_set", "hnumo_wind_begin first")),
        "schedule-before-begin": (False, lambda L, h, c: L.hnumo_wind_schedule(h, ptr(tab), 2, 3, 0, 0),
                                  ("hnumo_wind_schedule", "hnumo_wind_begin first")),
        "get-before-begin": (False, lambda L, h, c: L.hnumo_wind_get(h, ptr(np.zeros(2 * c.scalars["npoin_q"])),
                                                                     2 * c.scalars["npoin_q"], C.byref(r)),
                             ("hnumo_wind_get", "hnumo_wind_begin first")),
        "end-before-begin": (False, lambda L, h, c: L.hnumo_wind_end(h), ("hnumo_wind_end", "hnumo_wind_begin first")),
        "set-M0": (True, lambda L, h, c: L.hnumo_wind_set(h, ptr(c2), 0), ("hnumo_wind_set", "M must be 1..4, got 0")),
        "set-other-M": (True, lambda L, h, c: L.hnumo_wind_set(h, ptr(np.ones(3)), 3),
                        ("hnumo_wind_set", "M = 3", "hnumo_wind_begin took M = 2")),
        "set-null": (True, lambda L, h, c: L.hnumo_wind_set(h, None, 2), ("hnumo_wind_set", "coef is NULL")),
        "schedule-M9": (True, lambda L, h, c: L.hnumo_wind_schedule(h, ptr(tab), 9, 3, 0, 0),
                        ("hnumo_wind_schedule", "M must be 1..4, got 9")),
        "schedule-other-M": (True, lambda L, h, c: L.hnumo_wind_schedule(h, ptr(tab), 1, 3, 0, 0),
                             ("hnumo_wind_schedule", "M = 1", "hnumo_wind_begin took M = 2")),
        "schedule-null": (True, lambda L, h, c: L.hnumo_wind_schedule(h, None, 2, 3, 0, 0), ("hnumo_wind_schedule", "coef is NULL")),
        "schedule-nrows": (True, lambda L, h, c: L.hnumo_wind_schedule(h, ptr(tab), 2, -1, 0, 0),
                           ("hnumo_wind_schedule", "nrows must be >= 0, got -1")),
        "schedule-first": (True, lambda L, h, c: L.hnumo_wind_schedule(h, ptr(tab), 2, 3, -2, 0),
                           ("hnumo_wind_schedule", "first must be >= 0, got -2")),
        "schedule-mode": (True, lambda L, h, c: L.hnumo_wind_schedule(h, ptr(tab), 2, 3, 0, 7),
                          ("hnumo_wind_schedule", "mode must be HNUMO_WIND_HOLD or HNUMO_WIND_REPEAT, got 7")),
        "get-null-tau": (True, lambda L, h, c: L.hnumo_wind_get(h, None, 2 * c.scalars["npoin_q"], C.byref(r)),
                         ("hnumo_wind_get", "tau is NULL")),
        "get-null-row": (True, lambda L, h, c: L.hnumo_wind_get(h, ptr(np.zeros(2 * c.scalars["npoin_q"])),
                                                                 2 * c.scalars["npoin_q"], None),
                         ("hnumo_wind_get", "next_row is NULL")),
        "get-n": (True, lambda L, h, c: L.hnumo_wind_get(h, ptr(np.zeros(2 * c.scalars["npoin_q"] + 1)),
                                                          2 * c.scalars["npoin_q"] + 1, C.byref(r)),
                  ("hnumo_wind_get", "n must be 2*npoin_q = %d, got %d")),
    }


REFUSALS = _refusals()


@pytest.fixture(scope="module")
def refusal_engine(case_factory):
    from hnumo.engine import Engine
    case = W.case_of("N2", case_factory)
    e = Engine(case)
    yield e, case
    e.close()


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(name, refusal_engine):
    """Every refusal is code 4 with a message that names the call and the value, and changes nothing."""
    from hnumo.engine import lib
    e, case = refusal_engine
    begun, call, words = REFUSALS[name]
    npq = case.scalars["npoin_q"]
    if begun:
        e.wind_begin(W.patterns(case, 2))
    try:
        assert call(lib(), e.h, case) == 4
        msg = lib().hnumo_last_error(e.h).decode()
        for w in words:
            if "%d" in w:
                w = w % ((4 * npq, 4 * npq - 1) if name == "begin-n" else (2 * npq, 2 * npq + 1))
            assert w in msg, (w, msg)
        if begun:
            tau, row = e.wind_get()
            assert row == -1 and np.array_equal(tau, case.arrays["tau_wind"])
    finally:
        if begun:
            e.wind_end()


def test_destroy_frees_a_begun_wind(case_factory):
    """hnumo_engine_destroy with a wind begun and scheduled; the next engine of the case is a fresh one."""
    from hnumo.engine import Engine
    case = W.case_of("N2", case_factory)
    e = Engine(case)
    e.wind_begin(W.patterns(case, 2))
    e.wind_schedule(np.ones((2, 2)))
    e.wind_set(COEF2)
    e.close()
    e = Engine(case)
    try:
        assert np.array_equal(e.field("tau_wind_ave"), wind.ave(case.arrays["tau_wind"], case.scalars["N_btp"]))
    finally:
        e.close()


def test_device_wind_in_time_loop(case_factory, tmp_path):
    """time_loop(wind=DeviceWind): the schedule is installed once at the loop's first step; five steps of a held
    three-row table equal the per-step oracles, and a loop restarted from snapshot 2 resumes the table."""
    import io
    from hnumo import diagnostics as D
    from hnumo.engine import Engine
    case = W.case_of("N4", case_factory)
    pat, taus = schedule_taus(case, "hold")
    so, _ = oracle_run("N4", case, taus)
    dt = case.scalars["dt"]
    e = Engine(case)
    try:
        dw = wind.DeviceWind(e, pat, TABLE3, "hold")
        got = D.time_loop(case, e, 4.5 * dt, out_dir=str(tmp_path), dump_data=True, out=io.StringIO(), wind=dw)
        assert dw.next_row == 2 and W.same_state(got, so[4])
        dw.end()
        dw = wind.DeviceWind(e, pat, TABLE3, "hold")
        got = D.time_loop(case, e, 4.5 * dt, out_dir=str(tmp_path), time_initial=2 * dt, restart_file_number=2,
                          out=io.StringIO(), wind=dw, lcheck_conserved=False)
        assert dw.next_row == 2
    finally:
        e.close()
    # the restarted loop starts from the snapshot's state: what the snapshot's text keeps of it, then
    # steps 2, 3, 4 of the table
    st = D.restart_state(case, str(tmp_path / "mlswe0002"))
    want, _ = W.Oracles(case).run(taus[2:], st)
    assert W.same_state(got, want[-1])
