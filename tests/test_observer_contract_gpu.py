"""What the four after-step observers (flow statistics, vorticity series, sample sets, float sets)
share: a series of `capacity` entries on the device with its refusals, its count query, clear and
re-begin.  The per-feature tests check these by substring or for some observers only; here every
observer meets the same list, with the message texts written out (people grep run logs for them and
the Fortran bridge prints them).  The smallest case of the observer tests: bump10 at N = 2 (ngl = 3,
L = 2, 100 elements) carrying tests/states.py's moving state."""
import ctypes as C

import numpy as np
import pytest

import float_cases as FC
from hnumo import floats as FL
from hnumo import sample as S

pytestmark = pytest.mark.gpu
KINDS = ["stats", "vort", "sample", "floats"]
L, M, V = 2, 6, 14                                             # layers, points of a set, 5L + 4 state values

AFTER = {"stats": "flow statistics after the step (the step itself succeeded): the series is full (1 samples): "
                  "nothing accumulated; read it with clear = 1",
         "vort": "vorticity series after the step (the step itself succeeded): the series is full (1 samples): "
                 "nothing recorded; read it with clear = 1",
         "sample": "sample series after the step (the step itself succeeded): the series of sample set 0 is full "
                   "(1 samples): nothing recorded; read it with clear = 1",
         "floats": "float set after the step (the step itself succeeded): the series of float set 0 is full "
                   "(1 records): nothing recorded; read it with clear = 1"}
EXPLICIT = {"stats": "hnumo_stats_accumulate: the series is full (1 samples): nothing accumulated; read it with clear = 1",
            "vort": "hnumo_vort_record: the series is full (1 samples): nothing recorded; read it with clear = 1",
            "sample": "hnumo_sample_record: the series of sample set 0 is full (1 samples): nothing recorded; "
                      "read it with clear = 1",
            "floats": "hnumo_floats_record: the series of float set 0 is full (1 records): nothing recorded; "
                      "read it with clear = 1"}
# an explicit record with capacity 0: the statistics accumulate (their sums need no series)
NO_SERIES = {"stats": None,
             "vort": "hnumo_vort_record: no series (hnumo_vort_begin with series_capacity = 0)",
             "sample": "hnumo_sample_record: the series of sample set 0 is full (0 samples): nothing recorded; "
                       "read it with clear = 1",
             "floats": "hnumo_floats_record: the series of float set 0 is full (0 records): nothing recorded; "
                       "read it with clear = 1"}
SHORT = {"stats": "hnumo_stats_series: out holds n = {n} values, the series has 2*nlayers*count = {want}",
         "vort": "hnumo_vort_series: out holds n = {n} values, the series has 3*nlayers*count = {want}",
         "sample": "hnumo_sample_series: out holds n = {n} values, the series has V*M*count = {want}",
         "floats": "hnumo_floats_series: out holds n = {n} values, the series has 5*M*count = {want}"}
NO_STATE = {"stats": "hnumo_stats_accumulate: no state on the device yet (run a step first)",
            "vort": "hnumo_vort_record: no state on the device yet (run a step first)",
            "sample": "hnumo_sample_record: no state on the device yet (run a step first)",
            "floats": "hnumo_floats_advance: no state on the device yet (run a step first)"}
NEGATIVE = {"stats": "hnumo_stats_begin: every and series_capacity must be >= 0, got -1, 2",
            "vort": "hnumo_vort_begin: every and series_capacity must be >= 0, got -1, 2",
            "sample": "hnumo_sample_series_begin: every and capacity must be >= 0, got -1, 2",
            "floats": "hnumo_floats_begin: record_every and capacity must be >= 0, got -1, 2"}
HEAD = {"stats": (2, L), "vort": (3, L), "sample": (V, M), "floats": (5, M)}


class Observer:
    """One observer of a resident engine behind the four verbs the series share.  `every` is the
    statistics', vorticity's and sample sets' every and the floats' record_every (their own every
    is 1: the engine advances them after each step)."""

    def __init__(self, kind, case):
        from hnumo.engine import Engine, lib
        self.kind, self.lib = kind, lib()
        self.e = Engine(case)
        self.st = self.e.state()
        self.e.set_resident(True)
        xy = FL.seed_grid(case, 3, 2)
        assert xy.shape[1] == M and case.scalars["nlayers"] == L
        self.ids = ()
        if kind == "sample":
            self.ids = (S.DeviceSampler(self.e, xy=xy).id,)
        if kind == "floats":
            self.ids = (FL.DeviceFloats(self.e, xy, 1).id,)
        assert self.ids in ((), (0,))
        self.width = int(np.prod(HEAD[kind]))

    def step(self):
        self.e.ti_rk_bcl(*self.st)

    def raw_begin(self, every, cap):
        e, lb = self.e, self.lib
        return {"stats": lambda: lb.hnumo_stats_begin(e.h, every, cap),
                "vort": lambda: lb.hnumo_vort_begin(e.h, None, every, cap),
                "sample": lambda: lb.hnumo_sample_series_begin(e.h, 0, every, cap),
                "floats": lambda: lb.hnumo_floats_begin(e.h, 0, 1, every, cap)}[self.kind]()

    def begin(self, every, cap):
        assert self.raw_begin(every, cap) == 0, self.error()

    def record(self):
        e = self.e
        {"stats": e.stats_accumulate, "vort": e.vort_record, "sample": lambda: e.sample_record(0),
         "floats": lambda: e.floats_record(0)}[self.kind]()

    def series(self, clear=False):
        e = self.e
        return {"stats": e.stats_series, "vort": e.vort_series, "sample": lambda c: e.sample_series(0, c),
                "floats": lambda c: e.floats_series(0, c)}[self.kind](clear)

    def raw_series(self, buf, n, clear):
        """(return code, count) of hnumo_*_series(out = buf or NULL, n, &count, clear)."""
        fn = getattr(self.lib, f"hnumo_{self.kind}_series")
        count = C.c_int64(-1)
        p = buf.ctypes.data_as(C.POINTER(C.c_double)) if buf is not None else None
        return fn(self.e.h, *self.ids, p, n, C.byref(count), clear), count.value

    def error(self):
        return self.lib.hnumo_last_error(self.e.h).decode()


def text(excinfo):
    """everything after the code's own words in an EngineError"""
    assert excinfo.value.code == 4
    return str(excinfo.value).split("): ", 1)[1]


@pytest.fixture(scope="module")
def case(case_factory):
    return FC.moving(case_factory, "bump10", {"nop": 2})


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_carry_their_full_texts(case, kind):
    from hnumo.engine import EngineError
    o = Observer(kind, case)
    # a negative argument of begin; no state on the device yet
    assert o.raw_begin(-1, 2) == 4 and o.error() == NEGATIVE[kind]
    o.begin(0, 1)
    with pytest.raises(EngineError) as ei:
        o.e.floats_advance(0, 1.0) if kind == "floats" else o.record()
    assert text(ei) == NO_STATE[kind]
    # a full series refuses the engine's own recording after a step, and an explicit one
    o.begin(1, 1)
    o.step()
    with pytest.raises(EngineError) as ei:
        o.step()
    assert text(ei) == AFTER[kind]
    with pytest.raises(EngineError) as ei:
        o.record()
    assert text(ei) == EXPLICIT[kind]
    # a buffer one value short, and a negative n
    want = o.width
    buf = np.zeros(want)
    assert o.raw_series(buf, want - 1, 0) == (4, -1) and o.error() == SHORT[kind].format(n=want - 1, want=want)
    assert o.raw_series(None, -1, 0) == (4, -1) and o.error() == SHORT[kind].format(n=-1, want=want)
    assert not buf.any()
    # an explicit recording with no series
    o.begin(0, 0)
    if NO_SERIES[kind] is None:
        o.record()
    else:
        with pytest.raises(EngineError) as ei:
            o.record()
        assert text(ei) == NO_SERIES[kind]
    o.e.close()


@pytest.mark.parametrize("kind", KINDS)
def test_count_query_and_clear(case, kind):
    o = Observer(kind, case)
    o.begin(1, 3)
    for _ in range(2):
        o.step()
    assert o.raw_series(None, 0, 0) == (0, 2)                   # the (NULL, 0) query
    assert o.raw_series(None, 0, 1) == (0, 2)                   # clear without a buffer: nothing read, nothing cleared
    assert o.raw_series(None, 0, 0) == (0, 2)
    two = o.series()
    assert two.shape == HEAD[kind] + (2,) and two.any() and np.isfinite(two).all()
    buf = np.zeros(2 * o.width + 3)
    assert o.raw_series(buf, buf.size, 1) == (0, 2)             # clear with a buffer: read, then empty
    assert np.array_equal(buf[:2 * o.width], two.reshape(-1, order="F")) and not buf[2 * o.width:].any()
    assert o.raw_series(None, 0, 0) == (0, 0)
    assert o.series().shape == HEAD[kind] + (0,)
    o.step()                                                    # the emptied series records from its first slot again
    assert o.series(clear=True).shape == HEAD[kind] + (1,) and o.series().shape == HEAD[kind] + (0,)
    o.e.close()


@pytest.mark.parametrize("kind", KINDS)
def test_second_begin_resets_and_capacity_zero_records_nothing(case, kind):
    o = Observer(kind, case)
    o.begin(2, 2)
    o.step()
    assert o.raw_series(None, 0, 0) == (0, 0)
    o.begin(2, 2)                                               # count and the step counter start again
    o.step()
    assert o.raw_series(None, 0, 0) == (0, 0)
    o.step()
    assert o.raw_series(None, 0, 0) == (0, 1)
    o.begin(2, 2)                                               # ... also with an entry held
    assert o.raw_series(None, 0, 0) == (0, 0)
    # capacity 0: the steps succeed and nothing is recorded (the floats: no record asked for)
    o.begin(0 if kind == "floats" else 1, 0)
    for _ in range(2):
        o.step()
    assert o.raw_series(None, 0, 0) == (0, 0)
    assert o.series(clear=True).shape == HEAD[kind] + (0,)
    o.e.close()
