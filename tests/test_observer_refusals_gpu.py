"""The host-side refusals of the four field observers (flow statistics, vorticity products, eddy
covariances, energy budget): every C entry point of each, called through ctypes in each state in
which it refuses, with the return code 4 and the full hnumo_last_error text written out -- people grep
run logs for these texts and the Fortran bridge prints them.  Where several refusals apply at once the
order is part of the contract: not begun, then a NULL buffer, then a wrong n, then no samples; an
argument is refused before the state on the device is asked for.  Every case is refused on the host:
nothing is launched.  tests/test_observer_contract_gpu.py's case: bump10 at N = 2 (ngl = 3, L = 2, 100
elements) with tests/states.py's moving state, one engine per observer."""
import ctypes as C

import numpy as np
import pytest

import float_cases as FC

pytestmark = pytest.mark.gpu
L = 2
NO_STATE = "no state on the device yet (run a step first)"


@pytest.fixture(scope="module")
def case(case_factory):
    return FC.moving(case_factory, "bump10", {"nop": 2})


class Calls:
    """The raw calls on one engine: refused(text, name, *args) asserts code 4 and the whole message."""

    def __init__(self, case):
        from hnumo.engine import Engine, lib
        self.lib, self.e = lib(), Engine(case)
        self.st = self.e.state()
        self.e.set_resident(True)
        sc = case.scalars
        assert sc["nlayers"] == L
        self.npoin, self.npq = sc["npoin"], sc["npoin_q"]
        self.mem = np.zeros(16 * self.npoin * L + 2 * self.npq)    # room for the widest output
        self.buf = self.mem.ctypes.data_as(C.POINTER(C.c_double))
        self.i64 = C.c_int64(-7)

    def call(self, name, *args):
        return getattr(self.lib, name)(self.e.h, *args)

    def refused(self, text, name, *args):
        rc, msg = self.call(name, *args), self.lib.hnumo_last_error(self.e.h).decode()
        assert (rc, msg) == (4, f"{name}: {text}"), (name, args, rc, msg)

    def ok(self, name, *args):
        assert self.call(name, *args) == 0, (name, self.lib.hnumo_last_error(self.e.h).decode())

    def null_engine(self, name, *args):
        assert getattr(self.lib, name)(None, *args) == 4, name

    def close(self):
        assert not self.mem.any() and self.i64.value == -7       # no refusal wrote to its outputs
        self.e.close()


def test_flow_statistics(case):
    c = Calls(case)
    buf, cnt, first = c.buf, C.byref(c.i64), "call hnumo_stats_begin first"
    w4, w5 = 4 * c.npoin * L, 5 * c.npoin * L
    # before begin, with a NULL buffer and a wrong n together: not begun wins
    c.refused(first, "hnumo_stats_accumulate")
    c.refused(first, "hnumo_stats_sums", None, w4 - 1, cnt)
    c.refused(first, "hnumo_stats_set_sums", None, w4 - 1, -1)
    c.refused(first, "hnumo_stats_fields", None, w5 - 1)
    c.refused(first, "hnumo_stats_series", None, -1, cnt, 0)
    c.ok("hnumo_stats_end")                                        # (a no-op before begin)
    # negative arguments of begin
    c.refused("every and series_capacity must be >= 0, got -1, 2", "hnumo_stats_begin", -1, 2)
    c.refused("every and series_capacity must be >= 0, got 2, -1", "hnumo_stats_begin", 2, -1)
    c.ok("hnumo_stats_begin", 0, 1)
    # after begin, NULL and a wrong n: NULL wins
    c.refused("out is NULL", "hnumo_stats_sums", None, w4 - 1, cnt)
    c.refused("in is NULL", "hnumo_stats_set_sums", None, w4 - 1, -1)
    c.refused("out is NULL", "hnumo_stats_fields", None, w5 - 1)
    c.refused("out holds n = -1 values, the series has 2*nlayers*count = 0", "hnumo_stats_series", None, -1, cnt, 0)
    # a valid buffer and n = want - 1 (with a negative nsamples, with no samples: n wins)
    c.refused(f"n must be 4*npoin*nlayers = {w4}, got {w4 - 1}", "hnumo_stats_sums", buf, w4 - 1, cnt)
    c.refused(f"n must be 4*npoin*nlayers = {w4}, got {w4 - 1}", "hnumo_stats_set_sums", buf, w4 - 1, -1)
    c.refused(f"n must be 5*npoin*nlayers = {w5}, got {w5 - 1}", "hnumo_stats_fields", buf, w5 - 1)
    c.refused("out holds n = -1 values, the series has 2*nlayers*count = 0", "hnumo_stats_series", buf, -1, cnt, 0)
    # the right n: a negative nsamples, no samples, no state
    c.refused("nsamples must be >= 0", "hnumo_stats_set_sums", buf, w4, -1)
    c.refused("no samples yet", "hnumo_stats_fields", buf, w5)
    c.refused(NO_STATE, "hnumo_stats_accumulate")
    for name, args in (("hnumo_stats_begin", (0, 1)), ("hnumo_stats_accumulate", ()), ("hnumo_stats_sums", (buf, w4, cnt)),
                       ("hnumo_stats_set_sums", (buf, w4, 0)), ("hnumo_stats_fields", (buf, w5)),
                       ("hnumo_stats_series", (buf, 0, cnt, 0)), ("hnumo_stats_end", ())):
        c.null_engine(name, *args)
    c.close()


def test_vorticity_products(case):
    c = Calls(case)
    buf, cnt, first = c.buf, C.byref(c.i64), "call hnumo_vort_begin first"
    w4 = 4 * c.npoin * L
    c.refused(first, "hnumo_vort_fields", None, w4 - 1)
    c.refused(first, "hnumo_vort_record")
    c.refused(first, "hnumo_vort_series", None, -1, cnt, 0)
    c.ok("hnumo_vort_end")
    c.refused("every and series_capacity must be >= 0, got -1, 2", "hnumo_vort_begin", None, -1, 2)
    c.refused("every and series_capacity must be >= 0, got 2, -1", "hnumo_vort_begin", None, 2, -1)
    c.ok("hnumo_vort_begin", None, 0, 0)
    c.refused("out is NULL", "hnumo_vort_fields", None, w4 - 1)
    c.refused(f"n must be 4*npoin*nlayers = {w4}, got {w4 - 1}", "hnumo_vort_fields", buf, w4 - 1)
    c.refused("out holds n = -1 values, the series has 3*nlayers*count = 0", "hnumo_vort_series", None, -1, cnt, 0)
    c.refused("out holds n = -1 values, the series has 3*nlayers*count = 0", "hnumo_vort_series", buf, -1, cnt, 0)
    # no state on the device yet: ahead of "no series" for a record with series_capacity = 0
    c.refused(NO_STATE, "hnumo_vort_fields", buf, w4)
    c.refused(NO_STATE, "hnumo_vort_record")
    for name, args in (("hnumo_vort_begin", (None, 0, 1)), ("hnumo_vort_fields", (buf, w4)), ("hnumo_vort_record", ()),
                       ("hnumo_vort_series", (buf, 0, cnt, 0)), ("hnumo_vort_end", ())):
        c.null_engine(name, *args)
    c.close()


def test_eddy_covariances(case):
    c = Calls(case)
    buf, cnt, first = c.buf, C.byref(c.i64), "call hnumo_cov_begin first"
    w14, w16, w3 = 14 * c.npoin * L, 16 * c.npoin * L, 3 * L
    c.refused(first, "hnumo_cov_accumulate")
    c.refused(first, "hnumo_cov_sums", None, w14 - 1, cnt)
    c.refused(first, "hnumo_cov_set_sums", None, w14 - 1, -1)
    c.refused(first, "hnumo_cov_fields", None, w16 - 1)
    c.refused(first, "hnumo_cov_integrals", None, w3 - 1)
    c.ok("hnumo_cov_end")
    c.refused("every must be >= 0, got -1", "hnumo_cov_begin", None, None, -1)
    c.ok("hnumo_cov_begin", None, None, 0)
    c.refused("out is NULL", "hnumo_cov_sums", None, w14 - 1, cnt)
    c.refused("in is NULL", "hnumo_cov_set_sums", None, w14 - 1, -1)
    c.refused("out is NULL", "hnumo_cov_fields", None, w16 - 1)
    c.refused("out is NULL", "hnumo_cov_integrals", None, w3 - 1)
    c.refused(f"n must be 14*npoin*nlayers = {w14}, got {w14 - 1}", "hnumo_cov_sums", buf, w14 - 1, cnt)
    c.refused(f"n must be 14*npoin*nlayers = {w14}, got {w14 - 1}", "hnumo_cov_set_sums", buf, w14 - 1, -1)
    c.refused(f"n must be 16*npoin*nlayers = {w16}, got {w16 - 1}", "hnumo_cov_fields", buf, w16 - 1)
    c.refused(f"n must be 3*nlayers = {w3}, got {w3 - 1}", "hnumo_cov_integrals", buf, w3 - 1)
    c.refused("nsamples must be >= 0", "hnumo_cov_set_sums", buf, w14, -1)
    c.refused("no samples yet", "hnumo_cov_fields", buf, w16)
    c.refused("no samples yet", "hnumo_cov_integrals", buf, w3)
    c.refused(NO_STATE, "hnumo_cov_accumulate")
    for name, args in (("hnumo_cov_begin", (None, None, 0)), ("hnumo_cov_accumulate", ()), ("hnumo_cov_sums", (buf, w14, cnt)),
                       ("hnumo_cov_set_sums", (buf, w14, 0)), ("hnumo_cov_fields", (buf, w16)),
                       ("hnumo_cov_integrals", (buf, w3)), ("hnumo_cov_end", ())):
        c.null_engine(name, *args)
    c.close()


def test_energy_budget(case):
    c = Calls(case)
    buf, cnt, first = c.buf, C.byref(c.i64), "call hnumo_energy_begin first"
    wq, wn = 2 * c.npq, c.npoin * L
    null, nq2, nn = "quad2 or nodal is NULL", f"nq2 must be 2*npoin_q = {wq}, got {wq - 1}", f"nn must be npoin*nlayers = {wn}, got {wn - 1}"
    c.refused(first, "hnumo_energy_sample")
    c.refused(first, "hnumo_energy_series", None, -1, cnt, 0)
    c.refused(first, "hnumo_energy_sums", None, wq - 1, None, wn - 1, cnt)
    c.refused(first, "hnumo_energy_set_sums", None, wq - 1, None, wn - 1, -1)
    c.refused(first, "hnumo_energy_means", None, wq - 1, None, wn - 1)
    c.ok("hnumo_energy_end")
    c.refused("every and series_capacity must be >= 0, got -1, 2", "hnumo_energy_begin", None, -1, 2)
    c.refused("every and series_capacity must be >= 0, got 2, -1", "hnumo_energy_begin", None, 2, -1)
    c.ok("hnumo_energy_begin", None, 0, 0)
    # no series: ahead of the buffer's size
    c.refused("no series (hnumo_energy_begin was given series_capacity = 0)", "hnumo_energy_series", None, -1, cnt, 0)
    c.ok("hnumo_energy_begin", None, 0, 1)
    c.refused("out holds n = -1 values, the series has (3*nlayers+2)*count = 0", "hnumo_energy_series", None, -1, cnt, 0)
    c.refused("out holds n = -1 values, the series has (3*nlayers+2)*count = 0", "hnumo_energy_series", buf, -1, cnt, 0)
    # either buffer NULL and wrong sizes: NULL wins; nq2 is looked at before nn, both before nsamples
    for a, b in ((None, None), (None, buf), (buf, None)):
        c.refused(null, "hnumo_energy_sums", a, wq - 1, b, wn - 1, cnt)
        c.refused(null, "hnumo_energy_set_sums", a, wq - 1, b, wn - 1, -1)
        c.refused(null, "hnumo_energy_means", a, wq - 1, b, wn - 1)
    for text, q, n in ((nq2, wq - 1, wn - 1), (nq2, wq - 1, wn), (nn, wq, wn - 1)):
        c.refused(text, "hnumo_energy_sums", buf, q, buf, n, cnt)
        c.refused(text, "hnumo_energy_set_sums", buf, q, buf, n, -1)
        c.refused(text, "hnumo_energy_means", buf, q, buf, n)
    c.refused("nsamples must be >= 0", "hnumo_energy_set_sums", buf, wq, buf, wn, -1)
    c.refused("no samples yet", "hnumo_energy_means", buf, wq, buf, wn)
    c.refused(NO_STATE, "hnumo_energy_sample")
    for name, args in (("hnumo_energy_begin", (None, 0, 1)), ("hnumo_energy_sample", ()), ("hnumo_energy_series", (buf, 0, cnt, 0)),
                       ("hnumo_energy_sums", (buf, wq, buf, wn, cnt)), ("hnumo_energy_set_sums", (buf, wq, buf, wn, 0)),
                       ("hnumo_energy_means", (buf, wq, buf, wn)), ("hnumo_energy_end", ())):
        c.null_engine(name, *args)
    c.close()
