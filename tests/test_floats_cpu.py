"""Float sets (hnumo_floats_*, hnumo/floats.py), the parts that need no GPU: the declarations on both
sides of the boundary, the Python mirror HostFloats on the CPU oracle's stepped states through
time_loop(floats=...), the seeding helpers and the trajectory file."""
import io
import os
import re

import numpy as np
import pytest

from hnumo import diagnostics as D
from hnumo import floats as FL
from hnumo import sample as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hnumo_floats_create", "hnumo_floats_get", "hnumo_floats_plan", "hnumo_floats_set", "hnumo_floats_advance",
       "hnumo_floats_begin", "hnumo_floats_record", "hnumo_floats_series", "hnumo_floats_destroy")


def test_header_fortran_module_and_python_declare_the_float_sets():
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    f90 = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    py = open(os.path.join(REPO, "h-numo_amd", "hnumo", "engine.py")).read()
    public = re.search(r"public :: hnumo_engine_create.*?\n\s*\n", f90, re.S).group(0)
    for fn in NEW:
        assert re.search(r"\bint\s+%s\s*\(hnumo_engine \*eng" % fn, hdr), fn
        assert f"name='{fn}'" in f90, fn
        assert re.search(r"\b%s\b" % fn, public), fn
        assert f"L.{fn}.argtypes" in py, fn
        assert re.search(r"def %s\(self" % fn[len("hnumo_"):], py), fn
    assert re.search(r"#define HNUMO_ABI_VERSION 10\b", hdr)      # additive: the version stays
    assert re.search(r"HNUMO_ABI_EXPECTED = 10\b", f90)
    for name, v in (("HNUMO_FLOAT_ACTIVE", 0), ("HNUMO_FLOAT_LEFT", 1), ("HNUMO_FLOAT_LOST", 2)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr) and re.search(r"%s = %d\b" % (name, v), f90)
    assert (FL.ACTIVE, FL.LEFT, FL.LOST) == (0, 1, 2)
    # the number of arguments agrees between the header and the ctypes declarations
    for fn in NEW:
        c_args = re.search(r"\bint\s+%s\s*\((.*?)\);" % fn, hdr, re.S).group(1).count(",") + 1
        py_args = re.search(r"L\.%s\.argtypes = \[(.*?)\]\n" % fn, py).group(1).count(",") + 1
        f_args = re.search(r"function %s\((.*?)\)" % fn, f90).group(1).count(",") + 1
        assert c_args == py_args == f_args, (fn, c_args, py_args, f_args)


def test_seed_helpers(case_factory):
    case = case_factory("bump10", nop=2)
    xy = FL.seed_grid(case, 4, 3)
    c = np.asarray(case.arrays["coord"])[0:2]
    assert xy.shape == (2, 12) and xy.flags["F_CONTIGUOUS"]
    assert (xy.min(axis=1) > c.min(axis=1)).all() and (xy.max(axis=1) < c.max(axis=1)).all()
    assert xy[0, 0] == xy[0, 2] and xy[1, 0] != xy[1, 1]        # point m = i*ny + j
    ring = FL.seed_ring((3.0, -1.0), 2.0, 7, phase=0.5)
    assert ring.shape == (2, 7) and np.abs(np.hypot(ring[0] - 3.0, ring[1] + 1.0) - 2.0).max() <= 4 * 2.0 ** -52 * 4
    assert np.isclose(np.arctan2(ring[1, 0] + 1.0, ring[0, 0] - 3.0), 0.5)
    with pytest.raises(ValueError):
        FL.seed_grid(case, 0, 3)
    with pytest.raises(ValueError):
        FL.seed_ring((0, 0), 1.0, 0)


def test_write_trajectories_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    series = rng.normal(size=(5, 6, 3))
    layer = np.array([1, 2, 3, 1, 2, 3], np.int32)
    status = np.array([0, 0, 1, 2, 0, 0], np.int32)
    path = str(tmp_path / "floats.npz")
    FL.write_trajectories(path, series, layer, status)
    s, l, st = FL.read_trajectories(path)
    assert np.array_equal(s, series) and np.array_equal(l, layer) and np.array_equal(st, status)
    assert l.dtype == np.int32 and st.dtype == np.int32
    with pytest.raises(ValueError):
        FL.write_trajectories(path, series[:4], layer, status)
    with pytest.raises(ValueError):
        FL.write_trajectories(path, series, layer, status[:5])


def test_host_floats_rejects_bad_seeds(case_factory):
    case = case_factory("bump10", nop=2)
    xy = FL.seed_grid(case, 2, 2)
    with pytest.raises(ValueError):
        FL.HostFloats(case, xy, 3)                              # L = 2
    with pytest.raises(ValueError):
        FL.HostFloats(case, xy, 0)
    with pytest.raises(ValueError):
        FL.HostFloats(case, xy[0], 1)
    hf = FL.HostFloats(case, xy, 1)
    with pytest.raises(ValueError):
        hf.set(xy[:, :3], 1)
    # seeds outside the domain and seeds that are not finite are LEFT from the start
    far = xy.copy(order="F")
    far[0, 0], far[1, 1] = 1e9, np.nan
    hf = FL.HostFloats(case, far, 1)
    assert list(hf.status) == [FL.LEFT, FL.LEFT, FL.ACTIVE, FL.ACTIVE] and list(hf.elem[:2]) == [0, 0]


def test_time_loop_advances_host_floats_on_the_oracles_states(case_factory, tmp_path):
    """time_loop(floats=HostFloats) over 3 oracle steps = the mirror advanced by hand on the states
    of a second oracle run; the floats' velocities are what HostSampler reads at their locations."""
    import oracle as O
    import float_cases as FC
    name, kw = FC.CASES[1]
    case = FC.moving(case_factory, name, kw)
    dt = case.scalars["dt"]
    xy, layer = FC.seeds(case)
    hf = FL.HostFloats(case, xy, layer)
    q, qb, qp = D.time_loop(case, O.Oracle(case), 3 * dt, out_dir=str(tmp_path), out=io.StringIO(), lcheck_conserved=False,
                            lprint_diagnostics=False, floats=hf)
    o = O.Oracle(case)
    st = o.state()
    by_hand = FL.HostFloats(case, xy, layer)
    for _ in range(3):
        o.ti_rk_bcl(*st)
        by_hand.advance(st[0])
    assert np.array_equal(st[0], q)
    a, b = hf.get(), by_hand.get()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    on = hf.status == FL.ACTIVE
    assert on.sum() > hf.M // 2 and not np.array_equal(a["x"][on], xy[0][on])
    v = S.HostSampler(case, hf.elem, hf.xi, hf.eta).sample(q, qb)
    m = np.arange(hf.M)
    assert np.array_equal(v[5 * (layer - 1) + 1, m], a["u"]) and np.array_equal(v[5 * (layer - 1) + 2, m], a["v"])
    # a list of sets, and a run without floats ends on the same state
    two = [FL.HostFloats(case, xy, layer), FL.HostFloats(case, xy[:, :5], layer[:5])]
    q2, _, _ = D.time_loop(case, O.Oracle(case), 3 * dt, out_dir=str(tmp_path), out=io.StringIO(), lcheck_conserved=False,
                           lprint_diagnostics=False, floats=two)
    assert np.array_equal(q2, q) and np.array_equal(two[0].x, hf.x) and np.array_equal(two[1].x, hf.x[:5])


def test_zero_dt_keeps_the_position_bit_for_bit(case_factory):
    import float_cases as FC
    name, kw = FC.CASES[0]
    case = FC.moving(case_factory, name, kw)
    xy, layer = FC.seeds(case)
    hf = FL.HostFloats(case, xy, layer)
    e0 = hf.elem.copy()
    for _ in range(2):
        hf.advance(case.arrays["q_df"], 0.0)
    assert np.array_equal(hf.x, xy[0]) and np.array_equal(hf.y, xy[1]) and np.array_equal(hf.elem, e0)
    on = e0 > 0
    assert (hf.wx[on] != 0).any() and not hf.fresh[on].any() and hf.fresh[~on].all()
