"""On-device run diagnostics (hnumo_diag_geometry / hnumo_diagnostics / hnumo_layer_fields), the
parts that need no GPU: the declarations on both sides of the boundary, the unpacking of the flat
result array, and time_loop's fall-back to the host path for a stepper without `diagnostics`."""
import io
import os
import re

import numpy as np
import pytest

from hnumo import diagnostics as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hnumo_diag_geometry", "hnumo_diagnostics", "hnumo_layer_fields")


def test_header_and_fortran_module_declare_the_diagnostics():
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    f90 = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    public = re.search(r"public :: hnumo_engine_create.*?\n\s*\n", f90, re.S).group(0)
    for fn in NEW:
        assert re.search(r"\bint\s+%s\s*\(hnumo_engine \*eng" % fn, hdr), fn
        assert f"name='{fn}'" in f90, fn
        assert re.search(r"\b%s\b" % fn, public), fn
    assert re.search(r"#define HNUMO_ABI_VERSION 10\b", hdr)      # additive: the version stays


@pytest.mark.parametrize("L", [2, 3])
def test_unpack_diagnostics_round_trip(L):
    from hnumo.engine import unpack_diagnostics
    n = 12 + 11 * L
    out = np.arange(1.0, n + 1.0)                      # every slot its own value
    d = unpack_diagnostics(out, L)
    assert set(d) == {"cfl_b", "cfl", "min_dx", "min_dy", "qbmax", "qbmin", "mass", "qmax", "qmin"}
    assert (d["cfl_b"], d["cfl"], d["min_dx"], d["min_dy"]) == (1.0, 2.0, 3.0, 4.0)
    assert np.array_equal(d["qbmax"], out[4:8]) and np.array_equal(d["qbmin"], out[8:12])
    assert d["qmax"].shape == (5, L) and d["qmin"].shape == (5, L) and d["mass"].shape == (L,)
    for k in range(L):
        b = 12 + 11 * k
        assert d["mass"][k] == out[b]
        assert np.array_equal(d["qmax"][:, k], out[b + 1:b + 6])
        assert np.array_equal(d["qmin"][:, k], out[b + 6:b + 11])
    # back to the flat layout
    flat = np.concatenate([[d["cfl_b"], d["cfl"], d["min_dx"], d["min_dy"]], d["qbmax"], d["qbmin"]] +
                          [np.concatenate([[d["mass"][k]], d["qmax"][:, k], d["qmin"][:, k]]) for k in range(L)])
    assert np.array_equal(flat, out)
    for bad in (n - 1, n + 1, 12 + 11 * (L + 1)):
        with pytest.raises(ValueError):
            unpack_diagnostics(np.zeros(bad), L)


def test_time_loop_device_diagnostics_falls_back_to_the_host(case_factory, tmp_path):
    """The CPU oracle has no `diagnostics`: device_diagnostics=True then reports on the host and
    writes what device_diagnostics=False writes."""
    import oracle as O
    case = case_factory("bump10")
    runs = {}
    for flag in (False, True):
        o = O.Oracle(case)
        assert not hasattr(o, "diagnostics")
        d = tmp_path / str(flag)
        buf = io.StringIO()
        st = D.time_loop(case, o, 200.0, out_dir=str(d), dump_data=True, out=buf, device_diagnostics=flag)
        files = {p.name: p.read_text() for p in sorted(d.iterdir())}
        runs[flag] = (buf.getvalue(), files, st)
    assert runs[True][0] == runs[False][0]
    assert sorted(runs[True][1]) == sorted(runs[False][1])
    assert {"mass_mlswe.cons", "mlswe_FIN.txt", "mlswe0000", "mlswe0002"} <= set(runs[True][1])
    for name, text in runs[False][1].items():
        assert runs[True][1][name] == text, name
    for a, b in zip(runs[True][2], runs[False][2]):
        assert np.array_equal(a, b)
