"""The Fortran side of the time-dependent wind (include/hnumo_engine.f90): the module compiles with the
hnumo_wind_* interfaces, a program that calls each of them with the argument kinds the C header declares
compiles against it, and linking against the real library proves every bound symbol resolves."""
import os
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC = shutil.which("amdflang") or "/opt/rocm/lib/llvm/bin/amdflang"
WIND = ("hnumo_wind_begin", "hnumo_wind_set", "hnumo_wind_schedule", "hnumo_wind_get", "hnumo_wind_end")

PROG = """
program wind_calls
    use iso_c_binding
    use hnumo_engine_c
    implicit none
    type(c_ptr) :: eng
    real(c_double) :: patterns(2, 4, 2), coef(2, 3), tau(2, 4)
    integer(c_int32_t) :: next_row
    integer(c_int) :: rc
    character(len=32) :: arg
    call get_command_argument(1, arg)
    print '(3I4)', HNUMO_WIND_MAXM, HNUMO_WIND_HOLD, HNUMO_WIND_REPEAT
    if (trim(arg) /= 'call') stop
    ! (never reached by the test: there is no engine here; the calls are what the compiler checks)
    eng = c_null_ptr
    rc = hnumo_wind_begin(eng, patterns, int(size(patterns), c_int64_t), 2_c_int32_t)
    rc = hnumo_wind_set(eng, coef(:, 1), 2_c_int32_t)
    rc = hnumo_wind_schedule(eng, coef, 2_c_int32_t, 3_c_int32_t, 0_c_int32_t, HNUMO_WIND_REPEAT)
    rc = hnumo_wind_get(eng, tau, int(size(tau), c_int64_t), next_row)
    rc = hnumo_wind_end(eng)
end program wind_calls
"""


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_fortran_module_compiles_with_the_wind_interfaces():
    src = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    for fn in WIND:
        assert f"name='{fn}'" in src, fn
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "wind_calls.f90"), "w").write(PROG)
        subprocess.run([FC, "-c", os.path.join(REPO, "include", "hnumo_engine.f90")], cwd=d, check=True, capture_output=True)
        subprocess.run([FC, "-c", "wind_calls.f90"], cwd=d, check=True, capture_output=True)


@pytest.mark.skipif(not os.path.exists(FC) or not os.path.exists(os.path.join(REPO, "h-numo_amd", "libhnumo_engine.so")),
                    reason="no Fortran compiler or engine library")
def test_fortran_wind_symbols_resolve_and_constants_match_the_header():
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "wind_calls.f90"), "w").write(PROG)
        subprocess.run([FC, "-c", os.path.join(REPO, "include", "hnumo_engine.f90")], cwd=d, check=True, capture_output=True)
        lib = os.path.join(REPO, "h-numo_amd")
        subprocess.run([FC, "wind_calls.f90", "hnumo_engine.o", "-o", "wind_calls", "-L" + lib, "-lhnumo_engine",
                        "-Wl,-rpath," + lib], cwd=d, check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "wind_calls")], check=True, capture_output=True, text=True).stdout
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    want = [int(hdr.split("#define " + k)[1].split()[0]) for k in ("HNUMO_WIND_MAXM", "HNUMO_WIND_HOLD", "HNUMO_WIND_REPEAT")]
    assert [int(x) for x in out.split()] == want == [4, 0, 1]
