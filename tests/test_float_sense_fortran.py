"""The Fortran side of the float sets' sensors (include/hnumo_engine.f90): the module compiles with the
hnumo_floats_sensors / _sense / _sense_info interfaces, a program that calls each of them with the argument
kinds the C header declares compiles against it, and linking against the real library proves every bound
symbol resolves.  The manner of tests/test_wind_fortran.py."""
import os
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC = shutil.which("amdflang") or "/opt/rocm/lib/llvm/bin/amdflang"
SENSE = ("hnumo_floats_sensors", "hnumo_floats_sense", "hnumo_floats_sense_info")

PROG = """
program float_sense_calls
    use iso_c_binding
    use hnumo_engine_c
    implicit none
    type(c_ptr) :: eng
    real(c_double) :: out(9, 4), series(14, 4, 2)
    integer(c_int32_t) :: nrows, K
    integer(c_int64_t) :: count
    integer(c_int) :: rc
    character(len=32) :: arg
    call get_command_argument(1, arg)
    print '(2I4)', HNUMO_FLOAT_SENSE_STATE, HNUMO_FLOAT_SENSE_VORT
    if (trim(arg) /= 'call') stop
    ! (never reached by the test: there is no engine here; the calls are what the compiler checks)
    eng = c_null_ptr
    rc = hnumo_floats_sensors(eng, 0_c_int32_t, HNUMO_FLOAT_SENSE_STATE + HNUMO_FLOAT_SENSE_VORT)
    rc = hnumo_floats_begin(eng, 0_c_int32_t, 1_c_int32_t, 1_c_int32_t, 2_c_int32_t)
    rc = hnumo_floats_sense_info(eng, 0_c_int32_t, nrows, K)
    rc = hnumo_floats_sense(eng, 0_c_int32_t, out, int(size(out), c_int64_t))
    rc = hnumo_floats_series(eng, 0_c_int32_t, series, int(size(series), c_int64_t), count, 0_c_int32_t)
end program float_sense_calls
"""


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_fortran_module_compiles_with_the_sensor_interfaces():
    src = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    for fn in SENSE:
        assert f"name='{fn}'" in src, fn
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "float_sense_calls.f90"), "w").write(PROG)
        subprocess.run([FC, "-c", os.path.join(REPO, "include", "hnumo_engine.f90")], cwd=d, check=True, capture_output=True)
        subprocess.run([FC, "-c", "float_sense_calls.f90"], cwd=d, check=True, capture_output=True)


@pytest.mark.skipif(not os.path.exists(FC) or not os.path.exists(os.path.join(REPO, "h-numo_amd", "libhnumo_engine.so")),
                    reason="no Fortran compiler or engine library")
def test_fortran_sensor_symbols_resolve_and_constants_match_the_header():
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "float_sense_calls.f90"), "w").write(PROG)
        subprocess.run([FC, "-c", os.path.join(REPO, "include", "hnumo_engine.f90")], cwd=d, check=True, capture_output=True)
        lib = os.path.join(REPO, "h-numo_amd")
        subprocess.run([FC, "float_sense_calls.f90", "hnumo_engine.o", "-o", "float_sense_calls", "-L" + lib, "-lhnumo_engine",
                        "-Wl,-rpath," + lib], cwd=d, check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "float_sense_calls")], check=True, capture_output=True, text=True).stdout
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    want = [int(hdr.split("#define " + k)[1].split()[0]) for k in ("HNUMO_FLOAT_SENSE_STATE", "HNUMO_FLOAT_SENSE_VORT")]
    assert [int(x) for x in out.split()] == want == [1, 2]
