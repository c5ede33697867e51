"""The Fortran side of the region sets (include/hnumo_engine.f90): the module compiles with the
hnumo_regions_* interfaces, a program that calls each of them with the argument kinds the C header declares
compiles against it, and linking against the real library proves every bound symbol resolves."""
import os
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC = shutil.which("amdflang") or "/opt/rocm/lib/llvm/bin/amdflang"
REGIONS = ("hnumo_regions_create", "hnumo_regions_sample", "hnumo_regions_series", "hnumo_regions_area", "hnumo_regions_destroy")

PROG = """
program regions_calls
    use iso_c_binding
    use hnumo_engine_c
    implicit none
    type(c_ptr) :: eng
    integer(c_int32_t) :: labels(16), id
    real(c_double), target :: f(144), series(14, 3, 4)
    real(c_double) :: area(3)
    integer(c_int64_t) :: count
    integer(c_int) :: rc
    character(len=32) :: arg
    call get_command_argument(1, arg)
    print '(4I4)', HNUMO_ABI_EXPECTED, HNUMO_REGION_MAXSETS, HNUMO_REGION_FLOW, HNUMO_REGION_VORT
    if (trim(arg) /= 'call') stop
    ! (never reached by the test: there is no engine here; the calls are what the compiler checks)
    eng = c_null_ptr
    labels = 1_c_int32_t
    rc = hnumo_regions_create(eng, labels, int(size(labels), c_int64_t), 3_c_int32_t, HNUMO_REGION_FLOW + HNUMO_REGION_VORT, &
                              c_loc(f), 1_c_int32_t, 4_c_int32_t, id)
    rc = hnumo_regions_create(eng, labels, int(size(labels), c_int64_t), 3_c_int32_t, HNUMO_REGION_FLOW, c_null_ptr, &
                              0_c_int32_t, 4_c_int32_t, id)
    rc = hnumo_regions_sample(eng, id)
    rc = hnumo_regions_series(eng, id, c_null_ptr, 0_c_int64_t, count, 0_c_int32_t)
    rc = hnumo_regions_series(eng, id, c_loc(series), int(size(series), c_int64_t), count, 1_c_int32_t)
    rc = hnumo_regions_area(eng, id, area, int(size(area), c_int64_t))
    rc = hnumo_regions_destroy(eng, id)
end program regions_calls
"""


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_fortran_module_compiles_with_the_regions_interfaces():
    src = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    for fn in REGIONS:
        assert f"name='{fn}'" in src, fn
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "regions_calls.f90"), "w").write(PROG)
        subprocess.run([FC, "-c", os.path.join(REPO, "include", "hnumo_engine.f90")], cwd=d, check=True, capture_output=True)
        subprocess.run([FC, "-c", "regions_calls.f90"], cwd=d, check=True, capture_output=True)


@pytest.mark.skipif(not os.path.exists(FC) or not os.path.exists(os.path.join(REPO, "h-numo_amd", "libhnumo_engine.so")),
                    reason="no Fortran compiler or engine library")
def test_fortran_regions_symbols_resolve_and_the_abi_version_stays():
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "regions_calls.f90"), "w").write(PROG)
        subprocess.run([FC, "-c", os.path.join(REPO, "include", "hnumo_engine.f90")], cwd=d, check=True, capture_output=True)
        lib = os.path.join(REPO, "h-numo_amd")
        subprocess.run([FC, "regions_calls.f90", "hnumo_engine.o", "-o", "regions_calls", "-L" + lib, "-lhnumo_engine",
                        "-Wl,-rpath," + lib], cwd=d, check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "regions_calls")], check=True, capture_output=True, text=True).stdout
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    want = int(hdr.split("#define HNUMO_ABI_VERSION")[1].split()[0])
    assert int(out.split()[0]) == want == 10
    for name, v in zip(("HNUMO_REGION_MAXSETS", "HNUMO_REGION_FLOW", "HNUMO_REGION_VORT"), out.split()[1:4]):
        assert int(v) == int(hdr.split("#define " + name)[1].split()[0]), name
