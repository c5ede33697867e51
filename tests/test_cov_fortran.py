"""The Fortran side of the eddy covariances (include/hnumo_engine.f90): the module compiles with the
hnumo_cov_* interfaces, a program that calls each of them with the argument kinds the C header declares
compiles against it, and linking against the real library proves every bound symbol resolves."""
import os
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC = shutil.which("amdflang") or "/opt/rocm/lib/llvm/bin/amdflang"
COV = ("hnumo_cov_begin", "hnumo_cov_accumulate", "hnumo_cov_sums", "hnumo_cov_set_sums", "hnumo_cov_fields",
       "hnumo_cov_integrals", "hnumo_cov_end")

PROG = """
program cov_calls
    use iso_c_binding
    use hnumo_engine_c
    implicit none
    type(c_ptr) :: eng
    real(c_double), target :: f(9), zref(9, 2)
    real(c_double) :: sums(14, 9, 2), fields(16, 9, 2), integ(3, 2)
    integer(c_int64_t) :: nsamples
    integer(c_int) :: rc
    character(len=32) :: arg
    call get_command_argument(1, arg)
    print '(I4)', HNUMO_SAMPLE_COV
    if (trim(arg) /= 'call') stop
    ! (never reached by the test: there is no engine here; the calls are what the compiler checks)
    eng = c_null_ptr
    rc = hnumo_cov_begin(eng, c_loc(f), c_loc(zref), 1_c_int32_t)
    rc = hnumo_cov_begin(eng, c_null_ptr, c_null_ptr, 0_c_int32_t)
    rc = hnumo_cov_accumulate(eng)
    rc = hnumo_cov_sums(eng, sums, int(size(sums), c_int64_t), nsamples)
    rc = hnumo_cov_set_sums(eng, sums, int(size(sums), c_int64_t), nsamples)
    rc = hnumo_cov_fields(eng, fields, int(size(fields), c_int64_t))
    rc = hnumo_cov_integrals(eng, integ, int(size(integ), c_int64_t))
    rc = hnumo_cov_end(eng)
end program cov_calls
"""


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_fortran_module_compiles_with_the_cov_interfaces():
    src = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    for fn in COV:
        assert f"name='{fn}'" in src, fn
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "cov_calls.f90"), "w").write(PROG)
        subprocess.run([FC, "-c", os.path.join(REPO, "include", "hnumo_engine.f90")], cwd=d, check=True, capture_output=True)
        subprocess.run([FC, "-c", "cov_calls.f90"], cwd=d, check=True, capture_output=True)


@pytest.mark.skipif(not os.path.exists(FC) or not os.path.exists(os.path.join(REPO, "h-numo_amd", "libhnumo_engine.so")),
                    reason="no Fortran compiler or engine library")
def test_fortran_cov_symbols_resolve_and_the_source_matches_the_header():
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "cov_calls.f90"), "w").write(PROG)
        subprocess.run([FC, "-c", os.path.join(REPO, "include", "hnumo_engine.f90")], cwd=d, check=True, capture_output=True)
        lib = os.path.join(REPO, "h-numo_amd")
        subprocess.run([FC, "cov_calls.f90", "hnumo_engine.o", "-o", "cov_calls", "-L" + lib, "-lhnumo_engine",
                        "-Wl,-rpath," + lib], cwd=d, check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "cov_calls")], check=True, capture_output=True, text=True).stdout
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    want = int(hdr.split("#define HNUMO_SAMPLE_COV")[1].split()[0])
    assert int(out.split()[0]) == want == 3
