"""The Fortran side of the energy budget (include/hnumo_engine.f90): the module compiles with the
hnumo_energy_* interfaces, a program that calls each of them with the argument kinds the C header declares
compiles against it, and linking against the real library proves every bound symbol resolves."""
import os
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC = shutil.which("amdflang") or "/opt/rocm/lib/llvm/bin/amdflang"
ENERGY = ("hnumo_energy_begin", "hnumo_energy_sample", "hnumo_energy_series", "hnumo_energy_sums", "hnumo_energy_set_sums",
          "hnumo_energy_means", "hnumo_energy_end")

PROG = """
program energy_calls
    use iso_c_binding
    use hnumo_engine_c
    implicit none
    type(c_ptr) :: eng
    real(c_double), target :: zref(9, 2), series(8, 4)
    real(c_double) :: quad(2, 25), nodal(9, 2)
    integer(c_int64_t) :: nsamples, count
    integer(c_int) :: rc
    character(len=32) :: arg
    call get_command_argument(1, arg)
    print '(I4)', HNUMO_ABI_EXPECTED
    if (trim(arg) /= 'call') stop
    ! (never reached by the test: there is no engine here; the calls are what the compiler checks)
    eng = c_null_ptr
    rc = hnumo_energy_begin(eng, c_loc(zref), 1_c_int32_t, 4_c_int32_t)
    rc = hnumo_energy_begin(eng, c_null_ptr, 0_c_int32_t, 0_c_int32_t)
    rc = hnumo_energy_sample(eng)
    rc = hnumo_energy_series(eng, c_null_ptr, 0_c_int64_t, count, 0_c_int32_t)
    rc = hnumo_energy_series(eng, c_loc(series), int(size(series), c_int64_t), count, 1_c_int32_t)
    rc = hnumo_energy_sums(eng, quad, int(size(quad), c_int64_t), nodal, int(size(nodal), c_int64_t), nsamples)
    rc = hnumo_energy_set_sums(eng, quad, int(size(quad), c_int64_t), nodal, int(size(nodal), c_int64_t), nsamples)
    rc = hnumo_energy_means(eng, quad, int(size(quad), c_int64_t), nodal, int(size(nodal), c_int64_t))
    rc = hnumo_energy_end(eng)
end program energy_calls
"""


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_fortran_module_compiles_with_the_energy_interfaces():
    src = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    for fn in ENERGY:
        assert f"name='{fn}'" in src, fn
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "energy_calls.f90"), "w").write(PROG)
        subprocess.run([FC, "-c", os.path.join(REPO, "include", "hnumo_engine.f90")], cwd=d, check=True, capture_output=True)
        subprocess.run([FC, "-c", "energy_calls.f90"], cwd=d, check=True, capture_output=True)


@pytest.mark.skipif(not os.path.exists(FC) or not os.path.exists(os.path.join(REPO, "h-numo_amd", "libhnumo_engine.so")),
                    reason="no Fortran compiler or engine library")
def test_fortran_energy_symbols_resolve_and_the_abi_version_stays():
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "energy_calls.f90"), "w").write(PROG)
        subprocess.run([FC, "-c", os.path.join(REPO, "include", "hnumo_engine.f90")], cwd=d, check=True, capture_output=True)
        lib = os.path.join(REPO, "h-numo_amd")
        subprocess.run([FC, "energy_calls.f90", "hnumo_engine.o", "-o", "energy_calls", "-L" + lib, "-lhnumo_engine",
                        "-Wl,-rpath," + lib], cwd=d, check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "energy_calls")], check=True, capture_output=True, text=True).stdout
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    want = int(hdr.split("#define HNUMO_ABI_VERSION")[1].split()[0])
    assert int(out.split()[0]) == want == 10
