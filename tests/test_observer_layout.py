"""The host-only index work of the observers (h-numo_amd/csrc/observer_layout.h), run on the CPU.

tests/observer_layout_main.cpp includes the header; this module compiles it once per session with
AddressSanitizer and UBSan into a temporary directory and runs it as a child process.  Nothing is loaded
into Python.  The program's buffers have exactly the sizes their layouts say and its inputs hold 1, 2, 3 ...
in memory order, so every value says where it came from; the expected outputs are numpy's, written from the
layouts' words: the paired sums are [L][NP][npoin][2] on the device and (2*NP,npoin,L) for the caller
(include/hnumo_engine.h: hnumo_stats_sums at NP = 2, hnumo_cov_sums at NP = 7), a series entry is planar
[V][M] on the device and (V,M) for the caller."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="no g++ to compile tests/observer_layout_main.cpp with")


@pytest.fixture(scope="session")
def layout_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("observer_layout") / "observer_layout_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "observer_layout_main.cpp"), "-o", exe], check=True)
    return exe


def run(exe, *args):
    """the program's output lines as arrays of numbers"""
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (args, r.returncode, r.stderr[-2000:])   # (a sanitizer report fails the test)
    return [np.array(ln.split(), dtype=np.float64) for ln in r.stdout.split("\n")[:-1]]


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("NP", [2, 7])
@pytest.mark.parametrize("npoin", [1, 5, 27])
def test_paired_sums_pack_and_unpack(layout_exe, L, NP, npoin):
    n = 2 * NP * npoin * L
    caller = np.arange(1, n + 1, dtype=np.float64).reshape((2 * NP, npoin, L), order="F")
    device = np.empty((L, NP, npoin, 2))                       # C order: [L][NP][npoin][2]
    for k in range(L):
        for p in range(NP):
            for j in range(2):
                device[k, p, :, j] = caller[2 * p + j, :, k]
    packed, back = run(layout_exe, "pairs", L, NP, npoin)
    assert np.array_equal(packed, device.ravel()) and np.unique(packed).size == n
    assert np.array_equal(back, caller.ravel(order="F"))        # unpack after pack is the identity


@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("M", [1, 6])
@pytest.mark.parametrize("count", [0, 1, 3])
def test_transpose_of_planar_entries(layout_exe, V, M, count):
    planar = np.arange(1, V * M * count + 1, dtype=np.float64).reshape((count, V, M))
    want = planar.transpose(1, 2, 0)                            # (V,M,count)
    (got,) = run(layout_exe, "transpose", V, M, count)
    assert np.array_equal(got, want.ravel(order="F"))


@pytest.mark.parametrize("EPB", [1, 7, 28, 256])
def test_block_count_is_the_written_formula(layout_exe, EPB):
    for ne in (0, 1, EPB - 1, EPB, EPB + 1, 8192 * EPB + 1):
        (got,) = run(layout_exe, "blocks", ne, EPB)
        assert got[0] == max(1, min((ne + EPB - 1) // EPB, 8192)), (ne, EPB)
    # the fields kernels' cap
    for n in (0, 256, 257, 4096 * 256, 4096 * 256 + 1):
        (got,) = run(layout_exe, "blocks", n, 256, 4096)
        assert got[0] == max(1, min((n + 255) // 256, 4096)), n


def test_usage_errors(layout_exe):
    for args in ((), ("pairs", "1", "2"), ("nothing", "1", "2", "3")):
        assert subprocess.run([layout_exe, *args], capture_output=True).returncode == 2
