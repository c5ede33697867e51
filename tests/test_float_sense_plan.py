"""The host statements of the float sets' sensors (h-numo_amd/csrc/float_plan.h) on the CPU: the slot rule
float_sense_slots against a brute-force statement, and float_sense_host -- the forming, grouping and summing text
float_sense_kernel runs, in passes of K element slots -- against the Python mirror HostFloats.sense.

tests/float_sense_main.cpp includes the header; this module compiles it once per session with AddressSanitizer
and UBSan (and -ffp-contract=off, as the engine is built) into a temporary directory and runs it as a child
process.  Nothing is loaded into Python.  The manner of tests/test_float_plan.py; every comparison is
np.array_equal."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import float_cases as FC
from hnumo import floats as FL
from hnumo import sample as S
from hnumo.vorticity import coriolis_of
from test_float_plan import full_dump, i32, read_dump, write_dump

HERE = os.path.dirname(os.path.abspath(__file__))
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="no g++ to compile tests/float_sense_main.cpp with")


@pytest.fixture(scope="session")
def sense_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("float_sense") / "float_sense_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(HERE, "float_sense_main.cpp"), "-o", exe], check=True)
    return exe


def run(exe, d, tmp):
    tmp = str(tmp)
    write_dump(os.path.join(tmp, "in.bin"), d)
    r = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return read_dump(os.path.join(tmp, "out.bin"))


# ------------------------------------------------------------------ the slot rule
def brute_slots(elem, block):
    """The rule as the issue states it, quadratic: per block, a float is a head when it is active and it is the
    first of the block, or the one before it is inactive, or the one before it is in another element; the slot of
    an active float is the number of heads up to and including it, minus 1."""
    elem = np.asarray(elem)
    slot = np.full(elem.size, -1, np.int32)
    nslots, lists = [], []
    for b0 in range(0, elem.size, block):
        e = elem[b0:b0 + block]
        act = e > 0
        head = [bool(act[t]) and (t == 0 or not act[t - 1] or e[t - 1] != e[t]) for t in range(e.size)]
        for t in range(e.size):
            if act[t]:
                slot[b0 + t] = sum(head[:t + 1]) - 1
        nslots.append(sum(head))
        lists += [int(e[t]) - 1 for t in range(e.size) if head[t]]
    return slot, np.array(nslots, np.int32), np.array(lists, np.int32)


def slot_inputs():
    rng = np.random.default_rng(5)
    out = {}
    for n in (1, 255, 256, 257, 700, 1031):                          # ragged last blocks
        e = rng.integers(1, 12, n)
        e[rng.random(n) < 0.25] = 0                                   # inactive floats interleaved
        out[f"random{n}"] = e
        out[f"runs{n}"] = np.repeat(rng.integers(0, 6, n), rng.integers(1, 9, n))[:n]
    out["all_inactive"] = np.zeros(600, int)
    out["negative_is_inactive"] = np.array([3, -1, 3, 0, 3])
    out["one_element"] = np.full(700, 38)
    out["all_distinct"] = np.arange(1, 601)
    out["sorted"] = np.sort(rng.integers(1, 40, 900))
    out["two_runs_of_one_element"] = np.array([4, 4, 7, 4, 4, 0, 4])
    return out


@pytest.mark.parametrize("key", list(slot_inputs()))
def test_slot_rule_against_brute_force(sense_exe, tmp_path, key):
    elem = slot_inputs()[key].astype(np.int32)
    for block in (256, 64, 7):
        t = run(sense_exe, {"slot_elems": elem, "block": i32(block)}, tmp_path)
        slot, nslots, lists = brute_slots(elem, block)
        assert np.array_equal(t["slot"], slot) and np.array_equal(t["nslots"], nslots) and np.array_equal(t["list"], lists)
        # what the kernel relies on: slots count up by at most one, an active float's slot names its own element
        off = np.concatenate([[0], np.cumsum(nslots)])
        for b, b0 in enumerate(range(0, elem.size, block)):
            sl, e = slot[b0:b0 + block], elem[b0:b0 + block]
            on = sl >= 0
            assert np.array_equal(on, e > 0) and (sl < nslots[b]).all()
            assert np.array_equal(lists[off[b]:off[b + 1]][sl[on]], e[on] - 1)
    if key == "two_runs_of_one_element":
        assert list(brute_slots(elem, 256)[2]) == [3, 6, 3, 3]       # formed again in every separate run
    if key == "all_inactive":
        assert not brute_slots(elem, 256)[1].any()


# ------------------------------------------------------------------ bit for bit against the mirror
def sense_dump(case, xy, layer, q, dts, mask, Ks, coriolis=True):
    A, Sc = case.arrays, case.scalars
    d = full_dump(case, xy, layer, q, dts)
    n = Sc["npoin"]
    flat = lambda k: np.asarray(A[k], np.float64).reshape(-1, order="F")[:n].copy()
    d.update({"zbot": flat("zbot_df"), "alpha": np.asarray(A["alpha"], np.float64).reshape(-1), "gravity": np.array([Sc["gravity"]]),
              "ksi_x": flat("ksi_x"), "ksi_y": flat("ksi_y"), "eta_x": flat("eta_x"), "eta_y": flat("eta_y"),
              "dpsi": np.ascontiguousarray(np.asarray(A["dpsi"], np.float64)).reshape(-1),
              "mask": i32(mask), "K": i32(*Ks)})
    if coriolis:
        d["f"] = np.asarray(coriolis_of(case), np.float64)
    return d


@pytest.mark.parametrize("mask", [1, 2, 3])
@pytest.mark.parametrize("name,kw", FC.CASES, ids=FC.IDS)
def test_host_evaluation_in_passes_equals_the_mirror(sense_exe, case_factory, tmp_path, name, kw, mask):
    """6 advances of 0.7 element on the moving state: after each, the S rows of every float from the host
    evaluation in passes of the kernel's K, of K = 1 and of a K no block exceeds equal HostFloats.sense."""
    case = FC.moving(case_factory, name, kw)
    xy, layer = FC.seeds(case)
    q = case.arrays["q_df"]
    dt = FC.big_dt(case, q)
    hf = FL.HostFloats(case, xy, layer, sensors=mask)
    want = []
    for _ in range(6):
        hf.advance(q, dt)
        hf.record()
        want.append(hf.sense(q))
    want = np.stack(want, axis=2)
    ser = hf.series()
    nS = FL.sense_rows(mask)
    assert ser.shape == (5 + nS, hf.M, 6) and np.array_equal(ser[5:], want)
    t = run(sense_exe, sense_dump(case, xy, layer, q, [dt] * 6, mask, [0, 1, 300]), tmp_path)
    hist = t["hist"].reshape(6, 5, hf.M).transpose(1, 2, 0)
    assert np.array_equal(hist, ser[:5])
    K = int(t["K0"][0])
    assert 1 <= K < 300 and t["K1"][0] == 1
    for i in range(3):
        got = t[f"sense{i}"].reshape(6, nS, hf.M).transpose(1, 2, 0)
        assert np.array_equal(got, want), (i, int((got != want).sum()))
    # the grouping was exercised: some block takes several passes at the kernel's K, inactive floats read 0.0
    el = t["elem_sorted"].reshape(6, hf.M)[-1]
    runs = max(FL.sense_slots(el[b:b + 256])[1].size for b in range(0, hf.M, 256))
    assert runs > K, (runs, K)
    off = ser[4] == 0
    assert off.any() and not want[:, off].any() and np.isfinite(want).all()
    if mask & 1:
        assert np.array_equal(want[1], ser[2]) and np.array_equal(want[2], ser[3])     # the record's own u, v
