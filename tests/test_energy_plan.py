"""The host statements of the energy budget (h-numo_amd/csrc/energy_plan.h) on the CPU: energy_host -- the node
and quad functions energy_sample_kernel calls, looped over the elements in the kernel's phases -- against the
Python mirror hnumo.energy.HostEnergy.

tests/energy_main.cpp includes the header; this module compiles it once per session with AddressSanitizer and
UBSan (and -ffp-contract=off, as the engine is built) into a temporary directory and runs it as a child process.
Nothing is loaded into Python.  The manner of tests/test_float_sense_plan.py; every comparison is
np.array_equal."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import states
from hnumo import covariance as CV
from hnumo import energy as EN
from hnumo import sample as S
from test_float_plan import i32, read_dump, write_dump

HERE = os.path.dirname(os.path.abspath(__file__))
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="no g++ to compile tests/energy_main.cpp with")

# nop=2 6x6 L=2 with the quadratic drag; dg25L3 4x4 (botfr = 1, viscosity 50, wind); N=7; warped quadrilaterals
# (amplitudes halved as tests/test_cov_gpu.py does); one layer
CASES = [("bump10", {"nop": 2, "nelx": 6, "nely": 6, "botfr": 2, "cd": 1e-3}), ("dg25L3", {"nelx": 4, "nely": 4}),
         ("dg25N7L3", {"nelx": 3, "nely": 3}), ("qmbump8", {}), ("lake10", {"nop": 2, "nelx": 4, "nely": 4, "nlayers": 1})]
IDS = ["N2-L2-botfr2", "dg25L3", "dg25N7L3", "qmbump8", "one-layer"]
STATE = {"qmbump8": dict(amp=0.005, fr=0.001, jump=0.005)}


@pytest.fixture(scope="session")
def energy_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("energy") / "energy_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(HERE, "energy_main.cpp"), "-o", exe], check=True)
    return exe


def run(exe, d, tmp, status=0):
    tmp = str(tmp)
    write_dump(os.path.join(tmp, "in.bin"), d)
    r = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], capture_output=True, text=True)
    assert r.returncode == status and not r.stderr, (r.returncode, r.stderr[-2000:])
    return read_dump(os.path.join(tmp, "out.bin"))


def energy_dump(case, qs, taus, zref, series=True):
    A, Sc = case.arrays, case.scalars
    n = Sc["npoin"]
    flat = lambda k: np.asarray(A[k], np.float64).reshape(-1, order="F")[:n].copy()
    d = {"ngl": i32(Sc["ngl"]), "nelem_owned": i32(S.owned_elements(case)), "nlayers": i32(Sc["nlayers"]),
         "botfr": i32(Sc["botfr"]), "npoin": i32(n), "npoin_q": i32(Sc["npoin_q"]), "series": i32(int(series)),
         "gravity": np.array([Sc["gravity"]]), "cd": np.array([Sc["cd"]]), "visc": np.array([Sc["visc"]]),
         "alpha": np.asarray(A["alpha"], np.float64).reshape(-1)[:Sc["nlayers"]].copy(), "zbot": flat("zbot_df"),
         "ksi_x": flat("ksi_x"), "ksi_y": flat("ksi_y"), "eta_x": flat("eta_x"), "eta_y": flat("eta_y"), "jac": flat("jac"),
         "wjac": np.asarray(A["jacq"], np.float64).reshape(-1, order="F").copy(),
         "dpsi": np.ascontiguousarray(np.asarray(A["dpsi"], np.float64)).reshape(-1),
         "psiq": np.ascontiguousarray(np.asarray(A["psiq"], np.float64)).reshape(-1),
         "q": np.concatenate([np.asarray(q, np.float64).reshape(-1, order="F") for q in qs]),
         "tau": np.concatenate([np.asarray(t, np.float64).reshape(-1, order="F") for t in taus])}
    if zref is not None:
        d["zref"] = np.asarray(zref, np.float64).reshape(-1, order="F")
    return d


def inputs(case_factory, name, kw):
    """(case, two moving states of it, two winds -- the case's own plus a seeded random one, and a random one)"""
    rest = case_factory(name, **kw)
    p = {**states.DEFAULT, **STATE.get(name, {})}
    qs = [states.moving_state(rest, **p)[0], states.moving_state(rest, amp=0.7 * p["amp"], fr=1.3 * p["fr"], jump=0.5 * p["jump"])[0]]
    rng = np.random.default_rng(11)
    t0 = np.asarray(rest.arrays["tau_wind"], np.float64)
    taus = [np.asfortranarray(t0 + rng.uniform(-0.05, 0.05, t0.shape)), np.asfortranarray(rng.uniform(-0.05, 0.05, t0.shape))]
    return rest, qs, taus


@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
@pytest.mark.parametrize("ref", [True, False], ids=["zref", "nozref"])
def test_host_loop_equals_the_mirror(energy_exe, case_factory, tmp_path, name, kw, ref):
    case, qs, taus = inputs(case_factory, name, kw)
    Sc = case.scalars
    L, ne = Sc["nlayers"], Sc["nelem"]
    zref = CV.rest_elevations(case) if ref else None
    he = EN.HostEnergy(case, zref=zref)
    for q, t in zip(qs, taus):
        he.add(q, t)
    t = run(energy_exe, energy_dump(case, qs, taus, zref), tmp_path)
    quad, nodal, _ = he.sums()
    assert np.array_equal(t["quad"].reshape(quad.shape, order="F"), quad)
    assert np.array_equal(t["nodal"].reshape(nodal.shape, order="F"), nodal)
    rows = t["rows"].reshape(3 * L + 2, 2, order="F")
    want = he.series()
    for r, nm in enumerate(EN.series_names(L)):
        assert np.array_equal(rows[r], want[r]), (nm, rows[r], want[r])
    assert np.array_equal(t["part"].reshape(3 * L + 2, ne), he.partials)
    # the case exercises what it is here for
    assert quad[0].any() and np.isfinite(rows).all() and (rows[:L] > 0).all()
    assert bool(quad[1].any()) == (Sc["botfr"] != 0 and Sc["cd"] != 0) and bool(nodal.any()) == (Sc["visc"] != 0)
    assert (rows[L:2 * L] > 0).all()


def test_sums_only_and_rejected_input(energy_exe, case_factory, tmp_path):
    case, qs, taus = inputs(case_factory, *CASES[0])
    he = EN.HostEnergy(case, series=False)
    for q, t in zip(qs, taus):
        he.add(q, t)
    t = run(energy_exe, energy_dump(case, qs, taus, None, series=False), tmp_path)
    assert set(t) == {"quad", "nodal"}
    assert np.array_equal(t["quad"].reshape(he.sums()[0].shape, order="F"), he.sums()[0])
    d = energy_dump(case, qs, taus, None)
    d["tau"] = d["tau"][:-1]
    run(energy_exe, d, tmp_path, status=3)
    d = energy_dump(case, qs, taus, None)
    d["ngl"] = i32(7)                                                       # no such instantiation
    run(energy_exe, d, tmp_path, status=3)
