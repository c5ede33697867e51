"""The host statement of the migrating float sets (h-numo_amd/csrc/float_plan.h: the side table xface, the
arrival table, float_advance<NGL, true>, float_resume, the outbox / arrive statements) on the CPU.

tests/float_migrate_main.cpp runs every rank of a partition in one process; this module compiles it once
per session with AddressSanitizer and UBSan (and -ffp-contract=off, as the engine is built) and runs it as a
child process.  Nothing is loaded into Python.  Every rank's every float equals the Python mirror
hnumo.floats.HostFloatGroup after every advance: np.array_equal."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import float_cases as FC
import float_migrate_cases as MC
from hnumo import floats as FL
from hnumo import sample as S
from hnumo.facepart import halo_lists
from test_float_plan import i32, read_dump, write_dump

HERE = os.path.dirname(os.path.abspath(__file__))
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="no g++ to compile tests/float_migrate_main.cpp with")
INVALID = 3
FIELDS = ("x", "y", "wx", "wy", "xi", "eta", "elem", "status")


@pytest.fixture(scope="session")
def migrate_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("float_migrate") / "float_migrate_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(HERE, "float_migrate_main.cpp"), "-o", exe], check=True)
    return exe


def run(exe, d, tmp):
    """(exit status, records) of one run; a sanitizer report fails the test."""
    tmp = str(tmp)
    write_dump(os.path.join(tmp, "in.bin"), d)
    r = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], capture_output=True, text=True)
    assert r.returncode in (0, INVALID) and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.returncode, read_dump(os.path.join(tmp, "out.bin"))


def group_dump(case, parts, xy=None, layer=None, dts=(), scale=0.0, tables_only=False):
    Sc = case.scalars
    d = {"nranks": i32(len(parts)), "ngl": i32(Sc["ngl"]), "nlayers": i32(Sc["nlayers"]), "ldc": i32(3), "xgl": S.case_xgl(case),
         "dts": np.asarray(dts, np.float64), "scale": np.array([scale]), "tables_only": i32(int(tables_only))}
    if xy is not None:
        d["xy"] = np.asfortranarray(xy, dtype=np.float64).reshape(-1, order="F")
        d["layer"] = np.asarray(layer, np.int32)
    for r, p in enumerate(parts):
        A, pre = p.arrays, f"r{r}."
        nbh_proc, num, lst, _ = halo_lists(p)
        d.update({pre + "nelem": i32(p.scalars["nelem"]), pre + "nface": i32(p.scalars["nface"]),
                  pre + "face": np.asarray(A["face"], np.int32).reshape(-1, order="F"),
                  pre + "imapl": np.asarray(A["imapl"], np.int32).reshape(-1, order="F"),
                  pre + "imapr": np.asarray(A["imapr"], np.int32).reshape(-1, order="F"),
                  pre + "coord": np.asarray(A["coord"], np.float64)[:3].reshape(-1, order="F"),
                  pre + "q": np.asarray(A["q_df"], np.float64).reshape(-1, order="F"),
                  pre + "nbh_proc": nbh_proc, pre + "num_send_recv": num, pre + "nbh_send_recv": lst})
    return d


@pytest.mark.parametrize("row", MC.ROWS + [MC.NGL8], ids=MC.ROW_IDS + ["dg25N7L3_3x3_2morton"])
def test_every_rank_equals_the_group_mirror_after_every_advance(migrate_exe, case_factory, tmp_path, row):
    run_ = MC.mirror_run(case_factory, row, scaled=True)
    case, parts, grp = run_["case"], run_["parts"], run_["group"]
    rc, t = run(migrate_exe, group_dump(case, parts, run_["xy"], run_["layer"], [run_["dt"]] * MC.NADV, run_["scale"]), tmp_path)
    assert rc == 0
    M = grp.M
    crossed = 0
    for r in range(len(parts)):
        hist = t[f"r{r}.hist"].reshape(MC.NADV, 8, M)
        for a in range(MC.NADV):
            want = run_["fields"][a][r]
            for v, k in enumerate(FIELDS):
                assert np.array_equal(hist[a, v], want[k].astype(np.float64)), (r, a, k, int((hist[a, v] != want[k]).sum()))
        assert np.array_equal(t[f"r{r}.xface"].reshape(-1, 4, 2), np.asarray(grp.ranks[r].xface, np.int32))
        assert list(t[f"r{r}.arrive"]) == [e for els in grp.arrive[r] for e in els]
    assert t["inflight"][0] == 0 and 1 <= t["rounds"].max() <= FL.MAXROUNDS and t["rounds"].max() == grp.max_rounds
    assert sum(len(c) for c in grp.crossings) > 0.05 * M
    assert np.array_equal(run_["merged"], run_["ref"])              # (the NGL = 8 case too: the single-rank bits)


@pytest.mark.parametrize("row", MC.ROWS, ids=MC.ROW_IDS)
def test_side_and_arrival_tables_from_the_corner_coordinates(migrate_exe, case_factory, tmp_path, row):
    """xface and arrive against a construction that knows nothing of faces: the two elements, one on each rank,
    that hold both corner points of a side."""
    case, parts = MC.partition(case_factory, row)
    rc, t = run(migrate_exe, group_dump(case, parts, tables_only=True), tmp_path)
    assert rc == 0
    corners = [FC.corners_of(p) for p in parts]
    h = np.sqrt(((np.roll(corners[0], -1, axis=1) - corners[0]) ** 2).sum(axis=2)).min()
    side_corners = [(3, 0), (1, 2), (0, 1), (2, 3)]                 # xi=-1, xi=+1, eta=-1, eta=+1

    def holders(cc, a, b):                                          # elements of cc with corners at both a and b
        at = lambda p: (np.abs(cc - p[None, None, :]).sum(axis=2) < 1e-6 * h).any(axis=1)
        return np.nonzero(at(a) & at(b))[0]
    nfaces = 0
    for r, p in enumerate(parts):
        xface = t[f"r{r}.xface"].reshape(-1, 4, 2)
        nbr = t[f"r{r}.nbr"].reshape(-1, 4)
        ranks = [nb.rank for nb in p.fneighbours]
        off = np.concatenate([[0], np.cumsum([nb.faces.size for nb in p.fneighbours])])
        arrive = t[f"r{r}.arrive"]
        assert arrive.size == off[-1]
        seen = set()
        for e in range(xface.shape[0]):
            for s, (ia, ib) in enumerate(side_corners):
                a, b = corners[r][e, ia], corners[r][e, ib]
                across = [(q, holders(corners[q], a, b)) for q in range(len(parts)) if q != r]
                across = [(q, els) for q, els in across if els.size]
                k, pos = xface[e, s]
                if not across:
                    assert k == -1 and pos == -1 and nbr[e, s] != FL.OFF_RANK
                    continue
                (q, els), = across
                assert els.size == 1 and nbr[e, s] == FL.OFF_RANK
                assert ranks[k] == q and 0 <= pos < p.fneighbours[k].faces.size
                assert arrive[off[k] + pos] == e                   # my own end of the face
                # the neighbour's end: its table at (its index for me, the same pos)
                pq = parts[q]
                kq = [nb.rank for nb in pq.fneighbours].index(r)
                offq = np.concatenate([[0], np.cumsum([nb.faces.size for nb in pq.fneighbours])])
                assert t[f"r{q}.arrive"][offq[kq] + pos] == els[0]
                seen.add((int(k), int(pos)))
                nfaces += 1
        assert len(seen) == off[-1]                                 # every listed face is some side
    assert nfaces > 0 and nfaces % 2 == 0


def _set(k, v):
    def f(d):
        d[k] = v
    return f


def _at(k, i, v):
    def f(d):
        a = d[k].copy()
        a[i] = v
        d[k] = a
    return f


def _drop(k):
    def f(d):
        del d[k]
    return f


def _interior_face(d):
    face = d["r0.face"].reshape(8, -1, order="F")
    f = int(np.nonzero(face[7] > 0)[0][0])
    _at("r0.nbh_send_recv", 1, f + 1)(d)


def _wall_face(d):
    face = d["r0.face"].reshape(8, -1, order="F")
    f = int(np.nonzero(face[7] < 0)[0][0])
    _at("r0.nbh_send_recv", 0, f + 1)(d)


def _twice(d):
    _at("r0.nbh_send_recv", 2, d["r0.nbh_send_recv"][1])(d)


REJECT = {
    "num_send_recv NULL": (_drop("r0.num_send_recv"), "num_send_recv or nbh_send_recv is NULL"),
    "nbh_send_recv NULL": (_drop("r0.nbh_send_recv"), "num_send_recv or nbh_send_recv is NULL"),
    "num_send_recv < 0": (_at("r0.num_send_recv", 0, -1), "num_send_recv(1) < 0"),
    "face 0": (_at("r0.nbh_send_recv", 0, 0), "is out of range"),
    "face above nface": (_at("r0.nbh_send_recv", 1, 10 ** 6), "is out of range"),
    "an interior face": (_interior_face, "is not a processor face"),
    "a wall face": (_wall_face, "is not a processor face"),
    "a face listed twice": (_twice, "lies on a side that is listed already"),
}


@pytest.mark.parametrize("what", list(REJECT))
def test_rejected(migrate_exe, case_factory, tmp_path, what):
    case, parts = MC.partition(case_factory, MC.ROWS[0])
    d = group_dump(case, parts, tables_only=True)
    rc, t = run(migrate_exe, d, tmp_path)
    assert rc == 0 and (t["r0.xface"] >= 0).any()
    mutate, text = REJECT[what]
    mutate(d)
    rc, t = run(migrate_exe, d, tmp_path)
    assert rc == INVALID
    msg = t["error"].tobytes().rstrip(b"\0").decode()
    assert text in msg and msg.startswith("hnumo_floats_migrate"), msg
