"""The host statement of the float sets (h-numo_amd/csrc/float_plan.h) on the CPU: the side tables,
validation, seeding, and float_vel / float_locate / float_advance -- the text the kernel runs.

tests/float_plan_main.cpp includes the header; this module compiles it once per session with
AddressSanitizer and UBSan (and -ffp-contract=off, as the engine is built) into a temporary directory
and runs it as a child process on dumps of the mesh tables, the seeds and the states (the record
format is private to the two files).  Nothing is loaded into Python.  Comparisons with the Python
mirror hnumo.floats.HostFloats are np.array_equal; the analytic cases carry their own bounds."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import float_cases as FC
from hnumo import floats as FL
from hnumo import sample as S

HERE = os.path.dirname(os.path.abspath(__file__))
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="no g++ to compile tests/float_plan_main.cpp with")

INVALID = 3  # exit status of float_plan_main for HNUMO_ERR_INVALID
EPS = 2.0 ** -52


@pytest.fixture(scope="session")
def float_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("float_plan") / "float_plan_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(HERE, "float_plan_main.cpp"), "-o", exe], check=True)
    return exe


def write_dump(path, d):
    with open(path, "wb") as f:
        for k, v in d.items():
            v = np.ascontiguousarray(v)
            assert v.dtype in (np.int32, np.float64), (k, v.dtype)
            f.write(struct.pack("<i", len(k)) + k.encode() + (b"i" if v.dtype == np.int32 else b"d"))
            f.write(struct.pack("<q", v.size) + v.tobytes())


def read_dump(path):
    out = {}
    with open(path, "rb") as f:
        b = f.read()
    o = 0
    while o < len(b):
        (nl,) = struct.unpack_from("<i", b, o)
        k = b[o + 4:o + 4 + nl].decode()
        t = b[o + 4 + nl:o + 5 + nl]
        (n,) = struct.unpack_from("<q", b, o + 5 + nl)
        o += 13 + nl
        dt, sz = (np.int32, 4) if t == b"i" else (np.float64, 8)
        out[k] = np.frombuffer(b, dt, n, o).copy()
        o += n * sz
    return out


def run(exe, d, tmp):
    """(exit status, records) of one run; a sanitizer report fails the test."""
    tmp = str(tmp)
    write_dump(os.path.join(tmp, "in.bin"), d)
    r = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], capture_output=True, text=True)
    assert r.returncode in (0, INVALID) and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.returncode, read_dump(os.path.join(tmp, "out.bin"))


def i32(*v):
    return np.array(v, np.int32)


def mesh_dump(case):
    A, Sc = case.arrays, case.scalars
    return {"ngl": i32(Sc["ngl"]), "nelem": i32(Sc["nelem"]), "nelem_owned": i32(S.owned_elements(case)),
            "nlayers": i32(Sc["nlayers"]), "nface": i32(Sc["nface"]),
            "face": np.asarray(A["face"], np.int32).reshape(-1, order="F"),
            "imapl": np.asarray(A["imapl"], np.int32).reshape(-1, order="F"),
            "imapr": np.asarray(A["imapr"], np.int32).reshape(-1, order="F")}


def full_dump(case, xy, layer, q=None, dts=(), ldc=3):
    d = mesh_dump(case)
    d.update({"coord": np.asarray(case.arrays["coord"], np.float64)[:ldc].reshape(-1, order="F"), "ldc": i32(ldc),
              "xgl": S.case_xgl(case), "xy": np.asfortranarray(xy, dtype=np.float64).reshape(-1, order="F"),
              "layer": np.asarray(layer, np.int32), "dts": np.asarray(dts, np.float64)})
    if q is not None:
        d["q"] = np.asarray(q, np.float64).reshape(-1, order="F")
    return d


def hist_of(t, M):
    n = t["hist"].size // (5 * M)
    return t["hist"].reshape(n, 5, M).transpose(1, 2, 0)


# ------------------------------------------------------------------ side tables
def brute_sides(case, whole):
    """Side neighbours of `case`'s owned elements from the corner coordinates alone: the neighbour
    across a side is the other owned element with both of the side's corner points; a side without one
    is off-rank when the whole mesh `whole` has an element there, a wall otherwise."""
    def corners(c):
        n, ne = c.scalars["ngl"], c.scalars["nelem"]
        cn = np.array([0, n - 1, n * n - 1, n * (n - 1)])
        return np.asarray(c.arrays["coord"])[0:2, (np.arange(ne) * n * n)[:, None] + cn[None, :]].transpose(1, 2, 0)
    c, cw = corners(case), corners(whole)
    ne = S.owned_elements(case)
    h = np.sqrt(((np.roll(cw, -1, axis=1) - cw) ** 2).sum(axis=2)).min()
    side_corners = [(3, 0), (1, 2), (0, 1), (2, 3)]              # xi=-1, xi=+1, eta=-1, eta=+1

    def holders(cc, p):                                          # elements of cc with a corner at p
        return set(np.nonzero((np.abs(cc - p[None, None, :]).sum(axis=2) < 1e-6 * h).any(axis=1))[0].tolist())
    nbr = np.zeros((ne, 4), np.int32)
    for e in range(ne):
        for s, (a, b) in enumerate(side_corners):
            mine = (holders(c[:ne], c[e, a]) & holders(c[:ne], c[e, b])) - {e}
            assert len(mine) <= 1
            if mine:
                nbr[e, s] = mine.pop()
            else:
                there = holders(cw, c[e, a]) & holders(cw, c[e, b])
                nbr[e, s] = FL.OFF_RANK if len(there) == 2 else FL.WALL
                assert len(there) in (1, 2)
    return nbr


def check_sides(nbr):
    ne = nbr.shape[0]
    opposite = [1, 0, 3, 2]
    for e in range(ne):
        for s in range(4):
            n = nbr[e, s]
            assert -2 <= n < ne and n != e
            if n >= 0:
                assert e in nbr[n]                              # every interior side is mutual
    return opposite


@pytest.mark.parametrize("key", ["brick", "qmbump8", "face_rank0", "face_rank1", "ghost_rank1"])
def test_side_tables(float_exe, case_factory, tmp_path, key):
    whole = case_factory("qmbump8") if key == "qmbump8" else case_factory("dg25L3", nelx=5, nely=3) if key == "brick" else case_factory("bump10")
    case = whole
    if key.startswith("face"):
        from hnumo.facepart import face_partition
        case = face_partition(whole, 2, int(key[-1]), "block")
    elif key.startswith("ghost"):
        from hnumo.partition import partition
        case = partition(whole, 2, 1)
        assert 0 < case.nelem_owned < case.scalars["nelem"]
    d = mesh_dump(case)
    d["sides_only"] = i32(1)
    rc, t = run(float_exe, d, tmp_path)
    assert rc == 0
    nbr = t["nbr"].reshape(-1, 4)
    want = brute_sides(case, whole)
    assert np.array_equal(nbr, want), int((nbr != want).sum())
    assert np.array_equal(nbr, FL.side_neighbours(case))        # the mirror's own construction
    check_sides(nbr)
    assert (nbr == FL.WALL).any() and (nbr >= 0).any()
    assert (nbr == FL.OFF_RANK).any() == (case is not whole)
    if key == "qmbump8":
        # mixed orientation: some neighbours meet on sides that are not opposite ones
        back = np.array([[list(nbr[n]).index(e) if n >= 0 else -1 for n in nbr[e]] for e in range(nbr.shape[0])])
        opp = np.array([1, 0, 3, 2])[None, :]
        assert ((back != opp) & (nbr >= 0)).any()


# ------------------------------------------------------------------ bit for bit against the mirror
@pytest.mark.parametrize("name,kw", FC.CASES, ids=FC.IDS)
def test_advance_equals_the_mirror(float_exe, case_factory, tmp_path, name, kw):
    """6 advances on the moving state, the fastest float moving 0.7 of an element per advance: every
    field of every float, and the record after every advance, equal HostFloats."""
    case = FC.moving(case_factory, name, kw)
    xy, layer = FC.seeds(case)
    q = case.arrays["q_df"]
    dt = FC.big_dt(case, q)
    hf = FL.HostFloats(case, xy, layer)
    e0 = hf.elem.copy()
    want, stats = FC.run_mirror(hf, [(q, dt)] * 6)
    FC.check_conditions(hf, stats)
    rc, t = run(float_exe, full_dump(case, xy, layer, q, [dt] * 6), tmp_path)
    assert rc == 0
    assert np.array_equal(t["nbr"].reshape(-1, 4), hf.nbr) and np.array_equal(t["tol"], hf.tol)
    assert np.array_equal(t["corners"].reshape(-1, 8), hf.corners) and t["maxc"][0] == hf.maxc
    assert np.array_equal(t["elem0"], e0) and np.array_equal(t["status0"], np.where(e0 > 0, FL.ACTIVE, FL.LEFT))
    # sorted stably by the initial element; the permutation goes back to input order
    perm = t["perm"]
    assert np.array_equal(np.sort(perm), np.arange(hf.M)) and (np.diff(e0[perm]) >= 0).all()
    assert (np.diff(perm)[np.diff(e0[perm]) == 0] > 0).all()
    g = hf.get()
    for k, a in (("x", g["x"]), ("y", g["y"]), ("wx", g["u"]), ("wy", g["v"]), ("elem", g["elem"]), ("status", g["status"]),
                 ("xi", hf.xi), ("eta", hf.eta), ("fresh", hf.fresh), ("layer", hf.layer)):
        assert np.array_equal(t[k], a), (k, int((t[k] != a).sum()))
    assert np.array_equal(hist_of(t, hf.M), want)
    assert np.isfinite(want).all()


# ------------------------------------------------------------------ analytic cases
def hand_state(case, u, v):
    """q_df with thickness 1 and the nodal velocities u, v (npoin) in every layer."""
    q = np.zeros((3, case.scalars["npoin"], case.scalars["nlayers"]), order="F")
    q[0] = 1.0
    q[1] = np.asarray(u)[:, None]
    q[2] = np.asarray(v)[:, None]
    return q


def test_solid_body_rotation(float_exe, case_factory, tmp_path):
    """q1 = 1 and linear q2, q3 on a 6x6 N=4 brick: the interpolant is exact, and Heun's step on a
    rotation by theta = Omega dt multiplies every radius by sqrt(1 + theta^4/4).  theta = 0.2, 40
    advances (more than a revolution): every radius is r0 (1 + theta^4/4)^(n/2) to 1e-10."""
    case = case_factory("dg25L3", nelx=6, nely=6)
    assert case.scalars["ngl"] == 5 and case.scalars["nelem"] == 36
    x, y = np.asarray(case.arrays["coord"])[0], np.asarray(case.arrays["coord"])[1]
    xc, yc = 0.5 * (x.min() + x.max()), 0.5 * (y.min() + y.max())
    h = min(x.max() - x.min(), y.max() - y.min()) / 6
    om, theta, n = 1.0e-5, 0.2, 40
    q = hand_state(case, -om * (y - yc), om * (x - xc))
    radii = np.array([0.6, 1.1, 1.55, 2.05, 2.45]) * h
    xy = np.concatenate([FL.seed_ring((xc, yc), r, 8, phase=0.1 * i) for i, r in enumerate(radii)], axis=1)
    M = xy.shape[1]
    rc, t = run(float_exe, full_dump(case, xy, np.ones(M, np.int32), q, [theta / om] * n), tmp_path)
    assert rc == 0 and (t["status"] == FL.ACTIVE).all()
    hist = hist_of(t, M)
    r0 = np.repeat(radii, 8)
    for i in (0, n // 2 - 1, n - 1):
        r = np.hypot(hist[0, :, i] - xc, hist[1, :, i] - yc)
        want = r0 * (1.0 + theta ** 4 / 4.0) ** ((i + 1) / 2.0)
        assert np.abs(r / want - 1.0).max() <= 1e-10, (i, float(np.abs(r / want - 1.0).max()))
    # the stored velocity is the field at the float
    assert np.abs(hist[2, :, -1] + om * (hist[1, :, -1] - yc)).max() <= 1e-10 * om * r0.max()
    for m in range(0, M, 8):
        assert np.unique(hist[4, m]).size >= (8 if r0[m] > h else 4), (m, np.unique(hist[4, m]))
    ang = np.unwrap(np.arctan2(hist[1, 0] - yc, hist[0, 0] - xc))
    assert ang[-1] - ang[0] > 2 * np.pi * 1.15                 # n atan(theta (1 - ..)) ~ 7.8 rad


def test_uniform_flow_into_the_east_wall(float_exe, case_factory, tmp_path):
    """x ends within 64 eps max|coord| of the wall and stays there; y keeps moving with v."""
    case = case_factory("dg25L3", nelx=5, nely=3)
    c = np.asarray(case.arrays["coord"])
    xw, x0 = c[0].max(), c[0].min()
    h = (xw - x0) / 5
    ylo, yhi = c[1].min(), c[1].max()
    U, V, dt, n = 2.0, 0.25, 0.3 * h / 2.0, 12
    q = hand_state(case, np.full(c.shape[1], U), np.full(c.shape[1], V))
    xs = xw - h * np.array([0.05, 0.45, 1.2, 2.6])
    ys = ylo + (yhi - ylo) * np.array([0.1, 0.3, 0.5])
    xy = np.array([[a, b] for a in xs for b in ys]).T
    M = xy.shape[1]
    assert ys.max() + n * dt * V < yhi - 0.1 * (yhi - ylo)        # no float meets the north wall
    rc, t = run(float_exe, full_dump(case, xy, np.full(M, 2, np.int32), q, [dt] * n), tmp_path)
    assert rc == 0 and (t["status"] == FL.ACTIVE).all()
    hist = hist_of(t, M)
    bound = 64 * EPS * np.abs(c[0:2]).max()
    free = np.minimum(xy[0][:, None] + dt * U * np.arange(1, n + 1)[None, :], xw)
    assert np.abs(hist[0] - free).max() <= bound + 1e-12 * xw
    at_wall = xy[0][:, None] + dt * U * np.arange(1, n + 1)[None, :] > xw
    assert at_wall[:, -1].all() and not at_wall[:, 0].all()
    assert np.abs(hist[0][at_wall] - xw).max() <= bound            # at the wall, and it stays there
    yw = xy[1][:, None] + dt * V * np.arange(1, n + 1)[None, :]
    assert np.abs(hist[1] - yw).max() <= 1e-10 * (yhi - ylo)        # y keeps moving with v
    # (the weights of a point sum to 1 within 4 ngl^2 eps: tests/test_sample_cpu.py)
    assert np.abs(hist[2] / U - 1.0).max() <= 100 * EPS and np.abs(hist[3] / V - 1.0).max() <= 100 * EPS


def test_bounded_outcomes(float_exe, case_factory, tmp_path):
    """A displacement across five element boundaries ends LOST where four do not; a non-finite
    velocity ends LOST; both runs return."""
    case = case_factory("bump10", nop=2)                            # 10 x 10 elements
    c = np.asarray(case.arrays["coord"])
    npoin = c.shape[1]
    h = (c[0].max() - c[0].min()) / 10
    y = c[1].min() + 4.5 * h
    xy = np.array([[c[0].min() + 0.5 * h, y], [c[0].min() + 0.5 * h, y], [c[0].min() + 2.5 * h, y]]).T
    q = hand_state(case, np.full(npoin, 1.0), np.zeros(npoin))
    # the predictor of float 0 crosses 4 boundaries, that of float 1 (next run) 5
    rc, t = run(float_exe, full_dump(case, xy, i32(1, 1, 2), q, [4.0 * h]), tmp_path)
    assert rc == 0 and list(t["status"]) == [FL.ACTIVE] * 3
    assert np.abs(t["x"] - (xy[0] + 4.0 * h)).max() <= 1e-9 * h and list(t["elem"]) == [45, 45, 47]
    rc, t = run(float_exe, full_dump(case, xy, i32(1, 1, 2), q, [5.0 * h]), tmp_path)
    assert rc == 0 and list(t["status"]) == [FL.LOST, FL.LOST, FL.LOST]
    assert not t["elem"].any() and not t["wx"].any() and np.abs(t["x"] - (xy[0] + 5.0 * h)).max() <= 1e-9 * h
    hf = FL.HostFloats(case, xy, i32(1, 1, 2))
    hf.advance(q, 5.0 * h)
    assert np.array_equal(hf.status, t["status"]) and np.array_equal(hf.x, t["x"])
    # a node without thickness under float 2 (layer 2): 0/0; an infinite momentum under float 0
    for bad, who in ((np.nan, 2), (np.inf, 0)):
        q2 = q.copy(order="F")
        e = int(FL.HostFloats(case, xy, i32(1, 1, 2)).elem[who]) - 1
        if np.isnan(bad):
            q2[:, e * 9 + 4, 1] = 0.0
        else:
            q2[1, e * 9 + 4, 0] = np.inf
        rc, t = run(float_exe, full_dump(case, xy, i32(1, 1, 2), q2, [0.1 * h, 0.1 * h]), tmp_path)
        assert rc == 0
        want = [FL.ACTIVE] * 3
        want[who] = FL.LOST
        if who == 0:
            want[1] = FL.LOST                                       # (float 1 is float 0's twin)
        assert list(t["status"]) == want
        lost = np.array(want) == FL.LOST
        assert not t["elem"][lost].any() and not t["wx"][lost].any() and np.isfinite(t["x"]).all()
        assert np.array_equal(t["x"][lost], xy[0][lost])            # lost at the fresh evaluation: where it was
        hf2 = FL.HostFloats(case, xy, i32(1, 1, 2))
        for _ in range(2):
            hf2.advance(q2, 0.1 * h)
        for k, a in (("x", hf2.x), ("y", hf2.y), ("wx", hf2.wx), ("status", hf2.status), ("elem", hf2.elem)):
            assert np.array_equal(t[k], a), k


def test_zero_dt_keeps_the_position(float_exe, case_factory, tmp_path):
    name, kw = FC.CASES[2]
    case = FC.moving(case_factory, name, kw)
    xy, layer = FC.seeds(case)
    rc, t = run(float_exe, full_dump(case, xy, layer, case.arrays["q_df"], [0.0, 0.0]), tmp_path)
    assert rc == 0
    on = t["elem0"] > 0
    assert np.array_equal(t["x"], xy[0]) and np.array_equal(t["y"], xy[1])
    assert np.array_equal(t["elem"], t["elem0"]) and (t["wx"][on] != 0).any() and not t["fresh"][on].any()


# ------------------------------------------------------------------ validation
def _drop(k):
    def f(d):
        del d[k]
    return f


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


def _two_faces_on_a_side(d):
    # face 2's left element lists face 1's nodes: two faces on one side, and a side without a face
    m = d["imapl"].reshape(3, 3, -1, order="F").copy(order="F")
    f1 = int(np.nonzero(d["face"].reshape(8, -1, order="F")[6] == 1)[0][0])
    f2 = int(np.nonzero(d["face"].reshape(8, -1, order="F")[6] == 1)[0][1])
    m[:, :, f2] = m[:, :, f1]
    d["imapl"] = m.reshape(-1, order="F")


def _no_side(d):
    m = d["imapl"].reshape(3, 3, -1, order="F").copy(order="F")
    m[0, :, 0], m[1, :, 0] = [1, 2, 3], [1, 2, 3]               # a diagonal: no side of the element
    d["imapl"] = m.reshape(-1, order="F")


def _missing_face(d):
    f = d["face"].reshape(8, -1, order="F")[:, 1:].copy(order="F")
    d["face"], d["nface"] = f.reshape(-1, order="F"), i32(f.shape[1])
    d["imapl"] = d["imapl"].reshape(3, 3, -1, order="F")[:, :, 1:].reshape(-1, order="F")
    d["imapr"] = d["imapr"].reshape(3, 3, -1, order="F")[:, :, 1:].reshape(-1, order="F")


def _coord(i, j, v):
    def f(d):
        c = d["coord"].reshape(3, -1, order="F").copy(order="F")
        c[i, j] = v(c) if callable(v) else v
        d["coord"] = c.reshape(-1, order="F")
    return f


def _collapse(d):
    c = d["coord"].reshape(3, -1, order="F").copy(order="F")
    c[:, 18:21] = c[:, 18:19]                                       # element 3's bottom edge: length 0
    d["coord"] = c.reshape(-1, order="F")


REJECT = {
    "face NULL": (_drop("face"), "face, imapl or imapr is NULL"),
    "imapr NULL": (_drop("imapr"), "face, imapl or imapr is NULL"),
    "nelem_owned above nelem": (_set("nelem_owned", i32(101)), "nelem_owned in 0..nelem"),
    "face(7) 0": (_at("face", 6, 0), "out of range"),
    "face(8) above nelem": (_at("face", 8 + 7, 101), "out of range"),
    "nodes on no side": (_no_side, "are not one side of element"),
    "two faces on a side": (_two_faces_on_a_side, "two faces on one side"),
    "a side without a face": (_missing_face, "has a side without a face"),
    "coord NULL": (_drop("coord"), "coord is NULL"),
    "ldc 4": (_set("ldc", i32(4)), "ldc must be 2 or 3"),
    "xgl NULL": (_drop("xgl"), "xgl is NULL"),
    "xgl not ascending": (_at("xgl", 1, -1.0), "ascend strictly"),
    "coord NaN": (_coord(0, 7, np.nan), "coord is not finite"),
    "edge of length 0": (_collapse, "has an edge of length 0"),
    "curved element": (_coord(0, 2 * 9 + 4, lambda c: c[0, 2 * 9 + 4] + 1e-3 * (c[0, 2 * 9 + 2] - c[0, 2 * 9])), "not the bilinear map"),
    "xy NULL": (_drop("xy"), "xy is NULL"),
    "layer NULL": (_drop("layer"), "layer is NULL"),
    "M 0": (_set("M", i32(0)), "M must be >= 1"),
    "M -1": (_set("M", i32(-1)), "M must be >= 1"),
    "layer 0": (_at("layer", 1, 0), "is outside 1.."),
    "layer above nlayers": (_at("layer", 2, 3), "is outside 1.."),
}


@pytest.mark.parametrize("what", list(REJECT))
def test_rejected(float_exe, case_factory, tmp_path, what):
    case = case_factory("bump10", nop=2)
    xy = FL.seed_grid(case, 2, 2)
    d = full_dump(case, xy, i32(1, 2, 1, 2))
    d["M"] = i32(4)
    rc, t = run(float_exe, d, tmp_path)
    assert rc == 0 and (t["elem0"] > 0).all()
    mutate, text = REJECT[what]
    mutate(d)
    rc, t = run(float_exe, d, tmp_path)
    assert rc == INVALID
    msg = t["error"].tobytes().rstrip(b"\0").decode()
    assert text in msg, msg


def test_unsupported_ngl_is_rejected(float_exe, case_factory, tmp_path):
    case = case_factory("bump10", nop=6)                            # ngl = 7: no kernel
    assert case.scalars["ngl"] == 7
    rc, t = run(float_exe, full_dump(case, FL.seed_grid(case, 2, 2), i32(1, 1, 1, 1)), tmp_path)
    assert rc == INVALID and "unsupported ngl" in t["error"].tobytes().decode()
