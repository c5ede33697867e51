"""The host-only plan of a sample set (h-numo_amd/csrc/sample_plan.h): locating physical points in
the owned elements, the caller-supplied form, validation, and the kernel's work lists, run on the
CPU.

tests/sample_plan_main.cpp includes the header; this module compiles it once per session with
AddressSanitizer and UBSan into a temporary directory and runs it as a child process on dumps of
coord / xgl / points (the record format is private to the two files).  Nothing is loaded into
Python.  Expectations are built in numpy from the grids themselves: points by the forward bilinear
map of known (element, xi0, eta0), cells from the corner nodes.

Bounds: tol_e = 64 eps max|coord| / (half the element's shortest edge) in
reference coordinates -- on the warped grid divided by the sine of the element's smallest corner
angle, the conditioning of its map -- and 64 eps max|coord| in physical coordinates."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="no g++ to compile tests/sample_plan_main.cpp with")

INVALID = 3  # exit status of sample_plan_main for HNUMO_ERR_INVALID
EPS = 2.0 ** -52


@pytest.fixture(scope="session")
def sample_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sample_plan") / "sample_plan_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "sample_plan_main.cpp"), "-o", exe], check=True)
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


class Grid:
    """A case's owned elements as the plan sees them."""

    def __init__(self, case):
        from hnumo import sample as S
        self.case = case
        self.ngl, self.L = case.scalars["ngl"], case.scalars["nlayers"]
        self.P = self.ngl ** 2
        self.ne = S.owned_elements(case)
        self.nall = case.scalars["nelem"]
        self.coord = np.asfortranarray(case.arrays["coord"], dtype=np.float64)
        self.xgl = S.case_xgl(case)
        n = self.ngl
        cn = np.array([0, n - 1, n * n - 1, n * (n - 1)])
        self.corners = self.coord[0:2, (np.arange(self.nall) * self.P)[:, None] + cn[None, :]]   # (2, E, 4)
        self.maxc = np.abs(self.coord[0:2, :self.ne * self.P]).max()
        c = self.corners
        edge = np.sqrt(((np.roll(c, -1, axis=2) - c) ** 2).sum(axis=0))                       # (E, 4)
        self.tol = 64 * EPS * self.maxc / (0.5 * edge.min(axis=1))                              # tol_e (E,)
        # the sine of the smallest corner angle
        a, b = np.roll(c, -1, axis=2) - c, np.roll(c, 1, axis=2) - c
        cross = np.abs(a[0] * b[1] - a[1] * b[0])
        self.sin_min = (cross / np.sqrt((a ** 2).sum(axis=0) * (b ** 2).sum(axis=0))).min(axis=1)

    def forward(self, e, xi, eta):
        """The bilinear map of element e (0-based, array) at (xi, eta): (2, M)."""
        c = self.corners[:, e, :]
        w = np.stack([0.25 * (1 - xi) * (1 - eta), 0.25 * (1 + xi) * (1 - eta), 0.25 * (1 + xi) * (1 + eta),
                      0.25 * (1 - xi) * (1 + eta)], axis=-1)
        return (c * w[None]).sum(axis=2)

    def dump(self, xy, ldc=3, source=0):
        return {"ngl": i32(self.ngl), "nelem_owned": i32(self.ne), "nlayers": i32(self.L), "source": i32(source),
                "ldc": i32(ldc), "coord": self.coord[:ldc].reshape(-1, order="F"), "xgl": self.xgl,
                "xy": np.asfortranarray(xy, dtype=np.float64).reshape(-1, order="F")}

    def ref_dump(self, elem, xi, eta, source=0):
        return {"ngl": i32(self.ngl), "nelem_owned": i32(self.ne), "nlayers": i32(self.L), "source": i32(source),
                "ref": i32(1), "xgl": self.xgl, "elem": np.asarray(elem, np.int32),
                "xi_eta": np.stack([xi, eta]).reshape(-1, order="F")}


CASES = {"dg25L3_5x3": ("dg25L3", dict(nelx=5, nely=3)), "bump10_N2": ("bump10", dict(nop=2)), "qmbump8": ("qmbump8", {}),
         "dg25N7L3_3x3": ("dg25N7L3", dict(nelx=3, nely=3)), "bump10_rank1": ("bump10", {})}
BRICK = ["dg25L3_5x3", "bump10_N2", "dg25N7L3_3x3", "bump10_rank1"]
_grids = {}


@pytest.fixture
def grid(case_factory):
    def get(key):
        if key not in _grids:
            name, kw = CASES[key]
            case = case_factory(name, **kw)
            if key == "bump10_rank1":
                from hnumo.partition import partition
                case = partition(case, 2, 1)
                assert 0 < case.nelem_owned < case.scalars["nelem"]        # the rank holds ghosts
            _grids[key] = Grid(case)
        return _grids[key]
    return get


def check_chunks(t, elem, M):
    """The work lists of a plan: every point in exactly one chunk, <= 256 points and <= K distinct
    elements per chunk, consistent slots, a bijective permutation; returns (chunk of each sorted
    point, K)."""
    K, V, ES, CH, LDS, nch = (int(x) for x in t["scalars"])
    assert CH == 256 and K >= 1 and K * ES * 8 <= LDS < (K + 1) * ES * 8
    perm, slot, cp, ce, el = t["perm"], t["slot"], t["chunk_pt"], t["chunk_el"], t["el_list"]
    assert perm.size == M and np.array_equal(np.sort(perm), np.arange(M))
    se = elem[perm]
    assert (np.diff(se) >= 0).all()                                         # sorted by element ...
    same = np.diff(se) == 0
    assert (np.diff(perm)[same] > 0).all()                                  # ... stably
    assert cp.size == nch + 1 and ce.size == nch + 1 and cp[0] == 0 and cp[-1] == M and ce[0] == 0 and ce[-1] == el.size
    assert (np.diff(cp) >= 1).all() and (np.diff(cp) <= 256).all()
    assert (np.diff(ce) >= 0).all() and (np.diff(ce) <= K).all()
    chunk_of = np.repeat(np.arange(nch), np.diff(cp))
    for c in range(nch):
        s = slice(cp[c], cp[c + 1])
        els = el[ce[c]:ce[c + 1]]
        assert np.unique(els).size == els.size
        on = se[s] > 0
        assert (slot[s][~on] == -1).all()
        assert (slot[s][on] >= 0).all() and (slot[s][on] < els.size).all()
        assert np.array_equal(els[slot[s][on]] + 1, se[s][on])
        assert set(els + 1) == set(se[s][on])                               # no element without a point
    return chunk_of, K


def check_weights(t, g, M):
    from hnumo import sample as S
    perm = t["perm"]
    xe = t["xi_eta"].reshape(2, M, order="F")
    w = t["w"].reshape(2 * g.ngl, M)
    on = t["elem"][perm] > 0
    want = np.concatenate([S.lagrange_weights(g.xgl, xe[0, perm]), S.lagrange_weights(g.xgl, xe[1, perm])])
    assert np.array_equal(w[:, on], want[:, on]) and not w[:, ~on].any()


@pytest.mark.parametrize("key", list(CASES))
def test_interior_points_come_back(sample_exe, grid, tmp_path, key):
    g = grid(key)
    rng = np.random.default_rng(11)
    M = 400
    e = rng.integers(0, g.ne, M)
    e[:g.ne] = np.arange(g.ne)[:M]                                          # every owned element at least once
    xi0, eta0 = rng.uniform(-0.9, 0.9, M), rng.uniform(-0.9, 0.9, M)
    xy = g.forward(e, xi0, eta0)
    rc, t = run(sample_exe, g.dump(xy), tmp_path)
    assert rc == 0
    assert t["maxc"][0] == g.maxc
    assert np.array_equal(t["elem"], e + 1)
    xe = t["xi_eta"].reshape(2, M, order="F")
    bound = g.tol[e] / (g.sin_min[e] if key == "qmbump8" else 1.0)
    if key == "qmbump8":
        assert g.sin_min[:g.ne].min() < 0.999                               # the grid is warped
    print(key, "max |dxi|/bound", float((np.abs(xe[0] - xi0) / bound).max()), float((np.abs(xe[1] - eta0) / bound).max()))
    assert (np.abs(xe[0] - xi0) <= bound).all() and (np.abs(xe[1] - eta0) <= bound).all()
    back = g.forward(e, xe[0], xe[1])
    assert np.abs(back - xy).max() <= 64 * EPS * g.maxc
    check_chunks(t, t["elem"], M)
    check_weights(t, g, M)
    # coord(2,npoin) gives the same plan
    rc2, t2 = run(sample_exe, g.dump(xy, ldc=2), tmp_path)
    assert rc2 == 0 and all(np.array_equal(t[k], t2[k]) for k in t)


def lowest_closed_cell(g, xy, scale):
    """Per point the lowest owned element (1-based; 0: none) whose closed cell, widened by `scale`
    times the plan's tolerance, contains it (brick grids: cells are boxes)."""
    c = g.corners[:, :g.ne, :]
    lo, hi = c.min(axis=2), c.max(axis=2)                                   # (2, ne)
    pad = scale * g.tol[None, :g.ne] * 0.5 * (hi - lo)
    inside = np.ones((xy.shape[1], g.ne), bool)
    for d in range(2):
        inside &= (xy[d][:, None] >= (lo[d] - pad[d])[None, :]) & (xy[d][:, None] <= (hi[d] + pad[d])[None, :])
    return np.where(inside.any(axis=1), inside.argmax(axis=1) + 1, 0)


@pytest.mark.parametrize("key", BRICK)
def test_regular_grid_on_a_brick(sample_exe, grid, tmp_path, key):
    """Grid lines on the element edges and through the element centres: the four domain corners,
    points on interior edges and at interior vertices (four closed cells each)."""
    from hnumo import sample as S
    g = grid(key)
    c = g.corners[:, :g.ne, :]
    wx, wy = (c[0].max(axis=1) - c[0].min(axis=1)).max(), (c[1].max(axis=1) - c[1].min(axis=1)).max()
    dx, dy = wx / 2, wy / 2
    if key == "dg25L3_5x3":
        assert dx == 200.0e3                                                # 2000 km / 5 elements / 2: exact
    xi, yi, xy = S.regular_grid(g.case, dx, dy)
    assert xi[0] == g.coord[0, :g.ne * g.P].min() and yi[0] == g.coord[1, :g.ne * g.P].min()
    # i*dx <= xmax - xmin decides the last line (a dy that is not exact in double may lose it)
    xmax, ymax = g.coord[0, :g.ne * g.P].max(), g.coord[1, :g.ne * g.P].max()
    assert xi[-1] <= xmax < xi[-1] + dx and yi[-1] <= ymax < yi[-1] + dy
    assert np.array_equal(xi, xi[0] + np.arange(xi.size) * dx) and np.array_equal(yi, yi[0] + np.arange(yi.size) * dy)
    if key == "dg25L3_5x3":
        assert xi.size == 11 and xi[-1] == xmax
    M = xy.shape[1]
    assert M == xi.size * yi.size and xy[0, 1] == xi[0] and xy[1, 1] == yi[1]   # meshgrid, column-major
    rc, t = run(sample_exe, g.dump(xy), tmp_path)
    assert rc == 0
    want = lowest_closed_cell(g, xy, 1.0)
    # (the expectation does not hinge on the tolerance: no point lies near its edge)
    assert np.array_equal(want, lowest_closed_cell(g, xy, 1.0 / 16)) and np.array_equal(want, lowest_closed_cell(g, xy, 16.0))
    if key != "bump10_rank1":
        assert (want > 0).all()                                             # a rectangle of elements: every point located
    assert (want > 0).sum() >= M // 2
    assert np.array_equal(t["elem"], want)
    xe = t["xi_eta"].reshape(2, M, order="F")
    assert (np.abs(xe) <= 1.0).all()
    on = want > 0
    back = g.forward(want[on] - 1, xe[0, on], xe[1, on])
    assert np.abs(back - xy[:, on]).max() <= 64 * EPS * g.maxc
    # edges and vertices are among the points
    assert (np.abs(xe[0, on]) == 1.0).any() and ((np.abs(xe[0, on]) == 1.0) & (np.abs(xe[1, on]) == 1.0)).any()
    check_chunks(t, t["elem"], M)
    check_weights(t, g, M)


@pytest.mark.parametrize("key", ["dg25L3_5x3", "qmbump8", "bump10_rank1"])
def test_points_without_an_element(sample_exe, grid, tmp_path, key):
    g = grid(key)
    own = g.coord[0:2, :g.ne * g.P]
    lo, hi = own.min(axis=1), own.max(axis=1)
    mid = 0.5 * (lo + hi)
    far = 1e-6 * (hi - lo)                                                  # >> tol_e in x, y (about 1e-14 of the domain)
    assert (far > 1e3 * g.tol.max() * (hi - lo)).all()
    pts = [[hi[0] + far[0], mid[1]], [lo[0] - far[0], mid[1]], [mid[0], hi[1] + far[1]], [mid[0], lo[1] - far[1]],
           [hi[0] * 10 + 1e9, hi[1]], [np.nan, mid[1]], [mid[0], np.nan], [np.inf, mid[1]], [mid[0], -np.inf]]
    inside = g.forward(np.array([0]), np.array([0.25]), np.array([-0.5]))[:, 0]
    pts.append(list(inside))
    nghost = g.nall - g.ne
    if key == "bump10_rank1":
        assert nghost > 0
        ge = np.arange(g.ne, g.nall)
        z = np.zeros(nghost)
        pts += list(g.forward(ge, z, z + 0.3).T)                            # points inside the ghost elements
    xy = np.array(pts).T
    rc, t = run(sample_exe, g.dump(xy), tmp_path)
    assert rc == 0
    elem = t["elem"]
    assert not elem[:9].any()
    assert elem[9] == 1
    assert not elem[10:].any()
    xe = t["xi_eta"].reshape(2, -1, order="F")
    assert not xe[:, elem == 0].any()
    check_chunks(t, elem, xy.shape[1])
    check_weights(t, g, xy.shape[1])


def test_700_points_in_one_element(sample_exe, grid, tmp_path):
    g = grid("dg25L3_5x3")
    rng = np.random.default_rng(5)
    e = np.concatenate([np.full(700, 7), [0, 3, 14]])
    rng.shuffle(e)
    M = e.size
    xy = g.forward(e, rng.uniform(-0.9, 0.9, M), rng.uniform(-0.9, 0.9, M))
    xy[:, 5] = np.nan                                                       # and one point without an element
    rc, t = run(sample_exe, g.dump(xy), tmp_path)
    assert rc == 0
    want = e + 1
    want[5] = 0
    assert np.array_equal(t["elem"], want)
    chunk_of, K = check_chunks(t, t["elem"], M)
    n7 = int((want == 8).sum())
    assert n7 in (699, 700)
    chunks7 = np.unique(chunk_of[t["elem"][t["perm"]] == 8])
    assert chunks7.size == 3                                                # 256 + 256 + the rest
    assert int(t["scalars"][5]) == 3


@pytest.mark.parametrize("key", ["dg25N7L3_3x3", "bump10_N2"])
def test_more_elements_than_slots(sample_exe, grid, tmp_path, key):
    """One point per element: chunks are cut by the arena's K element slots, not by 256 points."""
    g = grid(key)
    e = np.arange(g.ne)[::-1].copy()
    z = np.zeros(g.ne)
    for source, V in ((0, 5 * g.L + 4), (1, 5 * g.L)):
        rc, t = run(sample_exe, g.ref_dump(e + 1, z + 0.5, z - 0.25, source), tmp_path)
        assert rc == 0
        K = int(t["scalars"][0])
        assert int(t["scalars"][1]) == V and int(t["scalars"][2]) == (V * g.P) | 1
        assert K == 32768 // (8 * ((V * g.P) | 1))
        if key == "dg25N7L3_3x3":
            assert K < g.ne
        check_chunks(t, t["elem"], g.ne)
        assert int(t["scalars"][5]) == -(-g.ne // min(K, 256))
        assert np.array_equal(t["elem"], e + 1)
        assert np.array_equal(t["xi_eta"].reshape(2, -1, order="F"), np.stack([z + 0.5, z - 0.25]))
        check_weights(t, g, g.ne)


def test_caller_supplied_nodes_have_unit_weights(sample_exe, grid, tmp_path):
    g = grid("bump10_N2")
    e = np.repeat(np.arange(g.ne), g.P)
    i, j = np.tile(np.arange(g.P) % g.ngl, g.ne), np.tile(np.arange(g.P) // g.ngl, g.ne)
    rc, t = run(sample_exe, g.ref_dump(e + 1, g.xgl[i], g.xgl[j]), tmp_path)
    assert rc == 0
    M = e.size
    w = t["w"].reshape(2 * g.ngl, M)
    perm = t["perm"]
    assert np.array_equal(w[:g.ngl], np.eye(g.ngl)[:, i[perm]]) and np.array_equal(w[g.ngl:], np.eye(g.ngl)[:, j[perm]])
    check_chunks(t, t["elem"], M)


def _valid(g):
    xy = g.forward(np.array([0, 1, 2]), np.array([0.1, 0.2, 0.3]), np.array([0.0, -0.4, 0.6]))
    return g.dump(xy)


def _drop(k):
    def f(d, g):
        del d[k]
    return f


def _set(k, v):
    def f(d, g):
        d[k] = v
    return f


def _xgl(fn):
    def f(d, g):
        x = d["xgl"].copy()
        fn(x)
        d["xgl"] = x
    return f


def _swap(x):
    x[1], x[2] = x[2], x[1]


def _curved(d, g):
    c = d["coord"].reshape(3, -1, order="F").copy(order="F")
    I = 2 * g.P + g.ngl + 1                                                 # node (2,2) of element 3: interior
    c[0, I] += 1e-3 * (c[0, 2 * g.P + g.ngl - 1] - c[0, 2 * g.P])
    d["coord"] = c.reshape(-1, order="F")


def _ref(fn):
    def f(d, g):
        r = g.ref_dump(np.array([1, 0, 3]), np.array([0.1, 0.0, 1.0]), np.array([-1.0, 0.0, 0.6]))
        d.clear()
        d.update(r)
        fn(d)
    return f


def _xe(i, v):
    def f(d):
        x = d["xi_eta"].copy()
        x[i] = v
        d["xi_eta"] = x
    return f


def _pop(k):
    def f(d):
        del d[k]
        d["M"] = i32(3)
    return f


def _elem(i, v):
    def f(d):
        e = d["elem"].copy()
        e[i] = v
        d["elem"] = e
    return f


REJECT = {
    "coord NULL": (_drop("coord"), "coord is NULL"),
    "xy NULL": (_drop("xy"), "xy is NULL"),
    "xgl NULL": (_drop("xgl"), "xgl is NULL"),
    "ldc 4": (_set("ldc", i32(4)), "ldc must be 2 or 3"),
    "ldc 1": (_set("ldc", i32(1)), "ldc must be 2 or 3"),
    "M 0": (_set("M", i32(0)), "M must be >= 1"),
    "M -1": (_set("M", i32(-1)), "M must be >= 1"),
    "xgl not ascending": (_xgl(_swap), "ascend strictly"),
    "xgl repeated": (_xgl(lambda x: x.__setitem__(1, x[0])), "ascend strictly"),
    "xgl from -0.5": (_xgl(lambda x: x.__setitem__(0, -0.5)), "ascend strictly"),
    "xgl to 1.5": (_xgl(lambda x: x.__setitem__(-1, 1.5)), "ascend strictly"),
    "xgl NaN": (_xgl(lambda x: x.__setitem__(1, np.nan)), "ascend strictly"),
    "curved element": (_curved, "not the bilinear map"),
    "ref elem NULL": (_ref(_pop("elem")), "elem is NULL"),
    "ref xi_eta NULL": (_ref(_pop("xi_eta")), "xi_eta is NULL"),
    "ref xgl not ascending": (_ref(lambda d: d.__setitem__("xgl", d["xgl"][::-1].copy())), "ascend strictly"),
    "ref M 0": (_ref(lambda d: d.__setitem__("M", i32(0))), "M must be >= 1"),
    "ref elem -1": (_ref(_elem(1, -1)), "outside 0.."),
    "ref elem past the owned": (_ref(_elem(0, 10 ** 6)), "outside 0.."),
    "ref xi above 1": (_ref(_xe(0, 1.0 + 2.0 ** -52)), "outside [-1,1]"),
    "ref eta below -1": (_ref(_xe(3, -1.0000001)), "outside [-1,1]"),
    "ref xi NaN": (_ref(_xe(4, np.nan)), "outside [-1,1]"),
}


@pytest.mark.parametrize("what", list(REJECT))
def test_rejected(sample_exe, grid, tmp_path, what):
    g = grid("dg25L3_5x3")
    d = _valid(g)
    rc, t = run(sample_exe, d, tmp_path)
    assert rc == 0 and np.array_equal(t["elem"], [1, 2, 3])
    mutate, text = REJECT[what]
    mutate(d, g)
    rc, t = run(sample_exe, d, tmp_path)
    assert rc == INVALID
    msg = t["error"].tobytes().rstrip(b"\0").decode()
    assert text in msg, msg


def test_owned_limit_of_the_partition_rank(sample_exe, grid, tmp_path):
    """elem = nelem_owned is the last valid element of a rank; its first ghost is rejected."""
    g = grid("bump10_rank1")
    z = np.zeros(1)
    rc, t = run(sample_exe, g.ref_dump([g.ne], z, z), tmp_path)
    assert rc == 0
    rc, t = run(sample_exe, g.ref_dump([g.ne + 1], z, z), tmp_path)
    assert rc == INVALID
