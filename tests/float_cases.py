"""The float sets' test cases, shared by tests/test_float_plan.py (C++ host statement against the
Python mirror) and tests/test_floats_gpu.py (kernel against the mirror): a plain helper module.

Four grids -- dg25L3 5x3 (N=4, L=3), bump10 at N=2 (100 elements, L=2), qmbump8 (warped
quadrilaterals that meet in either direction), dg25N7L3 3x3 (N=7) -- carrying tests/states.py's
moving state, and seeds that exercise every branch of the location: rings around the interior
vertices (floats that cross to the diagonal neighbour take two hops), points within 1e-9 (in
reference coordinates) of element edges on either side, points exactly on edges and on vertices and
points 0.2 short of them, and points 0.1 short of every wall of the domain.  big_dt moves the fastest
float about 0.7 of an element per advance."""
import numpy as np

from states import moving_case

CASES = [("dg25L3", {"nelx": 5, "nely": 3}), ("bump10", {"nop": 2}), ("qmbump8", {}), ("dg25N7L3", {"nelx": 3, "nely": 3})]
IDS = ["dg25L3_5x3", "bump10_N2", "qmbump8", "dg25N7L3_3x3"]
_cache = {}


def moving(case_factory, name, kw):
    """The case carrying its moving state (built once)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = moving_case(case_factory(name, **kw))
    return _cache[key]


def corners_of(case):
    """(ne, 4, 2): the corner nodes of the owned elements, counter-clockwise from (-1,-1)."""
    from hnumo import sample as S
    n, ne = case.scalars["ngl"], S.owned_elements(case)
    cn = np.array([0, n - 1, n * n - 1, n * (n - 1)])
    c = np.asarray(case.arrays["coord"])[0:2, (np.arange(ne) * n * n)[:, None] + cn[None, :]]
    return np.ascontiguousarray(c.transpose(1, 2, 0))


def forward(c, xi, eta):
    """The bilinear map of corners c (4, 2) at (xi, eta)."""
    w = np.array([0.25 * (1 - xi) * (1 - eta), 0.25 * (1 + xi) * (1 - eta), 0.25 * (1 + xi) * (1 + eta), 0.25 * (1 - xi) * (1 + eta)])
    return (w[:, None] * c).sum(axis=0)


def seeds(case, max_edge_elems=16):
    """(xy (2, M), layer (M)): the seeds described above; layers cycle through 1..L."""
    from hnumo import floats as FL
    c = corners_of(case)
    ne = c.shape[0]
    h = np.sqrt(((np.roll(c, -1, axis=1) - c) ** 2).sum(axis=2)).min()
    pts = []
    # rings of 4 around every interior vertex (a corner that four owned elements share)
    key = np.round(c.reshape(-1, 2) / (1e-6 * h)).astype(np.int64)
    uniq, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    first = {}
    for t, u in enumerate(inv.reshape(-1)):
        first.setdefault(int(u), t)
    for u in np.nonzero(cnt == 4)[0]:
        v = c.reshape(-1, 2)[first[int(u)]]
        pts += list(FL.seed_ring(v, 0.12 * h, 4, phase=0.3 + 0.37 * u).T)
    # edges and vertices of a few elements: half of them at the domain's walls (where a stepped state
    # has no normal velocity at the wall's own nodes: a float reaches a wall from inside the element,
    # so 0.2 short of every side is seeded too)
    nbr = FL.side_neighbours(case)
    wall = np.nonzero((nbr == FL.WALL).any(axis=1))[0]
    rng = np.random.default_rng(17)
    pick = list(rng.permutation(wall)[:max_edge_elems // 2]) + list(rng.permutation(ne))
    chosen = list(dict.fromkeys(int(e) for e in pick))[:max_edge_elems]
    d = 1e-9
    for e in chosen:
        for t in (-0.6, 0.35):
            for s in (-1.0, 1.0):
                for a in (s * 0.8, s * (1.0 - d), s, s * (1.0 + d)):
                    pts.append(forward(c[e], a, t))
                    pts.append(forward(c[e], t, a))
        pts += list(c[e])
    # 0.1 short of every wall, all round the domain
    for e in wall:
        for side in np.nonzero(nbr[e] == FL.WALL)[0]:
            a = 0.9 if side % 2 else -0.9
            for t in (-0.6, 0.35):
                pts.append(forward(c[e], a, t) if side < 2 else forward(c[e], t, a))
    xy = np.asfortranarray(np.array(pts).T)
    layer = (np.arange(xy.shape[1]) % case.scalars["nlayers"] + 1).astype(np.int32)
    return xy, layer


def big_dt(case, q, frac=0.7):
    """dt that moves the fastest node velocity `frac` of the shortest element edge."""
    c = corners_of(case)
    h = np.sqrt(((np.roll(c, -1, axis=1) - c) ** 2).sum(axis=2)).min()
    n = c.shape[0] * case.scalars["ngl"] ** 2
    u, v = q[1, :n] / q[0, :n], q[2, :n] / q[0, :n]
    return float(frac * h / np.sqrt(u * u + v * v).max())


def run_mirror(hf, states_dts):
    """Advance the mirror hf through [(q, dt), ...]; returns (records (5, M, n), stats) where stats
    has per float whether it changed element, its most hops in one location, whether a wall moved it."""
    e0 = hf.elem.copy()
    changed = np.zeros(hf.M, bool)
    hops = np.zeros(hf.M, np.int32)
    walled = np.zeros(hf.M, bool)
    recs = []
    for q, dt in states_dts:
        before = hf.elem.copy()
        hf.advance(q, dt)
        changed |= (hf.elem != before) & (hf.elem > 0)
        hops = np.maximum(hops, hf.hops)
        walled |= hf.walled
        g = hf.get()
        recs.append(np.stack([g["x"], g["y"], g["u"], g["v"], g["elem"].astype(np.float64)]))
    return np.stack(recs, axis=2), dict(changed=changed, hops=hops, walled=walled, elem0=e0)


def check_conditions(hf, stats, wall=True):
    """What the seeds must exercise, from the mirror alone.  wall = False: the state cannot take a float
    to a wall (and the mirror agrees that none got there)."""
    from hnumo import floats as FL
    on = stats["elem0"] > 0
    assert on.sum() >= 0.9 * hf.M                                  # nearly every seed lies in the domain
    assert stats["changed"][on].sum() * 3 >= on.sum(), (int(stats["changed"].sum()), int(on.sum()))
    assert (stats["hops"] >= 2).any()
    assert stats["walled"].any() == wall
    assert not (hf.status == FL.LOST).any()
