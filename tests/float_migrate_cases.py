"""The migrating float sets' test cases, shared by tests/test_float_migrate_plan.py, _cpu.py and _gpu.py:
a plain helper module.  Two rows -- bump10 at N=2 on 2 block ranks, dg25L3 5x3 on 4 Morton ranks -- with
tests/float_cases.py's seeds (max_edge_elems=24) plus rings of radius 0.12 h around points on the rank
boundaries and around the vertices where ranks meet, and dg25N7L3 3x3 on 2 Morton ranks (NGL = 8).  The
state is tests/states.py's moving state; an advance moves the fastest float 0.7 of an element."""
import numpy as np

import float_cases as FC
from hnumo import floats as FL
from hnumo.facepart import face_partition

ROWS = [(1, 2, "block"), (0, 4, "morton")]            # (index into FC.CASES, ranks, element order)
ROW_IDS = ["bump10_N2_2block", "dg25L3_5x3_4morton"]
NGL8 = (3, 2, "morton")      # (a 3x3 brick has no 2-block split: two chunks of the Morton curve, 4 + 5 elements)
NADV = 6
_cache = {}


def partition(case_factory, row):
    """(case, parts) of a row."""
    which, n, order = row
    key = ("parts", row)
    if key not in _cache:
        case = FC.moving(case_factory, *FC.CASES[which])
        _cache[key] = (case, [face_partition(case, n, r, order) for r in range(n)])
    return _cache[key]


def boundary_rings(case, parts):
    """Rings of 8 seeds of radius 0.12 h around the midpoints and third points of every face between two
    ranks, and around every vertex that elements of three or more ranks share."""
    c = FC.corners_of(case)
    h = np.sqrt(((np.roll(c, -1, axis=1) - c) ** 2).sum(axis=2)).min()
    owner = np.zeros(c.shape[0], np.int64)
    for r, p in enumerate(parts):
        owner[np.asarray(p.elems)] = r
    face = np.asarray(case.arrays["face"])
    pts = []
    side_corners = {}
    key = lambda v: tuple(np.round(v / (1e-6 * h)).astype(np.int64))
    at = {}
    for e in range(c.shape[0]):
        for v in c[e]:
            at.setdefault(key(v), (v, set()))[1].add(int(owner[e]))
    n = 0
    for f in range(face.shape[1]):
        el, er = int(face[6, f]) - 1, int(face[7, f]) - 1
        if er < 0 or owner[el] == owner[er]:
            continue
        shared = [v for v in c[el] if any(np.abs(v - w).sum() < 1e-6 * h for w in c[er])]
        assert len(shared) == 2
        for t in (0.5, 0.3):
            mid = shared[0] + t * (shared[1] - shared[0])
            pts += list(FL.seed_ring(mid, 0.12 * h, 8, phase=0.2 + 0.41 * n).T)
            n += 1
    for v, owners in at.values():
        if len(owners) >= 3:
            pts += list(FL.seed_ring(v, 0.12 * h, 8, phase=0.1 + 0.29 * n).T)
            n += 1
    return np.array(pts).T


def seeds(case, parts):
    xy, _ = FC.seeds(case, max_edge_elems=24)
    xy = np.asfortranarray(np.concatenate([xy, boundary_rings(case, parts)], axis=1))
    layer = (np.arange(xy.shape[1]) % case.scalars["nlayers"] + 1).astype(np.int32)
    return xy, layer


def mirror_run(case_factory, row, scaled=True, nadv=NADV):
    """NADV advances of big_dt on the moving state: the single-rank mirror `one` with its series `ref`, the
    group mirror with the ranks' series and their merge, and the per-advance records of every rank."""
    key = ("run", row, scaled, nadv)
    if key in _cache:
        return _cache[key]
    case, parts = partition(case_factory, row)
    xy, layer = seeds(case, parts)
    q = case.arrays["q_df"]
    dt = FC.big_dt(case, q)
    one = FL.HostFloats(case, xy, layer)
    scale = one.maxc if scaled else 0.0
    grp = FL.HostFloatGroup(parts, xy, layer, coord_scale=scale)
    # where every seed sits: one rank at the most, and in the single-rank run's element
    agree = True
    for m in range(one.M):
        on = [(r, int(hf.elem[m])) for r, hf in enumerate(grp.ranks) if hf.status[m] == FL.ACTIVE]
        agree = agree and len(on) == (1 if one.elem[m] > 0 else 0)
        agree = agree and all(int(parts[r].elems[e - 1]) + 1 == int(one.elem[m]) for r, e in on)
    states = [p.arrays["q_df"] for p in parts]
    fields = []
    for _ in range(nadv):
        one.advance(q, dt)
        one.record()
        grp.advance(states, dt)
        grp.record()
        fields.append([{k: getattr(hf, k).copy() for k in ("x", "y", "wx", "wy", "xi", "eta", "elem", "status")} for hf in grp.ranks])
    sers = grp.series()
    out = dict(case=case, parts=parts, xy=xy, layer=layer, dt=dt, one=one, group=grp, ref=one.series(), series=sers,
               merged=FL.merge_series(sers, parts), seed_elems_agree=agree, fields=fields, scale=scale)
    _cache[key] = out
    return out
