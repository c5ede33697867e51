"""The re-fetch of the persistent sub-cycle's B inputs (kernels_btp.hip, StageCfg::IDLEB).  Term
buffer 1 overlays a stage's bottom-layer qprime, face statics and face coefficients, so every stage
but a launch's last copies them back in behind its D phases; in the 256-thread exact-sum arenas the
copies are issued by waves 1..3, idle during E1, and not by the E1 wave.  The hazard is an LDS word of
the next stage's inputs that is missing, torn or read before its copy has landed -- every wave waits
for its own copies only, and one barrier orders them for the others -- which a 3x3 mesh shows as well
as 25x25; nothing may move a bit.  As in tests/test_stage_boundary_gpu.py: small meshes, 2
baroclinic steps, the persistent engine against the CPU oracle and against an engine on per-stage
launches (HNUMO_PERSISTENT=0) -- the state and every parity field.

The compile-time condition per instantiation of the exact-sum arena (StageCfg<NGL, NQ, false>: BS
threads, RC quad rows per term chunk, NCH chunks, chunk k in buffer k & 1, buffer 1 over the B
inputs):

    N   NQ   BS   RC   NCH   IDLEB   the copies are issued by
    2    5  128    5     1   false   both waves
    3    7  256    7     1   true    waves 1..3 (one chunk: buffer 1 never holds terms)
    4    9  256    3     3   true    waves 1..3 (dg25L3: the bench's arena)
    5   11  256    1    11   true    waves 1..3 (the chains summed by their own lanes, VSUM)
    7   15  256    -     -   false   all four (the slim arena: no term buffers; waits in the next stage)

so both branches run: N = 2 keeps the issue from every wave, N = 3, 4, 5 take the three-wave rotation.
(The issue this file answers asked for the copies a whole D phase earlier, where NCH is odd and at
least 3 -- N = 4 and N = 5 -- and for N with NCH == 1 as the other branch; that variant measured
slower and is not in the code, DESIGN.md section 9 round 20, and the cases stay as asked.)"""
import numpy as np
import pytest

import matrix as M

pytestmark = pytest.mark.gpu

NSTEPS = 2
# dg25L3's physics (three layers, wind, bottom friction on: the qprime copy is among the re-fetched)
DG = {
    # every element a corner, an edge or the single interior one
    "dg-3x3": dict(nelx=3, nely=3),
    # interior elements with four polled faces
    "dg-6x6": dict(nelx=6, nely=6),
    # no bottom friction: no qprime copy
    "dg-6x6-nobotfr": dict(nelx=6, nely=6, botfr=0, cd=0.0),
    # SSP(3,3): other stage flags, and another stage count in front of the launch's last stage, which
    # alone has no re-fetch
    "dg-6x6-ssp33": dict(nelx=6, nely=6, kstages=3),
}
# the lake at rest, two layers, no bottom friction
LAKE = {"lake-4x4-L2": dict(nelx=4, nely=4, nlayers=2)}


def _cell(N):
    # the double gyre as tests/matrix.py builds its cells at this order: 4x4 (3x3 above N = 4), the time
    # steps scaled with the order, a moving state
    return dict(N=N, family="dg3", visc=3, walls="mixed", botfr=1, shear=0, mesh="brick", state="moving")


ORDERS = {"dg-N2": 2, "dg-N3": 3, "dg-N5": 5}
NAMES = list(DG) + list(LAKE) + list(ORDERS)


def _case(name, case_factory):
    if name in DG:
        return case_factory("dg25L3", **DG[name])
    if name in LAKE:
        return case_factory("lake10", **LAKE[name])
    return M.cell_case(_cell(ORDERS[name]), case_factory)


def _engine_run(case):
    from hnumo import bundle as B
    from hnumo.engine import Engine
    e = Engine(case)
    try:
        st = e.state()
        for _ in range(NSTEPS):
            e.ti_rk_bcl(*st)
        fields = {f: e.field(f) for f, _ in B.FIELDS}
        path = e.stage_path
        aborts = e.persistent_stats["aborts"]
    finally:
        e.close()
    return st, fields, path, aborts


@pytest.mark.parametrize("name", NAMES)
def test_early_refetch_bitwise(name, case_factory, monkeypatch):
    from hnumo import bundle as B
    case = _case(name, case_factory)
    if name in ORDERS:
        assert case.scalars["ngl"] - 1 == ORDERS[name] and case.scalars["nlayers"] == 3
    else:
        assert case.scalars["ngl"] == 5
    st, fields, path, aborts = _engine_run(case)
    assert path == "persistent", path
    assert aborts == 0

    so, ofields = M.run_oracle(case, NSTEPS)
    for nm, x, y in zip(("q", "qb", "qprime"), st, so):
        assert np.isfinite(y).all(), nm
        assert np.array_equal(x, y), ("oracle", nm)
    for f, _ in B.FIELDS:
        assert np.array_equal(fields[f], ofields[f]), ("oracle", f)

    monkeypatch.setenv("HNUMO_PERSISTENT", "0")
    st0, fields0, path0, _ = _engine_run(case)
    monkeypatch.delenv("HNUMO_PERSISTENT")
    assert path0 == "per-stage", path0
    for nm, x, y in zip(("q", "qb", "qprime"), st, st0):
        assert np.array_equal(x, y), ("per-stage", nm)
    for f in fields:
        assert np.array_equal(fields[f], fields0[f]), ("per-stage", f)
