"""The stage-to-stage boundary of the persistent sub-cycle (kernels_btp.hip, stage_body with
PERSIST): E1 updates the state in place and keeps the Shu-Osher copies itself, each wave waits for
its re-fetched B inputs before the barrier in front of E2, and one LDS barrier, with no wait for the
trace stores, separates E2 from the next stage's interpolation.  None of it may move a bit: small
double-gyre meshes (dg25L3's physics, N=4), 2 baroclinic steps, the persistent engine against the
CPU oracle and against an engine on per-stage launches (HNUMO_PERSISTENT=0) -- the state and
every parity field."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = {
    # every element a corner, an edge or the single interior one; corner nodes take the wall fix on
    # two faces in E1
    "3x3": dict(nelx=3, nely=3),
    # interior elements with four polled faces
    "6x6": dict(nelx=6, nely=6),
    # no-slip and free-slip walls in the in-place E1
    "6x6_mixed_walls": dict(nelx=6, nely=6, x_boundary=(2, 4)),
    # SSP(3,3): a1 != 0 with a3 == 0 -- qb0 saved and read, qb2 never
    "6x6_ssp33": dict(nelx=6, nely=6, kstages=3),
}
NSTEPS = 2


def _engine_run(case):
    from hnumo import bundle as B
    from hnumo.engine import Engine
    e = Engine(case)
    st = e.state()
    for _ in range(NSTEPS):
        e.ti_rk_bcl(*st)
    fields = {f: e.field(f) for f, _ in B.FIELDS}
    path = e.stage_path
    e.close()
    return st, fields, path


@pytest.mark.parametrize("name", list(CASES))
def test_stage_boundary_bitwise(name, case_factory, monkeypatch):
    import oracle as O
    from hnumo import bundle as B
    case = case_factory("dg25L3", **CASES[name])
    st, fields, path = _engine_run(case)
    assert path == "persistent", path

    o = O.Oracle(case)
    so = o.state()
    for _ in range(NSTEPS):
        o.ti_rk_bcl(*so)
    for nm, x, y in zip(("q", "qb", "qprime"), st, so):
        assert np.isfinite(y).all(), nm
        assert np.array_equal(x, y), ("oracle", nm)
    for f, _ in B.FIELDS:
        assert np.array_equal(fields[f], o.field(f)), ("oracle", f)

    monkeypatch.setenv("HNUMO_PERSISTENT", "0")
    st0, fields0, path0 = _engine_run(case)
    monkeypatch.delenv("HNUMO_PERSISTENT")
    assert path0 == "per-stage", path0
    for nm, x, y in zip(("q", "qb", "qprime"), st, st0):
        assert np.array_equal(x, y), ("per-stage", nm)
    for f in fields:
        assert np.array_equal(fields[f], fields0[f]), ("per-stage", f)
