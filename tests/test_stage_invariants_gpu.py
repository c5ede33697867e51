"""The persistent sub-cycle's stage body on the small shapes at which a change of its code can go
wrong (kernels_btp.hip, stage_body with PERSIST): every face orientation and wall code, every
stage count of the SSP-RK tables, a physics without bottom friction, every instantiation of the
body -- among them the A2 interpolation with its rows unrolled and read one row ahead.  None of it
may move a bit: 2 baroclinic steps, the persistent engine against the CPU oracle and against an
engine on per-stage launches (HNUMO_PERSISTENT=0) -- the state and every parity field."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (configuration, overrides)
CASES = {
    # every element a corner, an edge or the one interior; corner nodes take two wall fixes
    "3x3": ("dg25L3", dict(nelx=3, nely=3)),
    # neighbour / local-face pairs a square mesh does not produce
    "2x5": ("dg25L3", dict(nelx=2, nely=5)),
    "5x2": ("dg25L3", dict(nelx=5, nely=2)),
    # no-slip and free-slip wall codes
    "6x6_mixed_walls": ("dg25L3", dict(nelx=6, nely=6, x_boundary=(2, 4))),
    # the stage tables: first_of_step on every stage (K=1), a1 == 0 / a3 == 0 patterns, save_q2 only
    # at K=5
    "4x4_k1": ("dg25L3", dict(nelx=4, nely=4, kstages=1)),
    "4x4_k2": ("dg25L3", dict(nelx=4, nely=4, kstages=2)),
    "4x4_k3": ("dg25L3", dict(nelx=4, nely=4, kstages=3)),
    "4x4_k5": ("dg25L3", dict(nelx=4, nely=4, kstages=5)),
    # botfr = 0: qpm == 0, two interpolation groups, no bottom-layer scratch
    "bump_4x4": ("bump10", dict(nelx=4, nely=4)),
    # the other instantiations of the same body (<3,5>: 128-thread blocks; <4,7>; <6,11>)
    "4x4_nop2": ("dg25L3", dict(nelx=4, nely=4, nop=2)),
    "4x4_nop3": ("dg25L3", dict(nelx=4, nely=4, nop=3)),
    "4x4_nop5": ("dg25L3", dict(nelx=4, nely=4, nop=5)),
    # the slim arena (<8,15>)
    "n7_3x3": ("dg25N7L3", dict(nelx=3, nely=3)),
}
# the instantiations the engine may run on per-stage launches instead: skipped with the reason then
MAY_NOT_PERSIST = {"4x4_nop2", "4x4_nop3", "4x4_nop5"}
NSTEPS = 2


def _engine_run(case):
    from hnumo import bundle as B
    from hnumo.engine import Engine
    e = Engine(case)
    st = e.state()
    path = e.stage_path
    for _ in range(NSTEPS):
        e.ti_rk_bcl(*st)
    fields = {f: e.field(f) for f, _ in B.FIELDS}
    e.close()
    return st, fields, path


@pytest.mark.parametrize("name", list(CASES))
def test_stage_invariants_bitwise(name, case_factory, monkeypatch):
    import oracle as O
    from hnumo import bundle as B
    cfg, over = CASES[name]
    case = case_factory(cfg, **over)
    st, fields, path = _engine_run(case)
    if name in MAY_NOT_PERSIST and path != "persistent":
        pytest.skip(f"{name}: the engine runs this shape on {path} launches")
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


def test_resident_three_steps(case_factory):
    """Three steps in resident mode behind the uploading one (no host round trip between the
    launches): the epoch and the stage tags carry from launch to launch."""
    import oracle as O
    from hnumo.engine import Engine
    case = case_factory("dg25L3", nelx=6, nely=6)
    e = Engine(case)
    assert e.stage_path == "persistent", e.stage_path
    e.set_resident(True)
    st = e.state()
    e.ti_rk_bcl(*st)  # (the first resident step uploads the state; bench_steps runs on the device's)
    e.bench_steps(3)
    e.sync(*st)
    e.close()
    o = O.Oracle(case)
    so = o.state()
    for _ in range(4):
        o.ti_rk_bcl(*so)
    for nm, x, y in zip(("q", "qb", "qprime"), st, so):
        assert np.isfinite(y).all(), nm
        assert np.array_equal(x, y), nm
