"""The trace hand-off of the persistent sub-cycle (kernels_btp.hip, stage_body with PERSIST, N <= 5):
each thread packs, once per launch, which LDS word it publishes and which slot of the neighbour it
writes (put_granule), and the stage loop carries that descriptor, whose sign also tells the
consumer whether its face has a neighbour.  The lane -> (face, component, node) -> neighbour slot map is
where this can go wrong, so the shapes are the smallest on which it differs: elements with
boundary and interior faces on either face side, one with four neighbours, mixed walls, a warped
grid whose rotated corner lists make neighbours disagree on local face numbers and node order,
both SSP schemes, and every NGL of the changed instantiations (128- and 256-thread blocks, 96 to
192 granules).  Two baroclinic steps of N_btp = 2 from a moving state: the second step's launches
find the previous epoch's tags in both granule buffers.  Bitwise: the persistent engine against
the CPU oracle and against an engine on per-stage launches (HNUMO_PERSISTENT=0) -- the state and
every parity field."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# N_btp = ceil(dt / dt_btp) = 2; far below the stability limit of the coarsest-celled N = 5 grid here
STEP = dict(dt=30.0, dt_btp=20.0)
CASES = {
    # every element: two interior and two boundary faces, as left and as right element of a face
    "2x2": dict(nelx=2, nely=2),
    # the centre element polls and publishes on four faces
    "3x3": dict(nelx=3, nely=3),
    "3x3_mixed_walls": dict(nelx=3, nely=3, x_boundary=(2, 4)),
    "4x4_warp_rotated": dict(nelx=4, nely=4, mesh=("warp", 0.15, True)),
    "3x3_ssp33": dict(nelx=3, nely=3, kstages=3),
    "3x3_ssp53": dict(nelx=3, nely=3, kstages=5),
    "3x3_ngl3": dict(nelx=3, nely=3, nop=2),
    "3x3_ngl4": dict(nelx=3, nely=3, nop=3),
    "3x3_ngl5": dict(nelx=3, nely=3, nop=4),
    "3x3_ngl6": dict(nelx=3, nely=3, nop=5),
}
NSTEPS = 2


def _case(case_factory, name):
    import states
    return states.moving_case(case_factory("dg25L3", **STEP, **CASES[name]))


def _engine_run(case, abort=None):
    from hnumo import bundle as B
    from hnumo.engine import Engine
    e = Engine(case)
    path = e.stage_path
    if abort is not None:
        e.debug_force_abort(abort)
    st = e.state()
    for _ in range(NSTEPS):
        e.ti_rk_bcl(*st)
    fields = {f: e.field(f) for f, _ in B.FIELDS}
    stats = e.persistent_stats
    e.close()
    return st, fields, path, stats


def _per_stage_run(case, monkeypatch):
    monkeypatch.setenv("HNUMO_PERSISTENT", "0")
    st0, fields0, path0, _ = _engine_run(case)
    monkeypatch.delenv("HNUMO_PERSISTENT")
    assert path0 == "per-stage", path0
    return st0, fields0


@pytest.mark.parametrize("name", list(CASES))
def test_trace_handoff_bitwise(name, case_factory, monkeypatch):
    import oracle as O
    from hnumo import bundle as B
    case = _case(case_factory, name)
    assert case.scalars["N_btp"] == 2
    st, fields, path, stats = _engine_run(case)
    assert path == "persistent", path
    assert stats["aborts"] == 0, stats

    o = O.Oracle(case)
    so = o.state()
    for _ in range(NSTEPS):
        o.ti_rk_bcl(*so)
    for nm, x, y in zip(("q", "qb", "qprime"), st, so):
        assert np.isfinite(y).all(), nm
        assert np.array_equal(x, y), ("oracle", nm)
    for f, _ in B.FIELDS:
        assert np.array_equal(fields[f], o.field(f)), ("oracle", f)

    st0, fields0 = _per_stage_run(case, monkeypatch)
    for nm, x, y in zip(("q", "qb", "qprime"), st, st0):
        assert np.array_equal(x, y), ("per-stage", nm)
    for f in fields:
        assert np.array_equal(fields[f], fields0[f]), ("per-stage", f)


def test_forced_abort_redo_is_identical(case_factory, monkeypatch):
    """The corrector's launch of the first step gives up (hnumo_debug_force_abort(1)) after the
    predictor's launch has published into both granule buffers; the step is redone on per-stage
    kernels.  The state after two steps is the per-stage engine's, bit for bit."""
    case = _case(case_factory, "4x4_warp_rotated")
    st, fields, path, stats = _engine_run(case, abort=1)
    assert path == "persistent", path
    assert stats["aborts"] == 1, stats
    st0, fields0 = _per_stage_run(case, monkeypatch)
    for nm, x, y in zip(("q", "qb", "qprime"), st, st0):
        assert np.isfinite(y).all(), nm
        assert np.array_equal(x, y), ("per-stage", nm)
    for f in fields:
        assert np.array_equal(fields[f], fields0[f]), ("per-stage", f)
