"""On-device run diagnostics (kernels_diag.hip through hnumo_diagnostics / hnumo_layer_fields):
every value the engine returns for the state it holds equals -- np.array_equal, no tolerance --
what the host restatement of the reference's routines (hnumo/diagnostics.py: layer_fields,
conserved_mass, courant, numpy max/min; pinned to the reference by tests/test_diagnostics.py)
gives on the same state after hnumo_sync."""
import io

import numpy as np
import pytest

from hnumo import diagnostics as D

pytestmark = pytest.mark.gpu
KEYS = ("cfl_b", "cfl", "min_dx", "min_dy", "qbmax", "qbmin", "mass", "qmax", "qmin")


def host_diagnostics(case, q, qb):
    """The host path's numbers for the state (q, qb) of `case`, and its layer fields."""
    qf = D.layer_fields(case, q)
    cfl_b, cfl, dxm, dym = D.courant(case, qf, qb)
    L = case.scalars["nlayers"]
    return {"cfl_b": cfl_b, "cfl": cfl, "min_dx": dxm, "min_dy": dym, "qbmax": qb.max(axis=1), "qbmin": qb.min(axis=1),
            "mass": np.array([D.conserved_mass(case, qf[0, :, k]) for k in range(L)]),
            "qmax": qf.max(axis=1), "qmin": qf.min(axis=1)}, qf


def assert_same(dev, host, keys=KEYS, what=""):
    for k in keys:
        a, b = np.asarray(dev[k], dtype=np.float64), np.asarray(host[k], dtype=np.float64)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        assert np.array_equal(a, b), (what, k, a, b, a - b)


def running_cell_minima(case):
    """courant.F90:95-99 per sub-cell in the reference's loop order (as hnumo.diagnostics.courant)."""
    A, S = case.arrays, case.scalars
    ngl, E = S["ngl"], S["nelem"]
    P, nc = ngl * ngl, ngl - 1
    e = np.arange(E)[:, None, None]
    j = np.arange(nc)[None, :, None]
    i = np.arange(nc)[None, None, :]
    corners = [e * P + j * ngl + i, e * P + j * ngl + i + 1, e * P + (j + 1) * ngl + i, e * P + (j + 1) * ngl + i + 1]
    corners = [np.broadcast_to(c, (E, nc, nc)).reshape(-1) for c in corners]
    x = np.stack([A["coord"][0, c] for c in corners])
    y = np.stack([A["coord"][1, c] for c in corners])
    return (np.minimum.accumulate(np.concatenate([[1e16], x.max(0) - x.min(0)]))[1:],
            np.minimum.accumulate(np.concatenate([[1e16], y.max(0) - y.min(0)]))[1:])


def resident_run(case, nsteps=2):
    """nsteps resident steps, the diagnostics and the layer fields BEFORE any sync, then the
    synced state."""
    from hnumo.engine import Engine
    e = Engine(case)
    q, qb, qp = e.state()
    e.set_resident(True)
    for _ in range(nsteps):
        e.ti_rk_bcl(q, qb, qp)
    dev = e.diagnostics()
    fields = e.layer_fields()
    e.sync(q, qb, qp)
    e.close()
    return dev, fields, q, qb


# bump10: N=4, L=2, uniform brick; qmbump8: general bilinear quadrilaterals; dg25N7L3 4x4: N=7
# (64-node elements, 49 sub-cells), 3 layers; bump10 at N=2: 9-node elements, the fewest nodes per
# element the engine supports (28 elements and 252 of 256 lanes per workgroup pass)
@pytest.mark.parametrize("name,kw", [("bump10", {}), ("qmbump8", {}), ("dg25N7L3", {"nelx": 4, "nely": 4}),
                                     ("bump10", {"nop": 2})])
def test_resident_diagnostics_equal_host(name, kw, case_factory):
    case = case_factory(name, **kw)
    if name == "qmbump8":
        # the config must exercise the running minimum: it keeps falling along the element order
        mdx, mdy = running_cell_minima(case)
        assert np.unique(mdx).size > 1 and np.unique(mdy).size > 1
        assert np.unique(mdx[case.scalars["ngl"] ** 2:]).size > 1     # beyond the first element too
    dev, fields, q, qb = resident_run(case)
    host, qf = host_diagnostics(case, q, qb)
    assert dev["qmax"].shape == (5, case.scalars["nlayers"])
    assert_same(dev, host, what=name)
    assert fields.shape == qf.shape and np.array_equal(fields, qf)


def test_two_rank_group_diagnostics(case_factory):
    """Two processor-face ranks of bump10 in a local exchange group, one step: each engine reports
    its own rank's numbers; combined as the reference's mpi_reduce combines them they are the
    single-rank engine's."""
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    from hnumo.facepart import face_partition
    case = case_factory("bump10")
    parts = [face_partition(case, 2, r, "block") for r in range(2)]
    engines = [Engine(p) for p in parts]
    local_group(engines)
    states = [e.state() for e in engines]
    group_ti_rk_bcl(engines, states)
    devs = [e.diagnostics() for e in engines]
    for r, (p, st, d) in enumerate(zip(parts, states, devs)):
        host, qf = host_diagnostics(p, st[0], st[1])
        assert_same(d, host, what=f"rank {r}")
        assert np.array_equal(engines[r].layer_fields(), qf)
    for e in engines:
        e.close()
    one = Engine(case)
    q, qb, qp = one.state()
    one.ti_rk_bcl(q, qb, qp)
    single = one.diagnostics()
    one.close()
    for k in ("qmax", "qbmax"):
        assert np.array_equal(np.maximum(devs[0][k], devs[1][k]), single[k]), k
    for k in ("qmin", "qbmin"):
        assert np.array_equal(np.minimum(devs[0][k], devs[1][k]), single[k]), k
    # two summation orders of npoin positive terms: each within npoin * 2**-53 relative of the
    # exact sum
    total = devs[0]["mass"] + devs[1]["mass"]
    bound = 2 * case.scalars["npoin"] * 2.0 ** -53
    assert np.all(np.abs(total - single["mass"]) <= bound * single["mass"]), (total, single["mass"])


def test_non_resident_engine_reports_its_last_output(case_factory):
    from hnumo.engine import Engine
    case = case_factory("bump10")
    e = Engine(case)
    q, qb, qp = e.state()
    e.ti_rk_bcl(q, qb, qp)
    dev = e.diagnostics()
    e.close()
    host, _ = host_diagnostics(case, q, qb)
    assert_same(dev, host)


def test_errors_and_mass_flag(case_factory):
    import ctypes as C
    from hnumo.engine import Engine, EngineError, lib
    case = case_factory("bump10")
    e = Engine(case)
    with pytest.raises(EngineError) as ei:
        e.diagnostics()                                   # no state on the device yet
    assert ei.value.code == 4 and lib().hnumo_last_error(e.h).decode().strip()
    q, qb, qp = e.state()
    e.ti_rk_bcl(q, qb, qp)
    L = case.scalars["nlayers"]
    for n in (12 + 11 * L - 1, 12 + 11 * (L + 1)):
        buf = np.zeros(12 + 11 * (L + 1))
        rc = lib().hnumo_diagnostics(e.h, 1, buf.ctypes.data_as(C.POINTER(C.c_double)), n)
        assert rc == 4 and lib().hnumo_last_error(e.h).decode().strip()
        assert not buf.any()                              # nothing written
    full, nomass = e.diagnostics(), e.diagnostics(mass=False)
    e.close()
    assert np.array_equal(nomass["mass"], np.zeros(L)) and np.all(full["mass"] > 0)
    assert_same(nomass, full, keys=[k for k in KEYS if k != "mass"])


def test_diagnostics_leave_the_stepping_undisturbed(case_factory):
    """The diagnostics are plain launches between the replays of the captured step (the persistent
    sub-cycle inside): a run that asks after every step ends on the bits of one that never asks."""
    from hnumo.engine import Engine
    case = case_factory("bump10")
    out = []
    for ask in (False, True):
        e = Engine(case)
        q, qb, qp = e.state()
        e.set_resident(True)
        for _ in range(4):
            e.ti_rk_bcl(q, qb, qp)
            if ask:
                e.diagnostics()
        e.sync(q, qb, qp)
        out.append((q, qb, qp, e.persistent_stats["aborts"], e.stage_path))
        e.close()
    for a, b in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(a, b)
    assert out[0][3] == out[1][3] and out[0][4] == out[1][4]


def test_time_loop_device_diagnostics_writes_the_same_text(case_factory, tmp_path):
    """5 steps of bump10 with a report and a snapshot every 2: stdout, mass_mlswe.cons and
    mlswe_FIN.txt are the same strings with the reports' numbers from the device as from the
    host (compared from the first report after a step on)."""
    from hnumo.engine import Engine
    case = case_factory("bump10")
    dt = case.scalars["dt"]
    got = {}
    for flag in (False, True):
        e = Engine(case)
        d = tmp_path / str(flag)
        buf = io.StringIO()
        D.time_loop(case, e, 5 * dt, out_dir=str(d), dump_data=True, time_restart=2 * dt, out=buf,
                    device_diagnostics=flag)
        e.close()
        text = buf.getvalue()
        rule = D._RULE + "\n"
        start = text.index(rule, text.index(rule) + 1) + len(rule)      # past the initial report
        cons = (d / "mass_mlswe.cons").read_text().splitlines()
        got[flag] = (text[start:], cons[1:], (d / "mlswe_FIN.txt").read_text())
    assert got[False][0].count("itime time dt dt_btp") == 3 and len(got[False][1]) == 2   # steps 2, 4, the end
    assert got[True][0] == got[False][0]
    assert got[True][1] == got[False][1]
    assert got[True][2] == got[False][2]
