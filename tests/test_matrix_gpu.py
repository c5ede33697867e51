"""GPU parity over the matrix of tests/matrix.py: the engine against the CPU oracle, bit for bit,
on every cell -- N = 2, 3, 4, 5, 7 crossed with the layer families (a single layer among them), the
viscosity methods, the wall codes, the drag laws, the shear solve and the mesh kinds, from states
that move (tests/states.py) -- on both stage paths, the default one and one launch per stage
(HNUMO_PERSISTENT=0).  The oracle runs once per cell and is shared.

Every cell runs again through the device code of large meshes (matrix.VARIANTS): an engine of 2,048
owned elements or more launches the per-stage barotropic kernel in a LEAN arena (N = 4) and the
large-mesh layer mass / consistency kernels (every N), which the cells' 16 or 9 elements would never
reach.  The experiment knobs force them ("large": the 5-per-CU arena, all cells; "large-nb4": the
4-per-CU arena, the N = 4 cells), every run asserts through Engine.kernel_variants that the variant
is what launches, and the comparison is the same: the cell's oracle result, bit for bit.  The
threshold itself is checked on engines that take no step.

A cell with method_visc == 1 runs its Laplacian kernels between the stages, so its default path is
the per-stage one (engine.hip, use_persistent); every other cell must take the persistent path.

Per N, on a moving lake cell, the two halves of a step are compared on their own (create_rhs_btp
and predict), on the default kernels and on the large-mesh ones, which tells which half is wrong
when a cell fails: create_rhs_btp is the stage kernel alone, predict adds the mass / cons kernels.
On the moving single-layer lake the resident engine's diagnostics, layer fields and flow statistics
equal their host mirrors.

The processor-face halo carries a moving state too: five cells (N = 7 with one layer, N = 2, one
layer at N = 4, three layers at N = 3, N = 5) as 2-rank local groups against the reference Fortran
under mpiexec on the same partitions (tests/golden/matrix_mpi2_*.npz), every rank bit for bit -- on
the default kernels and on the large-mesh ones, which multi-rank engines run with the face kernels'
fluxes and, in the LEAN arena, with the two-stream schedule's launches that signal their own stop
event.  A 4x4 cell splits into two blocks; 3x3 elements do not, and split along the Morton curve."""
import numpy as np
import pytest

import matrix as M
from util import rel

pytestmark = pytest.mark.gpu
_oracle = {}


def oracle_of(cell, case):
    if cell["name"] not in _oracle:
        _oracle[cell["name"]] = M.run_oracle(case, cell["nsteps"])
    return _oracle[cell["name"]]


def first_difference(st, so, fields, ofields):
    """The first differing array (with layer and variable for the layer states) and its rel, or None."""
    for nm, a, b in zip(("q", "qb", "qprime"), st, so):
        if np.array_equal(a, b):
            continue
        if a.ndim == 3:
            for k in range(a.shape[2]):
                for v in range(a.shape[0]):
                    if not np.array_equal(a[v, :, k], b[v, :, k]):
                        return dict(array=nm, layer=k, variable=v, rel=rel(a[v, :, k], b[v, :, k]))
        for v in range(a.shape[0]):
            if not np.array_equal(a[v], b[v]):
                return dict(array=nm, variable=v, rel=rel(a[v], b[v]))
    for f in ofields:
        if not np.array_equal(fields[f], ofields[f]):
            return dict(array=f, rel=rel(fields[f], ofields[f]))
    return None


def variant_engines(variant, cases, monkeypatch):
    """Engines of ``cases`` created under a kernel variant's environment (None: none), each checked
    to launch that variant: the settings honoured, in the engine's order, and the kernels chosen."""
    from hnumo.engine import Engine
    env = M.variant_env(variant) if variant else {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    engines = []
    try:
        for c in cases:
            engines.append(Engine(c))
        for k in env:
            monkeypatch.delenv(k)
        for e in engines:
            N = e.dims["ngl"] - 1
            if variant:
                assert e.overrides == M.variant_overrides(variant), e.overrides
                assert not any("ignored" in x for x in e.overrides)
                assert e.stage_path == "per-stage"
                assert e.kernel_variants == M.variant_kernels(variant, N), (variant, N, e.kernel_variants)
            else:
                assert e.overrides == [] and e.kernel_variants == dict(stage_arena=0, bcl_big=False)
    except BaseException:
        for e in engines:
            e.close()
        raise
    return engines


# (name, path): every cell on the two stage paths and through the large-mesh kernel variants
CELL_RUNS = [(c["name"], p) for c in M.CELLS for p in ("default", "per-stage")] + \
            [(c["name"], v) for v in M.VARIANTS for c in M.variant_cells(v)]


@pytest.mark.parametrize("name,path", CELL_RUNS, ids=["-".join(r) for r in CELL_RUNS])
def test_cell_matches_oracle_bitwise(name, path, case_factory, monkeypatch):
    from hnumo import bundle as B
    from hnumo.engine import Engine
    cell = M.BY_NAME[name]
    case = M.cell_case(cell, case_factory)
    so, ofields = oracle_of(cell, case)
    assert all(np.isfinite(x).all() for x in so)
    if path in M.VARIANTS:
        e, = variant_engines(path, [case], monkeypatch)
    else:
        if path == "per-stage":
            monkeypatch.setenv("HNUMO_PERSISTENT", "0")
        e = Engine(case)
        monkeypatch.delenv("HNUMO_PERSISTENT", raising=False)
    try:
        want = "per-stage" if path != "default" or cell["visc"] == 1 else "persistent"
        assert e.stage_path == want, (e.stage_path, want)
        if path == "default":
            assert e.kernel_variants == dict(stage_arena=0, bcl_big=False)
        st = e.state()
        assert np.array_equal(st[0], case.arrays["q_df"])
        for _ in range(cell["nsteps"]):
            e.ti_rk_bcl(*st)
        fields = {f: e.field(f) for f, _ in B.FIELDS}
    finally:
        e.close()
    assert first_difference(st, so, fields, ofields) is None


def _moving_lake(N, family=None):
    return next(c for c in M.CELLS if c["N"] == N and c["state"] == "moving" and c["family"].startswith("lake")
                and (family is None or c["family"] == family))


@pytest.mark.parametrize("kw,want", [(dict(nelx=32, nely=64), (5, True)), (dict(nelx=23, nely=89), (0, False)),
                                     (dict(nop=3, nelx=32, nely=64), (0, True))],
                         ids=["2048", "2047", "2048-N3"])
def test_large_mesh_kernels_start_at_2048_elements(kw, want, case_factory):
    """The default choice at the threshold itself (engine.hip, read_knobs), on engines that take no step."""
    from hnumo.engine import Engine
    case = case_factory("lake10", **kw)
    assert case.scalars["nelem"] == kw["nelx"] * kw["nely"] and case.scalars["nelem"] in (2047, 2048)
    e = Engine(case)
    try:
        assert e.overrides == []
        assert e.kernel_variants == dict(stage_arena=want[0], bcl_big=want[1]), e.kernel_variants
    finally:
        e.close()


HALF_RUNS = [(N, None) for N in M.LEVELS["N"]] + [(N, "large") for N in M.LEVELS["N"]]


@pytest.mark.parametrize("N,variant", HALF_RUNS, ids=[str(N) + ("-" + v if v else "") for N, v in HALF_RUNS])
def test_step_halves_match_oracle_bitwise(N, variant, case_factory, monkeypatch):
    """create_rhs_btp and predict on a moving lake cell of every N, on the default kernels and the
    large-mesh ones."""
    import oracle as O
    case = M.cell_case(_moving_lake(N), case_factory)
    o = O.Oracle(case)
    e, = variant_engines(variant, [case], monkeypatch)
    try:
        q, qb, qp = o.state()
        o.btp_bcl_coeffs(qp)
        r_o = o.create_rhs_btp(qb, qp)
        e.btp_bcl_coeffs(qp)
        r_e = e.create_rhs_btp(qb, qp)
        assert np.abs(r_o[1:]).max() > 0.0
        for v in range(3):
            assert np.array_equal(r_e[v], r_o[v]), ("create_rhs_btp", v, rel(r_e[v], r_o[v]))
        so, se = o.state(), e.state()
        o.predict(*so)
        e.predict(*se)
        assert first_difference(se, so, {}, {}) is None
    finally:
        e.close()


def test_single_layer_diagnostics_and_statistics_equal_host(case_factory):
    """L = 1, moving: the resident engine's diagnostics(), layer_fields() and flow statistics against
    the host mirrors (as tests/test_devdiag_gpu.py and tests/test_flowstats_gpu.py do for L >= 2)."""
    from hnumo import flowstats as F
    from hnumo.engine import Engine
    from test_devdiag_gpu import KEYS, assert_same, host_diagnostics
    cell = _moving_lake(4, "lake1")
    case = M.cell_case(cell, case_factory)
    assert case.scalars["nlayers"] == 1
    # the per-step states, from a non-resident engine
    e = Engine(case)
    q, qb, qp = e.state()
    steps = []
    for _ in range(cell["nsteps"]):
        e.ti_rk_bcl(q, qb, qp)
        steps.append(q.copy(order="F"))
    e.close()
    e = Engine(case)
    try:
        r = e.state()
        e.set_resident(True)
        st = F.DeviceFlowStats(e, every=0, series=len(steps))
        for _ in steps:
            e.ti_rk_bcl(*r)
            st.add()
        dev, lf = e.diagnostics(), e.layer_fields()
        sums, n, fields, series = st.sums, st.nsamples, st.fields(), st.series
        e.sync(*r)
    finally:
        e.close()
    assert np.array_equal(r[0], q) and np.array_equal(r[1], qb)
    host, qf = host_diagnostics(case, r[0], r[1])
    assert_same(dev, host, KEYS, cell["name"])
    assert np.array_equal(lf, qf)
    hs = F.HostFlowStats(case)
    for s in steps:
        hs.add(s)
    assert n == hs.nsamples and np.array_equal(sums, hs.sums)
    assert np.array_equal(fields, hs.fields()) and np.array_equal(series, hs.series)


HALO_RUNS = [(n, None) for n in M.HALO_CELLS] + [(n, "large") for n in M.HALO_CELLS]


@pytest.mark.parametrize("name,variant", HALO_RUNS, ids=[n + ("-" + v if v else "") for n, v in HALO_RUNS])
def test_face_halo_moving_matches_reference_mpi(name, variant, monkeypatch):
    import json
    import os
    import states
    from util import overrides_of
    from hnumo.case import build_case, make_config
    from hnumo.engine import group_ti_rk_bcl, local_group
    from hnumo.facepart import face_partition
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrix_mpi2_" + name + ".npz")
    g = dict(np.load(gold, allow_pickle=False))
    case = build_case(make_config(str(g["config"]), **overrides_of(g)), dense=False)
    case = states.moving_case(case, **json.loads(str(g["state_params"])))
    R = int(g["nranks"])
    parts = [face_partition(case, R, r, str(g["order"])) for r in range(R)]
    assert all(not np.array_equal(p.arrays["q_df"][1], 0.0 * p.arrays["q_df"][1]) for p in parts)
    engines = variant_engines(variant, parts, monkeypatch)
    try:
        local_group(engines)
        sts = [e.state() for e in engines]
        for _ in range(int(g["nsteps"])):
            group_ti_rk_bcl(engines, sts)
    finally:
        for e in engines:
            e.close()
    for r, st in enumerate(sts):
        for k, a in zip(("q_df", "qb_df", "qprime_df"), st):
            ref = g[f"{k}_r{r}"]
            assert np.array_equal(a, ref), (name, r, k, rel(a, ref))
