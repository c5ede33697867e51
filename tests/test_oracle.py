"""CPU tests: the oracle (C restatement) against the reference's golden vectors and, where
the reference harness can be built (oracle/_ref), against the reference Fortran itself."""
import hashlib
import os
import tempfile

import numpy as np
import pytest

from util import layer_mass

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
GOLDEN = ["bump10_rhs", "bump10_btp", "bump10_step2", "lake10_step1", "dg25_step1", "dg25L3_step1",
          "bump10q_step1", "dg8L3q_step1", "dg8N7L3_step1", "bump10_b2ns_step1", "bump10_mixed_step1",
          "lake10L3_step1", "bump10q_ns_step1", "dg8L3q_mixed_step1", "qmbump8_step2", "qmdg8L3_step1", "bump16_step1",
          "dg25N7L3_step1"]


def load(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False))


def golden_case(g, case_factory):
    from util import overrides_of
    return case_factory(str(g["config"]), **overrides_of(g))


def bundle_hash(case, mode, nsteps):
    from hnumo import bundle as B
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "b.bin")
        B.write_bundle(p, case, mode, nsteps)
        return hashlib.sha256(open(p, "rb").read()).hexdigest()


@pytest.mark.parametrize("fixture,nop", [("bump10_rhs", 4), ("dg8N7L3_step1", 7)])
def test_basis_matches_reference_bitwise(fixture, nop):
    """LGL nodes/weights and the interpolation/derivative tables equal the reference's
    mod_basis_create output (mod_basis.F90:60-186) bit for bit, at N=4 and N=7."""
    from hnumo.basis import Basis
    g = load(fixture)
    b = Basis(nop)
    for k, v in [("xgl", b.xgl), ("wgl", b.wgl), ("xnq", b.xnq), ("wnq", b.wnq), ("psiq", b.psiq),
                 ("dpsiq", b.dpsiq), ("dpsi", b.dpsi)]:
        assert np.array_equal(g["ref_" + k], v), k


@pytest.mark.parametrize("name", GOLDEN)
def test_oracle_matches_golden(name, case_factory):
    import oracle as O
    g = load(name)
    mode, nsteps, stride = str(g["mode"]), int(g["nsteps"]), int(g["stride"])
    case = golden_case(g, case_factory)
    assert bundle_hash(case, mode, nsteps) == str(g["bundle_sha256"]), "setup inputs changed: regenerate golden"
    o = O.Oracle(case)
    q, qb, qp = o.state()
    if mode == "rhs":
        o.btp_bcl_coeffs(qp)
        rhs = o.create_rhs_btp(qb, qp)
        assert np.array_equal(rhs, g["rhs"])
    elif mode == "btp":
        o.btp_bcl_coeffs(qp)
        o.ti_barotropic_ssprk(qb, qp)
    else:
        for _ in range(nsteps):
            o.ti_rk_bcl(q, qb, qp)
        assert np.array_equal(q[:, ::stride, :], g["q_df"])
        assert np.array_equal(qp[:, ::stride, :], g["qprime_df"])
    assert np.array_equal(qb[:, ::stride], g["qb_df"])
    from util import state_sha256
    for k, a in (("q_df", q), ("qb_df", qb), ("qprime_df", qp)):
        if k + "_sha256" in g:        # strided fixtures: the whole state, bit for bit
            assert state_sha256(a) == str(g[k + "_sha256"]), k
    for k in g:
        if k.startswith("field_"):
            a = o.field(k[6:]).reshape(-1, order="F")[::stride]
            assert np.array_equal(a, g[k]), k


@pytest.mark.ref
@pytest.mark.parametrize("variant", [
    dict(name="bump10", botfr=2, cd=1e-3, visc=25.0, method_visc=3, y_boundary=(2, 2)),
    dict(name="bump10", botfr=1, cd=1e-7, f0=1e-4, beta=1e-11, x_boundary=(2, 4)),
    dict(name="lake10", nlayers=3),
    dict(name="bump10q", y_boundary=(2, 2), botfr=2, cd=1e-3),   # quad-point LDG + no-slip walls
    dict(name="dg8L3q", x_boundary=(2, 4)),                       # 3 layers, wind, drag, mixed walls
])
def test_oracle_matches_reference_fortran(variant):
    """Branches the shipped configs do not exercise (quadratic drag, no-slip walls, mixed
    BCs, 3-layer lake): oracle vs the reference Fortran, bitwise, 1 baroclinic step."""
    import oracle as O
    from hnumo.case import build_case, make_config
    v = dict(variant)
    case = build_case(make_config(v.pop("name"), **v))
    ref = O.run_reference(case, "step", 1)
    o = O.Oracle(case)
    q, qb, qp = o.state()
    o.ti_rk_bcl(q, qb, qp)
    for k, a in [("q_df", q), ("qb_df", qb), ("qprime_df", qp)]:
        assert np.array_equal(a, ref[k]), k


@pytest.mark.ref
@pytest.mark.parametrize("name", ["bump10s", "dg8L3s"])
def test_shear_predictor_vs_reference_fortran(name, case_factory):
    """ad_mlswe > 0: the predictor (momentum_mass with the implicit vertical shear stress,
    mod_splitting.F90:182-287) against the reference Fortran (ref_driver mode 4), bit for bit.
    rhs_layer_shear_stress reads tau_u(nlayers+1) and tau_v(nlayers+1), which it never assigns
    (mod_create_rhs_mlswe.F90:160,246-258); the reference build's -finit-real=zero makes them 0.
    amdflang has no such flag, so the harness links the routine through a wrapper that
    zero-fills the stack its frame is about to occupy (oracle/zero_init_wrap.c, -Wl,--wrap)."""
    import oracle as O
    case = case_factory(name)
    ref = O.run_reference(case, "predict", 1)
    o = O.Oracle(case)
    q, qb, qp = o.state()
    o.predict(q, qb, qp)
    for k, a in [("q_df", q), ("qb_df", qb), ("qprime_df", qp)]:
        assert np.array_equal(a, ref[k]), k


@pytest.mark.parametrize("name", ["bump10s_predict", "dg8L3s_predict"])
def test_shear_predictor_golden(name, case_factory):
    """The same on the committed fixtures (no reference build needed)."""
    import oracle as O
    from util import overrides_of
    g = dict(np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False))
    case = case_factory(str(g["config"]), **overrides_of(g))
    assert bundle_hash(case, "predict", 1) == str(g["bundle_sha256"]), "setup inputs changed: regenerate golden"
    o = O.Oracle(case)
    q, qb, qp = o.state()
    o.predict(q, qb, qp)
    assert np.array_equal(q, g["q_df"]) and np.array_equal(qb, g["qb_df"]) and np.array_equal(qp, g["qprime_df"])


def _matrix_cells():
    import matrix as M
    return [c["name"] for c in M.CELLS]


def _matrix_oracle(cell, case):
    """(mode, nsteps, oracle state) of a matrix cell: its steps, or -- with ad_mlswe > 0, where the
    reference's own corrector is not finite (test_shear_predictor_vs_reference_fortran) -- the
    predictor."""
    import oracle as O
    mode, nsteps = ("predict", 1) if cell["shear"] else ("step", cell["nsteps"])
    o = O.Oracle(case)
    st = o.state()
    if mode == "predict":
        o.predict(*st)
    else:
        for _ in range(nsteps):
            o.ti_rk_bcl(*st)
    return mode, nsteps, st


@pytest.mark.ref
@pytest.mark.parametrize("name", _matrix_cells())
def test_matrix_oracle_matches_reference_fortran(name, case_factory):
    """Every cell of tests/matrix.py -- N = 2, 3, 4, 5, 7, one to three layers, every feature branch,
    from states that move (tests/states.py) -- oracle vs the reference Fortran, bit for bit."""
    import matrix as M
    import oracle as O
    cell = M.BY_NAME[name]
    case = M.cell_case(cell, case_factory)
    mode, nsteps, st = _matrix_oracle(cell, case)
    ref = O.run_reference(case, mode, nsteps)
    for k, a in zip(("q_df", "qb_df", "qprime_df"), st):
        assert np.isfinite(ref[k]).all(), k
        assert np.array_equal(a, ref[k]), k


@pytest.mark.parametrize("name", _matrix_cells())
def test_matrix_oracle_matches_golden(name, case_factory):
    """The same on the committed fixtures (tests/golden/matrix_*.npz, make_golden.py matrix): the
    state is rebuilt from the stored moving_state parameters and its bundle hash checked."""
    import matrix as M
    import states
    import json
    from util import overrides_of
    cell = M.BY_NAME[name]
    g = load("matrix_" + name)
    case = case_factory(str(g["config"]), **overrides_of(g))
    if str(g["state"]) == "moving":
        case = states.moving_case(case, **json.loads(str(g["state_params"])))
    mode, nsteps, st = _matrix_oracle(cell, case)
    assert (mode, nsteps) == (str(g["mode"]), int(g["nsteps"]))
    assert bundle_hash(case, mode, nsteps) == str(g["bundle_sha256"]), "setup inputs changed: regenerate golden"
    for k, a in zip(("q_df", "qb_df", "qprime_df"), st):
        assert np.isfinite(g[k]).all(), k
        assert np.array_equal(a, g[k]), k


def _halo_cells():
    import matrix as M
    return list(M.HALO_CELLS)


@pytest.mark.parametrize("name", _halo_cells())
def test_matrix_mpi_fixtures_are_current(name, case_factory):
    """The 2-rank fixtures of the moving halo cells (read by tests/test_matrix_gpu.py) were made from
    the inputs the partitioner builds today: every rank's bundle hash."""
    import json
    import states
    from util import overrides_of
    from hnumo.facepart import face_partition
    g = load("matrix_mpi2_" + name)
    case = states.moving_case(case_factory(str(g["config"]), **overrides_of(g)), **json.loads(str(g["state_params"])))
    for r in range(int(g["nranks"])):
        pc = face_partition(case, int(g["nranks"]), r, str(g["order"]))
        assert bundle_hash(pc, "step", int(g["nsteps"])) == str(g[f"bundle_sha256_r{r}"]), r


def test_shear_branch_is_live(case_factory):
    """ad_mlswe > 0 changes the predicted layer momenta (and only them)."""
    import oracle as O
    out = []
    for ad in (1.0e-2, 0.0):
        o = O.Oracle(case_factory("bump10s", ad_mlswe=ad))
        q, qb, qp = o.state()
        o.predict(q, qb, qp)
        out.append((q.copy(), qb.copy()))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0][0], out[1][0][0])
    assert not np.array_equal(out[0][0][1:], out[1][0][1:])


def test_bump_mass_conservation(case_factory):
    """The reference's only CI assertion: per-layer mass loss <= 1e-12 (CI/bump/check.F90:58)."""
    import oracle as O
    case = case_factory("bump10")
    o = O.Oracle(case)
    q, qb, qp = o.state()
    m0 = layer_mass(case, q)
    for _ in range(2):
        o.ti_rk_bcl(q, qb, qp)
    loss = np.abs(layer_mass(case, q) - m0) / m0
    assert (loss <= 1e-12).all(), loss


def test_lake_at_rest_is_well_balanced(case_factory):
    import oracle as O
    case = case_factory("lake10")
    o = O.Oracle(case)
    q, qb, qp = o.state()
    o.ti_rk_bcl(q, qb, qp)
    assert np.abs(qb[2:4]).max() < 1e-6 * np.abs(qb[0]).max()


def test_quad_ldg_branch_is_live(case_factory):
    """method_visc == 1 (quad-point LDG, mod_laplacian_quad.F90:125-223,252-355) takes its own
    path: the state after one step differs from the nodal-LDG run of the same case."""
    import oracle as O
    out = []
    for mv in (1, 3):
        case = case_factory("bump10q", method_visc=mv)
        o = O.Oracle(case)
        q, qb, qp = o.state()
        o.ti_rk_bcl(q, qb, qp)
        out.append(qb.copy())
    assert not np.array_equal(out[0], out[1])
