"""CPU tests of the parity matrix (tests/matrix.py) and of the state builder (tests/states.py).

The admissibility conditions are computed from the state alone, with numpy, from the case's
imapl / imapr / face / normal_vector -- neither the oracle nor the engine is asked -- and show
that a moving state is not secretly at rest or continuous, for every moving cell and every layer:

  (a) on the interior faces both signs of the normal velocity occur on at least a quarter of the
      face nodes each, and likewise both signs of the tangential velocity;
  (b) the left and right thickness traces differ at every interior face node;
  (c) on every interior face there is a node at which layer k of one side overlaps layer k+1 or
      k-1 of the other by more than 1e-6 of the thinner of the two (interfaces stacked on the
      bottom from the thicknesses, as the layer-overlap pressure of the face kernel stacks them);
      a single layer has no such neighbour, so the condition is empty at L = 1;
  (d) every thickness is positive, and the oracle runs the cell's steps with return code 0 and a
      finite state.
These are conditions, not tolerances."""
import numpy as np
import pytest

import matrix as M
import states

MOVING = [c["name"] for c in M.CELLS if c["state"] == "moving"]


def test_matrix_covers_every_pair():
    assert 25 <= len(M.CELLS) <= 35 and len(M.BY_NAME) == len(M.CELLS)
    assert M.missing_pairs(M.CELLS) == []
    assert M.missing_levels(M.CELLS) == []
    # the assertion bites: without its last N = 7 row or its single-layer rows the list is thinner
    assert M.missing_pairs([c for c in M.CELLS if c["family"] != "lake1"])
    assert M.missing_pairs([c for c in M.CELLS if c["N"] != 7])
    assert sum(c["state"] == "rest" for c in M.CELLS) <= 6


def test_kernel_variants_see_every_level():
    """The LEAN arenas exist at N = 4 only, so the N = 4 rows are all that "large-nb4" (and the arena
    of "large") can see: they hold every level of every other factor."""
    assert set(M.VARIANTS) == {"large", "large-nb4"}
    assert M.variant_cells("large") == M.CELLS
    nb4 = M.variant_cells("large-nb4")
    assert nb4 == [c for c in M.CELLS if c["N"] == 4] and len(nb4) >= 6
    assert M.missing_levels_of(nb4) == []
    # the assertion bites: a thinner list lacks a level
    assert M.missing_levels_of([c for c in nb4 if c["state"] == "moving"])
    assert M.missing_levels_of([c for c in nb4 if c["shear"] == 0])
    for v, (env, _) in M.VARIANTS.items():
        assert env["HNUMO_EXPERIMENTS"] == "1" and env["HNUMO_PERSISTENT"] == "0" and env["HNUMO_BCL_BIG"] == "1"
        assert M.variant_overrides(v) == ["HNUMO_STAGE_NB=" + env["HNUMO_STAGE_NB"], "HNUMO_BCL_BIG=1",
                                          "HNUMO_PERSISTENT=0"]
    assert M.variant_kernels("large", 4) == dict(stage_arena=5, bcl_big=True)
    assert M.variant_kernels("large-nb4", 4) == dict(stage_arena=4, bcl_big=True)
    assert all(M.variant_kernels("large", N) == dict(stage_arena=0, bcl_big=True) for N in (2, 3, 5, 7))


@pytest.mark.parametrize("name", [c["name"] for c in M.CELLS])
def test_cell_sizes_and_time_steps(name, case_factory):
    from hnumo.case import CONFIGS
    cell = M.BY_NAME[name]
    base, ov = M.cell_config(cell)
    case = case_factory(base, **ov)
    S = case.scalars
    assert S["nelem"] == (16 if cell["N"] <= 4 else 9) and S["ngl"] == cell["N"] + 1
    assert S["nlayers"] == M.FAMILY[cell["family"]][1]
    assert cell["nsteps"] == (1 if cell["N"] == 7 else 2)
    b = CONFIGS[base]
    assert S["N_btp"] == int(np.ceil(b["dt"] / b["dt_btp"]))


def _traces(case, a):
    """(left, right) traces (ngl, ninterior) of a nodal array on the interior faces."""
    A, S = case.arrays, case.scalars
    ngl, P = S["ngl"], S["ngl"] ** 2
    face = np.asarray(A["face"]).astype(np.int64)
    inter = np.flatnonzero(face[7] > 0)
    el, er = face[6, inter] - 1, face[7, inter] - 1
    il, ir = np.asarray(A["imapl"]).astype(np.int64)[:, :, inter], np.asarray(A["imapr"]).astype(np.int64)[:, :, inter]
    Il = el[None, :] * P + (il[1] - 1) * ngl + il[0] - 1
    Ir = er[None, :] * P + (ir[1] - 1) * ngl + ir[0] - 1
    return a[Il], a[Ir], inter


@pytest.mark.parametrize("name", MOVING)
def test_moving_state_is_admissible(name, case_factory):
    cell = M.BY_NAME[name]
    case = M.cell_case(cell, case_factory)
    A, S = case.arrays, case.scalars
    L, g, alpha = S["nlayers"], S["gravity"], np.asarray(A["alpha"])
    q = np.asarray(A["q_df"])
    assert (q[0] > 0.0).all()                                                     # (d), first half
    hl, hr, zl, zr = [], [], None, None
    for k in range(L):
        dl, dr, inter = _traces(case, q[0, :, k])
        assert (dl != dr).all(), ("b", k)                                          # (b)
        hl.append(dl)
        hr.append(dr)
        nv = np.asarray(A["normal_vector"])[:, :, inter]
        for side in (0, 1):
            u = _traces(case, q[1, :, k] / q[0, :, k])[side]
            v = _traces(case, q[2, :, k] / q[0, :, k])[side]
            un, ut = u * nv[0] + v * nv[1], -u * nv[1] + v * nv[0]
            for nm, w in (("normal", un), ("tangential", ut)):
                assert (w > 0.0).mean() >= 0.25 and (w < 0.0).mean() >= 0.25, ("a", k, side, nm)   # (a)
    # (c): interfaces z_L = zbot, z_{k-1} = z_k + (alpha_k / g) dp_k on either side
    zbl, zbr, _ = _traces(case, np.asarray(A["zbot_df"]))
    zl, zr = [None] * (L + 1), [None] * (L + 1)
    zl[L], zr[L] = zbl, zbr
    for k in range(L, 0, -1):
        zl[k - 1] = zl[k] + alpha[k - 1] / g * hl[k - 1]
        zr[k - 1] = zr[k] + alpha[k - 1] / g * hr[k - 1]
    for k in range(L):
        found = np.zeros(zbl.shape, dtype=bool)
        for (za, zb) in ((zl, zr), (zr, zl)):
            for kt in (k - 1, k + 1):
                if 0 <= kt < L:
                    ov = np.minimum(za[k], zb[kt]) - np.maximum(za[k + 1], zb[kt + 1])
                    thin = np.minimum(za[k] - za[k + 1], zb[kt] - zb[kt + 1])
                    found |= ov > 1e-6 * thin
        if L > 1:
            assert found.any(axis=0).all(), ("c", k)                               # (c)
    (qo, qbo, qpo), _ = M.run_oracle(case, cell["nsteps"])                         # (d): raises on rc != 0
    assert np.isfinite(qo).all() and np.isfinite(qbo).all() and np.isfinite(qpo).all()
    assert (qo[0] > 0.0).all()


def test_with_state_leaves_the_case_alone(case_factory):
    cell = M.BY_NAME[MOVING[0]]
    base, ov = M.cell_config(cell)
    case = case_factory(base, **ov)
    q0 = np.array(case.arrays["q_df"])
    mc = states.moving_case(case)
    assert np.array_equal(case.arrays["q_df"], q0) and not np.array_equal(mc.arrays["q_df"], q0)
    assert mc.arrays["face"] is case.arrays["face"] and mc.arrays["q_df"].flags["F_CONTIGUOUS"]
    q, qb, qp = states.moving_state(case, **states.DEFAULT)
    assert np.array_equal(qb[1], qb[0] - case.arrays["pbprime_df"])
