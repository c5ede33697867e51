"""Migrating float sets, from the Python mirrors alone (hnumo.floats.HostFloatGroup against HostFloats on
the whole mesh): a float's record on the rank that holds it is the single-rank float's, bit for bit,
through any number of crossings.  tests/float_migrate_cases.py has the partitions and the seeds; the
conditions below keep the seeds from quietly ceasing to exercise a branch."""
import os
import re

import numpy as np
import pytest

import float_migrate_cases as MC
from hnumo import floats as FL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = ("hnumo_floats_migrate", "hnumo_floats_release", "hnumo_floats_outbox", "hnumo_floats_deliver", "hnumo_floats_settle")
GROUP = ("hnumo_group_floats_migrate", "hnumo_group_floats_advance")


@pytest.mark.parametrize("row", MC.ROWS, ids=MC.ROW_IDS)
def test_merged_group_series_equal_the_single_rank_series(case_factory, row):
    """coord_scale = the global max|coord| on every rank (the whole mesh's own): np.array_equal for every
    float and record, none left out."""
    run = MC.mirror_run(case_factory, row, scaled=True)
    one, grp, merged, ref = run["one"], run["group"], run["merged"], run["ref"]
    assert merged.shape == ref.shape == (5, one.M, MC.NADV)
    assert np.array_equal(merged, ref), int((merged != ref).sum())
    assert np.isfinite(ref).all()
    # after the lowest-rank rule every seed sits in the single-rank run's element, on one rank
    assert run["seed_elems_agree"]
    # the protocol's own promises
    assert not any((hf.status == FL.LOST).any() for hf in grp.ranks) and not (one.status == FL.LOST).any()
    assert grp.in_flight_after == 0 and 1 <= grp.max_rounds <= FL.MAXROUNDS
    # what the seeds must exercise
    M = one.M
    nchange = sum(1 for p in grp.path if len(p) >= 2)
    assert nchange >= 0.05 * M, (nchange, M)
    assert any(len(p) >= 3 and p[i] in p[:i] for p in grp.path for i in range(2, len(p)))       # back on a rank it left
    cross = [c for cs in grp.crossings for c in cs]
    assert {c[1] for c in cross} == {0, 1}                                                       # in both stages
    assert max(c[2] for c in cross) >= 2                                                         # a crossing after an owned hop
    if len(grp.ranks) == 4:
        # through three ranks within one advance: two crossings of one float in the same advance, to a third rank
        assert any(a[0] == b[0] and len({a[3], a[4], b[4]}) == 3 for cs in grp.crossings for a, b in zip(cs, cs[1:]))
    assert grp.shared.sum() >= 20                                                                # seeds on shared edges


@pytest.mark.parametrize("row", MC.ROWS, ids=MC.ROW_IDS)
def test_each_ranks_own_tolerance_gives_the_same_bits_on_these_seeds(case_factory, row):
    """An observation about these seeds, not a guarantee: with coord_scale = 0 every rank accepts on the
    threshold of its own max|coord|, and no location of these runs falls between two thresholds."""
    run = MC.mirror_run(case_factory, row, scaled=False)
    assert np.array_equal(run["merged"], run["ref"])
    tols = [hf.tol for hf in run["group"].ranks]
    glob = run["one"].tol
    if len(tols) == 4:                              # (the two block ranks both reach the domain's largest coordinate)
        assert any((t != glob[np.asarray(p.elems)]).any() for t, p in zip(tols, run["parts"]))     # the thresholds do differ


def test_coord_scale_replaces_max_coord_in_the_tolerance(case_factory):
    import float_cases as FC
    case = FC.moving(case_factory, *FC.CASES[1])
    xy = FL.seed_grid(case, 3, 3)
    hf = FL.HostFloats(case, xy, 1)
    own = hf.tol.copy()
    hf.set_coord_scale(2.0 * hf.maxc)
    assert np.array_equal(hf.tol, 2.0 * own)                     # (a power of two: exact)
    hf.set_coord_scale(0.0)
    assert np.array_equal(hf.tol, own)
    assert np.array_equal(FL.HostFloats(case, xy, 1, coord_scale=hf.maxc).tol, own)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            hf.set_coord_scale(bad)


def test_merge_series_takes_the_holder_and_refuses_two(case_factory):
    parts = MC.partition(case_factory, MC.ROWS[0])[1]
    a, b = np.zeros((5, 3, 2)), np.zeros((5, 3, 2))
    a[:, 0, 0] = [1.0, 2.0, 3.0, 4.0, 5.0]          # float 0 on rank 0 in record 0, on rank 1 in record 1
    b[:, 0, 1] = [6.0, 7.0, 8.0, 9.0, 2.0]
    a[0, 0, 1] = -1.0                               # (rank 0's stale slot is not taken)
    a[:, 1, :] = 11.0                               # float 1: never held: rank 0's
    a[4, 1, :] = 0.0
    b[:, 2, 0] = [1.0, 1.0, 1.0, 1.0, 1.0]          # float 2 on rank 1, then held by nobody: rank 1's still
    b[0:4, 2, 1] = 2.5
    m = FL.merge_series([a, b], parts)
    assert list(m[:, 0, 0]) == [1.0, 2.0, 3.0, 4.0, parts[0].elems[4] + 1.0]
    assert list(m[:, 0, 1]) == [6.0, 7.0, 8.0, 9.0, parts[1].elems[1] + 1.0]
    assert list(m[:, 1, 1]) == [11.0, 11.0, 11.0, 11.0, 0.0]
    assert list(m[:, 2, 1]) == [2.5, 2.5, 2.5, 2.5, 0.0]
    b[4, 0, 0] = 3.0
    with pytest.raises(ValueError):
        FL.merge_series([a, b], parts)


def test_header_fortran_module_and_python_declare_the_migration_calls():
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    f90 = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    py = open(os.path.join(REPO, "h-numo_amd", "hnumo", "engine.py")).read()
    public = re.search(r"public :: hnumo_engine_create.*?\n\s*\n", f90, re.S).group(0)
    for fn in ENGINE:
        assert re.search(r"\bint\s+%s\s*\(hnumo_engine \*eng" % fn, hdr), fn
        assert f"name='{fn}'" in f90, fn
        assert re.search(r"\b%s\b" % fn, public), fn
        assert re.search(r"def %s\(self" % fn[len("hnumo_"):], py), fn
        c_args = re.search(r"\bint\s+%s\s*\((.*?)\);" % fn, hdr, re.S).group(1).count(",") + 1
        py_args = re.search(r"L\.%s\.argtypes = \[(.*?)\]\n" % fn, py).group(1).count(",") + 1
        f_args = re.search(r"function %s\((.*?)\)" % fn, f90).group(1).count(",") + 1
        assert c_args == py_args == f_args, (fn, c_args, py_args, f_args)
    for fn in GROUP:                                 # (the group calls are C and Python only, as hnumo_group_ti_rk_bcl)
        c_args = re.search(r"\bint\s+%s\s*\(hnumo_engine \*\*engines,(.*?)\);" % fn, hdr, re.S).group(1).count(",") + 2
        py_args = re.search(r"L\.%s\.argtypes = \[(.*?)\]\n" % fn, py).group(1).count(",") + 1
        assert c_args == py_args, (fn, c_args, py_args)
        assert re.search(r"def %s\(engines" % fn[len("hnumo_"):], py), fn
    assert re.search(r"#define HNUMO_ABI_VERSION 10\b", hdr) and re.search(r"HNUMO_ABI_EXPECTED = 10\b", f90)
    assert "the host's job" not in hdr
