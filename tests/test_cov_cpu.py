"""Eddy covariances (hnumo_cov_*, hnumo/covariance.py), the parts that need no GPU: the declarations on
both sides of the boundary, the numpy mirror HostEddyCov on the CPU oracle's moving states
(tests/states.py), and time_loop's eddy_cov hook.  Every comparison is np.array_equal unless it states
its bound."""
import io
import os
import re

import numpy as np
import pytest

import states
from hnumo import covariance as CV
from hnumo import diagnostics as D
from hnumo import flowstats as F
from hnumo import sample as S
from hnumo import vorticity as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hnumo_cov_begin", "hnumo_cov_accumulate", "hnumo_cov_sums", "hnumo_cov_set_sums", "hnumo_cov_fields",
       "hnumo_cov_integrals", "hnumo_cov_end")
CASES = [("bump10", {"nop": 2}, 3), ("dg25L3", {"nelx": 5, "nely": 3}, 4)]
EPS = float(np.finfo(np.float64).eps)
_states = {}


def test_header_fortran_module_and_python_declare_the_covariances():
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    f90 = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    py = open(os.path.join(REPO, "h-numo_amd", "hnumo", "engine.py")).read()
    abi = open(os.path.join(REPO, "h-numo_amd", "hnumo", "abi.py")).read()
    public = re.search(r"public :: hnumo_engine_create.*?\n\s*\n", f90, re.S).group(0)
    for fn in NEW:
        assert re.search(r"\bint\s+%s\s*\(hnumo_engine \*eng" % fn, hdr), fn
        assert f"name='{fn}'" in f90, fn
        assert re.search(r"\b%s\b" % fn, public), fn
        assert f"L.{fn}.argtypes" in abi, fn
        assert re.search(r"def %s\(self" % fn[len("hnumo_"):], py), fn
    assert re.search(r"#define HNUMO_SAMPLE_COV 3\b", hdr) and re.search(r"HNUMO_SAMPLE_COV = 3\b", f90)
    assert S.COV == 3 and S.source_id("cov") == 3 and S.nval(3, "cov") == 48
    assert re.search(r"#define HNUMO_ABI_VERSION 10\b", hdr)      # additive: the version stays
    assert re.search(r"HNUMO_ABI_EXPECTED = 10\b", f90)
    assert len(CV.SUM_NAMES) == CV.NSUM == 14 and len(CV.FIELD_NAMES) == CV.NFIELD == 16


def oracle_states(case_factory, name, kw, nsteps):
    """(the moving case, the CPU oracle's states after steps 1..nsteps of it), computed once."""
    key = (name, tuple(sorted(kw.items())), nsteps)
    if key not in _states:
        import oracle as O
        case = states.moving_case(case_factory(name, **kw))
        o = O.Oracle(case)
        q, qb, qp = o.state()
        out = []
        for _ in range(nsteps):
            o.ti_rk_bcl(q, qb, qp)
            out.append(q.copy(order="F"))
        assert all(np.isfinite(x).all() for x in out)
        _states[key] = (case, out)
    return _states[key]


def mirror(case, qs, **kw):
    cv = CV.HostEddyCov(case, **kw)
    for q in qs:
        cv.add(q)
    return cv


@pytest.mark.parametrize("name,kw,nsteps", CASES)
def test_sums_are_the_definitions(case_factory, name, kw, nsteps):
    """Every sum restated from layer_fields and HostVorticity.fields, added in sample order."""
    case, qs = oracle_states(case_factory, name, kw, nsteps)
    zref = CV.rest_elevations(case_factory(name, **kw))
    cv = mirror(case, qs, zref=zref)
    sums, n = cv.sums()
    L, npoin = case.scalars["nlayers"], case.scalars["npoin"]
    assert n == nsteps and sums.shape == (14, npoin, L)
    f = V.coriolis_of(case)[:, None]
    want = np.zeros_like(sums)
    for q in qs:
        lf, vf = D.layer_fields(case, q), V.HostVorticity(case).fields(q)
        h, u, v, d = lf[0], lf[1], lf[2], lf[4] - zref
        a = vf[0] + f
        for c, x in enumerate((h, u, v, u * h, v * h, (u * u) * h, (u * v) * h, (v * v) * h, d, d * d, a, u * a, v * a,
                               vf[2] * a)):
            want[c] = want[c] + x
    assert np.array_equal(sums, want)
    fl = cv.fields()
    assert fl.shape == (16, npoin, L) and np.isfinite(fl).all()
    assert np.array_equal(fl[12], sums[10] / sums[0])            # qm: the thickness-weighted mean PV (h*pv = a)


@pytest.mark.parametrize("name,kw,nsteps", CASES)
def test_bounds_against_the_flow_statistics(case_factory, name, kw, nsteps):
    """Half the trace of the Reynolds stresses is the EKE of HostFlowStats on the same samples; the
    tensor is positive semi-definite and the variance non-negative, each to the rounding bound of a
    quotient of sums of n same-sign terms (good to (n+2) eps each; um^2 + vm^2 <= 2 mke)."""
    case, qs = oracle_states(case_factory, name, kw, nsteps)
    cv = mirror(case, qs)
    st = F.HostFlowStats(case, series=False)
    for q in qs:
        st.add(q)
    fl, sf = cv.fields(), st.fields()
    n = nsteps
    Ruu, Ruv, Rvv, dvar = fl[5], fl[6], fl[7], fl[11]
    eke, mke = sf[4], sf[3]
    c = 8 * (n + 4) * EPS * mke
    assert (mke >= 0).all() and mke.max() > 0              # (mke is 0 at nodes where the velocity is: c = 0, equality)
    assert (np.abs(0.5 * (Ruu + Rvv) - eke) <= c).all()
    assert (Ruu >= -c).all() and (Rvv >= -c).all()
    assert (Ruv * Ruv <= (Ruu + c) * (Rvv + c)).all()
    sums = cv.sums()[0]
    assert (dvar >= -8 * (n + 4) * EPS * (sums[9] / float(n)).max()).all()
    # the means both observers hold are the same statements
    assert np.array_equal(fl[0], sf[0]) and np.array_equal(fl[3], sf[1]) and np.array_equal(fl[4], sf[2])
    # the moving state does fluctuate: the stresses are not rounding noise
    assert (0.5 * (Ruu + Rvv)).max() > 1e3 * c.max()


@pytest.mark.parametrize("name,kw,nsteps", CASES)
def test_zref_of_the_first_sample_gives_exact_zeros(case_factory, name, kw, nsteps):
    case, qs = oracle_states(case_factory, name, kw, nsteps)
    cv = mirror(case, qs[:1], zref=CV.elevations(case, qs[0]))
    fl = cv.fields()
    assert np.array_equal(fl[10], np.zeros_like(fl[10])) and np.array_equal(fl[11], np.zeros_like(fl[11]))
    assert not np.signbit(fl[10]).any() and not np.signbit(fl[11]).any()
    # without it the interior interfaces sit at their depth
    far = mirror(case, qs[:1]).fields()
    assert np.abs(far[10][:, -1]).min() > 1.0


@pytest.mark.parametrize("name,kw,nsteps", CASES)
def test_integrals_equal_the_chunked_tree(case_factory, name, kw, nsteps):
    case, qs = oracle_states(case_factory, name, kw, nsteps)
    cv = mirror(case, qs, zref=CV.rest_elevations(case_factory(name, **kw)))
    got, el, fl = cv.integrals(), cv.element_sums(), cv.fields()
    L, ne, P = case.scalars["nlayers"], case.scalars["nelem"], case.scalars["ngl"] ** 2
    assert got.shape == (3, L) and el.shape == (3, L, ne) and np.isfinite(got).all()
    w = np.asarray(case.arrays["jac"]).reshape(-1, order="F")
    for k in range(L):
        x = (fl[0, :, k] * (0.5 * (fl[5, :, k] + fl[7, :, k])), fl[11, :, k], fl[0, :, k] * fl[15, :, k])
        for c in range(3):
            # per element the products in node order from the first one
            for e in (0, ne - 1):
                s = w[e * P] * x[c][e * P]
                for i in range(1, P):
                    s = s + w[e * P + i] * x[c][e * P + i]
                assert el[c, k, e] == s
            # aligned power-of-two chunks, then the tree over their results: the same bits
            for ch in (2, 8, 1024):
                assert F.tree_sum([F.tree_sum(el[c, k, i:i + ch]) for i in range(0, ne, ch)]) == got[c, k]
    assert (got[0] > 0).all()


@pytest.mark.parametrize("name,kw,nsteps", CASES)
def test_saved_and_restored_sums_continue_on_the_same_bits(case_factory, name, kw, nsteps):
    case, qs = oracle_states(case_factory, name, kw, nsteps)
    zref = CV.rest_elevations(case_factory(name, **kw))
    whole = mirror(case, qs, zref=zref)
    a = mirror(case, qs[:2], zref=zref)
    saved, n = a.sums()
    b = CV.HostEddyCov(case, zref=zref)
    b.set_sums(saved, n)
    for q in qs[2:]:
        b.add(q)
    assert b.nsamples == whole.nsamples == nsteps
    assert np.array_equal(b.sums()[0], whole.sums()[0])
    assert np.array_equal(b.fields(), whole.fields()) and np.array_equal(b.integrals(), whole.integrals())
    with pytest.raises(ValueError):
        b.set_sums(saved[:4], n)


def test_fields_need_a_sample_and_zref_its_shape(case_factory):
    case = case_factory("bump10", nop=2)
    with pytest.raises(ValueError):
        CV.HostEddyCov(case).fields()
    with pytest.raises(ValueError):
        CV.HostEddyCov(case, zref=np.zeros(case.scalars["npoin"]))


def test_host_sampler_cov_source_at_nodes(case_factory):
    case, qs = oracle_states(case_factory, *CASES[0])
    fl = mirror(case, qs).fields()
    ngl, ne, L = case.scalars["ngl"], case.scalars["nelem"], case.scalars["nlayers"]
    P = ngl * ngl
    xgl = S.case_xgl(case)
    ln = np.tile(np.arange(P), ne)
    hs = S.HostSampler(case, np.repeat(np.arange(ne), P) + 1, xgl[ln % ngl], xgl[ln // ngl], source="cov")
    got = hs.sample_cov(fl)
    assert got.shape == (16 * L, ne * P)
    for k in range(L):
        assert np.array_equal(got[16 * k:16 * k + 16], fl[:, :, k])


def test_time_loop_eddy_cov_hook(case_factory, tmp_path):
    """3 steps with the oracle stepper: one sample per step; eddy_cov=None writes and returns what the
    loop does without the argument."""
    import oracle as O
    case, qs = oracle_states(case_factory, *CASES[0])
    tf = 3 * case.scalars["dt"]
    runs = {}
    for tag, kw in (("plain", {}), ("none", {"eddy_cov": None}), ("cov", {"eddy_cov": CV.HostEddyCov(case)})):
        d = tmp_path / tag
        buf = io.StringIO()
        st = D.time_loop(case, O.Oracle(case), tf, out_dir=str(d), dump_data=True, out=buf, **kw)
        runs[tag] = (buf.getvalue(), {p.name: p.read_bytes() for p in sorted(d.iterdir())}, st, kw.get("eddy_cov"))
    for tag in ("none", "cov"):
        assert runs[tag][0] == runs["plain"][0]
        assert runs[tag][1] == runs["plain"][1]
        for a, b in zip(runs[tag][2], runs["plain"][2]):
            assert np.array_equal(a, b)
    got, want = runs["cov"][3], mirror(case, qs)
    assert got.nsamples == 3
    assert np.array_equal(got.sums()[0], want.sums()[0]) and np.array_equal(got.fields(), want.fields())
    every2 = CV.HostEddyCov(case)
    D.time_loop(case, O.Oracle(case), tf, out_dir=str(tmp_path / "e2"), out=io.StringIO(), eddy_cov=every2, cov_every=2)
    assert every2.nsamples == 1 and np.array_equal(every2.sums()[0], mirror(case, qs[1:2]).sums()[0])
    with pytest.raises(ValueError):
        D.time_loop(case, O.Oracle(case), tf, out_dir=str(tmp_path / "bad"), eddy_cov=want, cov_every=0)
