"""Online flow statistics (hnumo_stats_*, hnumo/flowstats.py), the parts that need no GPU: the
declarations on both sides of the boundary, the pairwise tree, the numpy mirror HostFlowStats on
the CPU oracle's states, and time_loop's flow_stats hook.  Every comparison is np.array_equal
unless it says otherwise."""
import io
import math
import os
import re

import numpy as np
import pytest

from hnumo import diagnostics as D
from hnumo import flowstats as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hnumo_stats_begin", "hnumo_stats_accumulate", "hnumo_stats_sums", "hnumo_stats_set_sums",
       "hnumo_stats_fields", "hnumo_stats_series", "hnumo_stats_end")
CASES = [("bump10", {"nop": 2}, 3), ("dg25L3", {"nelx": 5, "nely": 3}, 4)]
_states = {}


def test_header_fortran_module_and_python_declare_the_statistics():
    hdr = open(os.path.join(REPO, "include", "hnumo_engine.h")).read()
    f90 = open(os.path.join(REPO, "include", "hnumo_engine.f90")).read()
    py = open(os.path.join(REPO, "h-numo_amd", "hnumo", "engine.py")).read()
    public = re.search(r"public :: hnumo_engine_create.*?\n\s*\n", f90, re.S).group(0)
    for fn in NEW:
        assert re.search(r"\bint\s+%s\s*\(hnumo_engine \*eng" % fn, hdr), fn
        assert f"name='{fn}'" in f90, fn
        assert re.search(r"\b%s\b" % fn, public), fn
        assert f"L.{fn}.argtypes" in py, fn
        assert re.search(r"def %s\(self" % fn[len("hnumo_"):], py), fn
    assert re.search(r"#define HNUMO_ABI_VERSION 10\b", hdr)      # additive: the version stays
    assert re.search(r"HNUMO_ABI_EXPECTED = 10\b", f90)


def rule(x):
    """The tree of the definition, stated level by level on plain floats."""
    x = [float(v) for v in x]
    while len(x) > 1:
        x = [x[2 * i] + x[2 * i + 1] if 2 * i + 1 < len(x) else x[2 * i] for i in range((len(x) + 1) // 2)]
    return x[0]


@pytest.mark.parametrize("n", [1, 2, 3, 15, 64, 1369])
def test_tree_sum(n):
    rng = np.random.default_rng(n)
    x = rng.uniform(0.5, 2.0, n) * 10.0 ** rng.integers(-3, 4, n)
    got = F.tree_sum(x)
    assert got == rule(x)
    exact = math.fsum(x)
    assert abs(got - exact) <= n * 2.0 ** -53 * exact
    if n <= 2:
        seq = x[0]
        for v in x[1:]:
            seq = seq + v
        assert got == seq
    # aligned power-of-two chunks, then the tree over their results: the same bits
    for ch in (2, 8, 1024):
        assert F.tree_sum([F.tree_sum(x[i:i + ch]) for i in range(0, n, ch)]) == got


def oracle_states(case_factory, name, kw, nsteps):
    """The CPU oracle's states after steps 1..nsteps of the case (computed once)."""
    key = (name, tuple(sorted(kw.items())), nsteps)
    if key not in _states:
        import oracle as O
        case = case_factory(name, **kw)
        o = O.Oracle(case)
        q, qb, qp = o.state()
        out = []
        for _ in range(nsteps):
            o.ti_rk_bcl(q, qb, qp)
            out.append(q.copy(order="F"))
        _states[key] = (case, out)
    return _states[key]


@pytest.mark.parametrize("name,kw,nsteps", CASES)
def test_host_flow_stats_on_oracle_states(case_factory, name, kw, nsteps):
    case, states = oracle_states(case_factory, name, kw, nsteps)
    for q in states:
        assert np.isfinite(q).all()
    st = F.HostFlowStats(case)
    for q in states:
        st.add(q)
    assert st.nsamples == nsteps
    S, f = st.sums, st.fields()
    assert S.shape == (4, case.scalars["npoin"], case.scalars["nlayers"]) and f.shape == (5,) + S.shape[1:]
    um, vm, mke = S[1] / S[0], S[2] / S[0], S[3] / S[0]
    assert np.array_equal(f[0], S[0] / float(nsteps))
    assert np.array_equal(f[1], um) and np.array_equal(f[2], vm) and np.array_equal(f[3], mke)
    assert np.array_equal(f[4], mke - 0.5 * (um * um + vm * vm))
    assert np.isfinite(f).all() and (f[0] > 0).all()
    # the sums are the layer fields' sums, the series the integrals of the last sample
    qf = [D.layer_fields(case, q) for q in states]
    h = qf[0][0]
    for x in qf[1:]:
        h = h + x[0]
    assert np.array_equal(S[0], h)
    ser = st.series
    assert ser.shape == (2, case.scalars["nlayers"], nsteps) and (ser > 0).all()
    w = np.asarray(case.arrays["jac"]).reshape(-1, order="F")
    for k in range(case.scalars["nlayers"]):
        vol = math.fsum(w * qf[-1][0][:, k])
        assert abs(ser[1, k, -1] - vol) <= case.scalars["npoin"] * 2.0 ** -53 * vol
    assert np.array_equal(st.ke_normalised(), ser[0] / ser[1])
    # stopped and continued through sums / nsamples
    a = F.HostFlowStats(case)
    for q in states[:2]:
        a.add(q)
    b = F.HostFlowStats(case)
    b.sums, b.nsamples = a.sums.copy(order="F"), a.nsamples
    for q in states[2:]:
        b.add(q)
    assert b.nsamples == nsteps and np.array_equal(b.sums, S) and np.array_equal(b.fields(), f)
    assert np.array_equal(b.series, ser[:, :, 2:])


def test_fields_need_a_sample(case_factory):
    with pytest.raises(ValueError):
        F.HostFlowStats(case_factory("bump10", nop=2)).fields()


def test_time_loop_flow_stats_hook(case_factory, tmp_path):
    """4 steps of bump10 (nop=2) with the oracle stepper: stats_every=2 samples the states after
    steps 2 and 4; flow_stats=None writes and returns what the loop does without the arguments."""
    import oracle as O
    case, states = oracle_states(case_factory, "bump10", {"nop": 2}, 4)
    tf = 4 * case.scalars["dt"]
    runs = {}
    for tag, kw in (("plain", {}), ("none", {"flow_stats": None, "stats_every": 3}),
                    ("stats", {"flow_stats": F.HostFlowStats(case), "stats_every": 2})):
        d = tmp_path / tag
        buf = io.StringIO()
        st = D.time_loop(case, O.Oracle(case), tf, out_dir=str(d), dump_data=True, out=buf, **kw)
        runs[tag] = (buf.getvalue(), {p.name: p.read_bytes() for p in sorted(d.iterdir())}, st, kw.get("flow_stats"))
    for tag in ("none", "stats"):
        assert runs[tag][0] == runs["plain"][0]
        assert runs[tag][1] == runs["plain"][1]
        for a, b in zip(runs[tag][2], runs["plain"][2]):
            assert np.array_equal(a, b)
    got = runs["stats"][3]
    want = F.HostFlowStats(case)
    want.add(states[1])
    want.add(states[3])
    assert got.nsamples == 2
    assert np.array_equal(got.sums, want.sums) and np.array_equal(got.series, want.series)
    with pytest.raises(ValueError):
        D.time_loop(case, O.Oracle(case), tf, out_dir=str(tmp_path / "bad"), flow_stats=want, stats_every=0)
