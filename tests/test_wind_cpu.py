"""The host side of the time-dependent wind (hnumo/wind.py): the blend's summation order, tau_wind_ave against
the CPU oracle, the schedule's rows, the coefficient tables, and time_loop(wind=HostWind) around an oracle-backed
stepper.  Every comparison is bitwise."""
import io
import os

import numpy as np
import pytest

import wind_cases as W
from hnumo import wind


def test_blend_adds_left_to_right_from_the_first_product():
    """1.0 + 2^-53 + 2^-53: left to right both small terms are lost to ties-to-even and the sum is 1.0; the
    other association adds 2^-52 first and gives 1 + 2^-52."""
    p = np.zeros((2, 3, 3), order="F")
    p[:, :, 0], p[:, :, 1], p[:, :, 2] = 1.0, 2.0 ** -53, 2.0 ** -53
    tau = wind.blend(p, (1.0, 1.0, 1.0))
    assert tau.shape == (2, 3) and np.array_equal(tau, np.ones((2, 3)))
    assert 1.0 + (2.0 ** -53 + 2.0 ** -53) == 1.0 + 2.0 ** -52 != 1.0
    # the product comes first: c_m*T_m is rounded before it is added
    p[:, :, 1], p[:, :, 2] = 2.0 ** -52, 2.0 ** -52
    assert np.array_equal(wind.blend(p, (1.0, 0.5, 0.5)), np.ones((2, 3)))


def test_blend_shapes():
    p = np.arange(12.0).reshape(2, 3, 2, order="F")
    assert np.array_equal(wind.blend(p, (2.0, 0.0)), 2.0 * p[:, :, 0])
    assert np.array_equal(wind.blend(p[:, :, 0], (3.0,)), 3.0 * p[:, :, 0])
    assert wind.blend(p, (1.0, 1.0)).flags["F_CONTIGUOUS"]
    with pytest.raises(ValueError):
        wind.blend(p, (1.0,))
    with pytest.raises(ValueError):
        wind.blend(np.zeros((2, 3, 5)), np.ones(5))


@pytest.fixture(scope="module")
def n2(case_factory):
    case = W.case_of("N2", case_factory)
    assert case.scalars["npoin_q"] == W.NPQ["N2"]
    return case


def test_ave_is_the_oracles_tau_wind_ave(n2):
    """wind.ave of a blended wind equals the tau_wind_ave field of an oracle created with that wind, after a
    step; and it is not tau itself: at least one value differs in bits."""
    tau = wind.blend(W.patterns(n2, 3), (0.5, 0.25, -1.0))
    (st,), o = W.Oracles(n2).run([tau])
    assert all(np.isfinite(a).all() for a in st)
    N = n2.scalars["N_btp"]
    assert N > 2
    a = wind.ave(tau, N)
    assert np.array_equal(a, o.field("tau_wind_ave"))
    assert (a != tau).any()
    # the case's own smooth wind too
    t0 = np.asarray(n2.arrays["tau_wind"])
    assert np.abs(t0).max() > 0.0
    assert np.array_equal(wind.ave(t0, N), W.Oracles(n2).run([t0])[1].field("tau_wind_ave"))


def test_row_for():
    H, R = wind.HOLD, wind.REPEAT
    assert [wind.row_for(k, 3, 0, H) for k in range(6)] == [0, 1, 2, 2, 2, 2]
    assert [wind.row_for(k, 3, 0, R) for k in range(7)] == [0, 1, 2, 0, 1, 2, 0]
    assert [wind.row_for(k, 3, 2, H) for k in range(3)] == [2, 2, 2]
    assert [wind.row_for(k, 3, 2, R) for k in range(4)] == [2, 0, 1, 2]
    assert [wind.row_for(k, 3, 7, R) for k in range(3)] == [1, 2, 0]
    assert wind.row_for(5, 1, 0, "hold") == 0 and wind.row_for(5, 1, 3, "repeat") == 0
    assert wind.row_for(0, 0) == -1
    for bad in (dict(k=-1, nrows=3), dict(k=0, nrows=3, first=-1), dict(k=0, nrows=-1), dict(k=0, nrows=3, mode=2),
                dict(k=0, nrows=3, mode="loop")):
        with pytest.raises(ValueError):
            wind.row_for(**bad)


def test_tables():
    r = wind.ramp(4)
    assert r.shape == (1, 4) and np.array_equal(r[0], [0.25, 0.5, 0.75, 1.0])
    assert np.array_equal(wind.ramp(1), [[1.0]])
    s = wind.seasonal(4)
    assert s.shape == (2, 4) and np.array_equal(s[0], np.ones(4))
    assert s[1, 0] == 0.0 and s[1, 1] == 1.0 and abs(s[1, 2]) < 1e-15 and s[1, 3] == -1.0
    for f in (wind.ramp, wind.seasonal):
        with pytest.raises(ValueError):
            f(0)


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_time_loop_with_an_identity_table_writes_the_same_files(n2, tmp_path):
    """A table of (1.0,) rows on the case's own pattern: 1.0*T is T in every bit, so the loop's files and state
    are those of a loop without a wind."""
    import oracle as O
    from hnumo import diagnostics as D
    dt = n2.scalars["dt"]
    a, b = tmp_path / "plain", tmp_path / "wind"
    plain = D.time_loop(n2, O.Oracle(n2), 2.5 * dt, out_dir=str(a), dump_data=True, out=io.StringIO())
    stp = W.OracleStepper(n2)
    hw = wind.HostWind(W.patterns(n2, 1), np.ones((1, 2)), "repeat")
    got = D.time_loop(n2, stp, 2.5 * dt, out_dir=str(b), dump_data=True, out=io.StringIO(), wind=hw)
    assert len(stp.winds) == 3 and all(np.array_equal(t, n2.arrays["tau_wind"]) for t in stp.winds)
    assert W.same_state(got, plain)
    fa, fb = _files(str(a)), _files(str(b))
    assert list(fa) == list(fb) and len(fa) >= 5
    assert fa == fb


def test_time_loop_with_a_ramp_equals_a_hand_written_loop(n2, tmp_path):
    """Three rows of a ramp, held: five steps of time_loop(wind=HostWind) against a loop that blends and steps by
    hand; the stepper is handed a wind only when the row changes."""
    from hnumo import diagnostics as D
    pat, tab = W.patterns(n2, 2), np.asfortranarray(np.vstack([wind.ramp(3)[0], [0.3, -0.2, 0.1]]))
    dt = n2.scalars["dt"]
    stp = W.OracleStepper(n2)
    got = D.time_loop(n2, stp, 4.5 * dt, out_dir=str(tmp_path), out=io.StringIO(), wind=wind.HostWind(pat, tab, "hold"))
    assert len(stp.winds) == 3
    taus = [wind.blend(pat, tab[:, wind.row_for(k, 3, 0, wind.HOLD)]) for k in range(5)]
    assert not np.array_equal(taus[0], taus[1]) and np.array_equal(taus[3], taus[2])
    want, _ = W.Oracles(n2).run(taus)
    assert all(np.isfinite(x).all() for x in want[-1])
    assert W.same_state(got, want[-1])
    # and the wind matters: the plain loop ends elsewhere
    import oracle as O
    plain = D.time_loop(n2, O.Oracle(n2), 4.5 * dt, out_dir=str(tmp_path), out=io.StringIO())
    assert not np.array_equal(plain[0], got[0])


def test_time_loop_restart_resumes_the_table(n2, tmp_path):
    """A loop restarted from snapshot 2 calls before_step with the run's step numbers 2, 3, ..."""
    from hnumo import diagnostics as D
    import oracle as O
    dt = n2.scalars["dt"]
    D.time_loop(n2, O.Oracle(n2), 2.5 * dt, out_dir=str(tmp_path), dump_data=True, out=io.StringIO())
    seen = []

    class Spy:
        def before_step(self, stepper, nstep):
            seen.append(nstep)

    D.time_loop(n2, O.Oracle(n2), 4.5 * dt, out_dir=str(tmp_path), time_initial=2 * dt, restart_file_number=2,
                out=io.StringIO(), wind=Spy())
    assert seen == [2, 3, 4]
