"""Migrating float sets on the device (kernels_float.hip: float_advance_kernel<NGL, 1, true>,
float_arrive_kernel<NGL>, through hnumo_group_floats_* and the host-carried calls): every rank's floats and
series equal -- np.array_equal, no tolerance -- the Python mirror hnumo.floats.HostFloatGroup fed with the
ranks' synced states, and the merged series equals the series of a single-rank engine on the whole mesh.
Cases and seeds are tests/float_migrate_cases.py's."""
import numpy as np
import pytest

import float_cases as FC
import float_migrate_cases as MC
from hnumo import floats as FL

pytestmark = pytest.mark.gpu
NSTEP, NBIG = 2, 4
NREC = NSTEP + NBIG
KEYS = ("x", "y", "u", "v", "elem", "status")
_runs = {}


def same(got, want, what=""):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


def global_q(parts, qs, case):
    from hnumo.facepart import gather_faces_state
    return gather_faces_state(list(zip(parts, qs)), "q_df", case)


def device_group_run(parts, case, xy, layer, scale, stats_capacity=None, expect_full=False):
    """2 group steps with every = 1, then 4 group advances of big_dt of the last state: (get per rank, series
    per rank, the ranks' q after each step, big_dt, the final states)."""
    from hnumo.engine import Engine, EngineError, group_ti_rk_bcl, local_group
    engines = [Engine(p) for p in parts]
    local_group(engines)
    gf = FL.GroupFloats(engines, xy, layer, coord_scale=scale)
    gf.begin(every=1, record_every=1, capacity=NREC)
    if stats_capacity is not None:
        for g in engines:
            g.stats_begin(every=1, series=stats_capacity)
    sts = [g.state() for g in engines]
    qs = []
    for i in range(NSTEP):
        if expect_full and i == NSTEP - 1:
            with pytest.raises(EngineError) as ei:
                group_ti_rk_bcl(engines, sts)
            assert ei.value.code == 4 and "flow statistics after the step" in str(ei.value)
        else:
            group_ti_rk_bcl(engines, sts)
        qs.append([st[0].copy(order="F") for st in sts])
    big = FC.big_dt(case, global_q(parts, qs[-1], case))
    for _ in range(NBIG):
        gf.advance(dt=big)
    got, ser = gf.get(), gf.series()
    for g in engines:
        g.close()
    return got, ser, qs, big, sts


def mirror_group_run(parts, xy, layer, scale, qs, dt, big):
    grp = FL.HostFloatGroup(parts, xy, layer, coord_scale=scale)
    for q in qs:
        grp.advance(q, dt)
        grp.record()
    for _ in range(NBIG):
        grp.advance(qs[-1], big)
        grp.record()
    return grp


def single_rank_series(case, xy, layer, big):
    from hnumo.engine import Engine
    e = Engine(case)
    st = e.state()
    e.set_resident(True)
    one = FL.DeviceFloats(e, xy, layer)
    one.begin(every=1, record_every=1, capacity=NREC)
    for _ in range(NSTEP):
        e.ti_rk_bcl(*st)
    for _ in range(NBIG):
        one.advance(dt=big)
    ref, g = one.series(), one.get()
    e.sync(*st)
    e.close()
    return ref, g, st


def full_run(case_factory, row):
    if row not in _runs:
        case, parts = MC.partition(case_factory, row)
        xy, layer = MC.seeds(case, parts)
        scale = float(np.abs(np.asarray(case.arrays["coord"])[0:2]).max())
        got, ser, qs, big, sts = device_group_run(parts, case, xy, layer, scale)
        _runs[row] = dict(case=case, parts=parts, xy=xy, layer=layer, scale=scale, got=got, ser=ser, qs=qs, big=big, sts=sts)
    return _runs[row]


ALL_ROWS = MC.ROWS + [MC.NGL8]
ALL_IDS = MC.ROW_IDS + ["dg25N7L3_3x3_2morton"]


@pytest.mark.parametrize("row", ALL_ROWS, ids=ALL_IDS)
def test_every_ranks_get_and_series_equal_the_group_mirror(case_factory, row):
    R = full_run(case_factory, row)
    case, parts = R["case"], R["parts"]
    grp = mirror_group_run(parts, R["xy"], R["layer"], R["scale"], R["qs"], case.scalars["dt"], R["big"])
    want_ser = grp.series()
    for r in range(len(parts)):
        same(R["got"][r], grp.ranks[r].get(), r)
        assert R["ser"][r].shape == want_ser[r].shape == (5, grp.M, NREC)
        assert np.array_equal(R["ser"][r], want_ser[r]), (r, int((R["ser"][r] != want_ser[r]).sum()))
    assert grp.in_flight_after == 0 and not any((g["status"] == FL.LOST).any() for g in R["got"])
    assert sum(1 for p in grp.path if len(p) >= 2) >= 0.05 * grp.M and 1 <= grp.max_rounds <= FL.MAXROUNDS
    # per record at most one rank holds a float
    assert sum((s[4] > 0).astype(int) for s in R["ser"]).max() == 1


@pytest.mark.parametrize("row", ALL_ROWS, ids=ALL_IDS)
def test_merged_series_is_the_single_rank_series(case_factory, row):
    """The merged series of the group against a single-rank engine on the whole mesh, every float and record,
    np.array_equal: the test that fails without migration (the floats drain across the rank boundaries).

    The comparison needs the two runs to carry the same field.  On the 2-block-rank partition of bump10 they
    do (every node of q_df has the single-rank run's bits after both steps; asserted, so the case cannot lapse),
    and the device series of the single-rank engine is the reference.  On the two Morton partitions the STEP
    itself differs between the partitioned and the single-rank run, before any float moves: a processor face
    is evaluated with the reference's multi-rank arithmetic (hnumo/facepart.py), measured here as 3135 of 3375
    (dg25L3 5x3, 4 ranks) and 4896 of 5184 (dg25N7L3 3x3, 2 ranks) nodes of q_df with other bits after one
    step, max |diff| / max |q| = 1.8e-5.  No float can have the single-rank engine's bits on another field, so
    there the reference is the single-rank definition on the field the ranks carry: HostFloats on the whole
    mesh fed with the gathered states -- which is what the single-rank engine computes on its own field, bit
    for bit (tests/test_floats_gpu.py)."""
    R = full_run(case_factory, row)
    case, parts, xy, layer = R["case"], R["parts"], R["xy"], R["layer"]
    merged = FL.merge_series(R["ser"], parts)
    ref, _, st1 = single_rank_series(case, xy, layer, R["big"])
    same_field = np.array_equal(global_q(parts, R["qs"][-1], case), st1[0])
    print(ALL_IDS[ALL_ROWS.index(row)], "state bits equal the single-rank run's:", same_field,
          "; floats whose merged series differs from the single-rank engine's:", int((merged != ref).any(axis=(0, 2)).sum()), "of", xy.shape[1])
    assert same_field == (row == MC.ROWS[0])
    if same_field:
        assert np.array_equal(merged, ref), int((merged != ref).any(axis=(0, 2)).sum())
    one = FL.HostFloats(case, xy, layer)
    assert one.maxc == R["scale"]
    for q in [global_q(parts, q, case) for q in R["qs"]] + [global_q(parts, R["qs"][-1], case)] * NBIG:
        one.advance(q, case.scalars["dt"] if len(one._records) < NSTEP else R["big"])
        one.record()
    want = one.series()
    assert np.array_equal(merged, want), int((merged != want).any(axis=(0, 2)).sum())
    assert np.isfinite(want).all() and (want[4] > 0).sum() > 0.5 * want[4].size
    held = sum((s[4] > 0).astype(int) for s in R["ser"])
    assert np.array_equal(held > 0, want[4] > 0)                  # a float the single-rank run holds is held by one rank


def crossing_seeds(case_factory, M, rng):
    """M seeds of row 0, those that change rank in the mirror's run first, in a shuffled order."""
    run = MC.mirror_run(case_factory, MC.ROWS[0], scaled=True)
    cross = [m for m, p in enumerate(run["group"].path) if len(p) >= 2]
    cross.sort(key=lambda m: -len(run["group"].crossings[m]))
    rest = [m for m in range(run["one"].M) if len(run["group"].path[m]) == 1]
    pick = np.array((cross + rest)[:M])
    rng.shuffle(pick)
    return run["case"], run["parts"], np.asfortranarray(run["xy"][:, pick]), run["layer"][pick].copy(), run["scale"]


@pytest.mark.parametrize("M", [1, 257])
def test_one_float_and_a_tail_wave_in_shuffled_order(case_factory, M):
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    case, parts, xy, layer, scale = crossing_seeds(case_factory, M, np.random.default_rng(M))
    engines = [Engine(p) for p in parts]
    local_group(engines)
    gf = FL.GroupFloats(engines, xy, layer, coord_scale=scale)
    sts = [g.state() for g in engines]
    group_ti_rk_bcl(engines, sts)
    qs = [st[0].copy(order="F") for st in sts]
    big = FC.big_dt(case, global_q(parts, qs, case))
    grp = FL.HostFloatGroup(parts, xy, layer, coord_scale=scale)
    for _ in range(3):
        gf.advance(dt=big)
        grp.advance(qs, big)
    got = gf.get()
    for g in engines:
        g.close()
    for r in range(2):
        same(got[r], grp.ranks[r].get(), r)
    assert sum(len(c) for c in grp.crossings) >= 1
    assert sum((g["status"] == FL.ACTIVE).astype(int) for g in got).max() == 1       # one rank holds a float


def test_a_migrating_and_a_plain_set_side_by_side_and_the_state_bits(case_factory):
    """The plain set behaves as ever (tests/test_floats_gpu.py: check_ranks): its floats are the one-rank
    mirror's of each rank, LEFT at a processor face for good.  The migrating one is the group mirror's.  The
    states end on the bits of a group run with no set at all."""
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    case, parts = MC.partition(case_factory, MC.ROWS[0])
    xy, layer = MC.seeds(case, parts)
    scale = float(np.abs(np.asarray(case.arrays["coord"])[0:2]).max())
    engines = [Engine(p) for p in parts]
    local_group(engines)
    plain = [FL.DeviceFloats(g, xy, layer) for g in engines]
    gf = FL.GroupFloats(engines, xy, layer, coord_scale=scale)
    assert gf.id == 1 and all(s.id == 0 for s in plain)
    for s in plain:
        s.begin(every=1)
    gf.begin(every=1)
    sts = [g.state() for g in engines]
    qs = []
    for _ in range(NSTEP):
        group_ti_rk_bcl(engines, sts)
        qs.append([st[0].copy(order="F") for st in sts])
    big = FC.big_dt(case, global_q(parts, qs[-1], case))
    for _ in range(2):
        gf.advance(dt=big)
        for s in plain:
            s.advance(dt=big)
    got_m, got_p = gf.get(), [s.get() for s in plain]
    for g in engines:
        g.close()
    grp = FL.HostFloatGroup(parts, xy, layer, coord_scale=scale)
    mirrors = [FL.HostFloats(p, xy, layer) for p in parts]
    for q, dt in [(q, case.scalars["dt"]) for q in qs] + [(qs[-1], big)] * 2:
        grp.advance(q, dt)
        for r, hf in enumerate(mirrors):
            hf.advance(q[r], dt)
    for r in range(len(parts)):
        same(got_m[r], grp.ranks[r].get(), ("migrating", r))
        same(got_p[r], mirrors[r].get(), ("plain", r))
        assert ((got_p[r]["status"] == FL.LEFT) & (mirrors[r].elem == 0)).any()
    # the plain set has lost floats the migrating one still carries
    assert sum((g["status"] == FL.ACTIVE).sum() for g in got_p) - int(grp.shared.sum()) < sum((g["status"] == FL.ACTIVE).sum() for g in got_m)
    bare = [Engine(p) for p in parts]
    local_group(bare)
    sts0 = [g.state() for g in bare]
    for _ in range(NSTEP):
        group_ti_rk_bcl(bare, sts0)
    for g in bare:
        g.close()
    for a, b in zip(sts, sts0):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_group_step_with_a_full_statistics_series_still_migrates(case_factory):
    R = full_run(case_factory, MC.ROWS[0])
    got, ser, qs, big, _ = device_group_run(R["parts"], R["case"], R["xy"], R["layer"], R["scale"], stats_capacity=1, expect_full=True)
    assert big == R["big"]
    for r in range(2):
        same(got[r], R["got"][r], r)
        assert np.array_equal(ser[r], R["ser"][r])


def test_host_carried_records_give_the_group_advances_bits(case_factory):
    """outbox on each engine, route by (destination rank, pos) in Python, deliver, settle."""
    from hnumo.engine import Engine, group_ti_rk_bcl, local_group
    R = full_run(case_factory, MC.ROWS[1])
    case, parts, xy, layer = R["case"], R["parts"], R["xy"], R["layer"]
    engines = [Engine(p) for p in parts]
    local_group(engines)
    gf = FL.GroupFloats(engines, xy, layer, coord_scale=R["scale"])
    gf.begin(every=1, record_every=1, capacity=NREC)
    sts = [g.state() for g in engines]
    for _ in range(NSTEP):
        group_ti_rk_bcl(engines, sts)
    fid, nrounds, carried = gf.id, [], 0
    for _ in range(NBIG):
        for g in engines:
            g.floats_advance(fid, R["big"])
        for rnd in range(FL.MAXROUNDS + 1):
            boxes = [g.floats_outbox(fid) for g in engines]
            if not any(d.shape[1] for d, _ in boxes):
                break
            assert rnd < FL.MAXROUNDS
            for src, (d, i) in enumerate(boxes):
                assert (np.diff(i[0]) > 0).all()                   # sorted by gid
                for dst in np.unique(i[4]):
                    sel = i[4] == dst
                    engines[int(dst)].floats_deliver(fid, src, d[:, sel], i[:, sel])
                    carried += int(sel.sum())
        nrounds.append(rnd)
        for g in engines:
            g.floats_settle(fid)
    got, ser = gf.get(), gf.series()
    for g in engines:
        g.close()
    assert carried > 0 and max(nrounds) >= 2
    for r in range(len(parts)):
        same(got[r], R["got"][r], r)
        assert np.array_equal(ser[r], R["ser"][r]), r


def test_code_4_paths(case_factory):
    from hnumo.engine import Engine, EngineError, group_floats_advance, group_floats_migrate, local_group
    from hnumo.facepart import face_partition, self_neighbour
    from hnumo.partition import partition
    case, parts = MC.partition(case_factory, MC.ROWS[0])
    xy = FL.seed_grid(case, 5, 4)

    def refused(f, text):
        with pytest.raises(EngineError) as ei:
            f()
        assert ei.value.code == 4 and text in str(ei.value), str(ei.value)

    # engines without a processor-face halo between ranks: one rank, ghost layers, the self-neighbour emulation
    for c in (case, partition(case, 2, 0), self_neighbour(face_partition(case, 2, 1, "block"))):
        e = Engine(c)
        s = FL.DeviceFloats(e, xy, 1)
        refused(lambda: e.floats_migrate(s.id, True, 0.0), "needs a processor-face halo")
        refused(lambda: e.floats_outbox(s.id), "does not migrate")
        e.close()
    engines = [Engine(p) for p in parts]
    local_group(engines)
    sets = [FL.DeviceFloats(g, xy, 1) for g in engines]
    fid = sets[0].id
    e = engines[0]
    for bad in (-1.0, float("nan"), float("inf")):
        refused(lambda: e.floats_migrate(fid, True, bad), "coord_scale must be finite and >= 0")
        refused(lambda: group_floats_migrate(engines, fid, True, bad), "coord_scale must be finite and >= 0")
    for unknown in (-1, 3, 8):
        refused(lambda: e.floats_migrate(unknown, True, 0.0), "no float set with id")
        refused(lambda: group_floats_migrate(engines, unknown, True, 0.0), "no float set with id")
        refused(lambda: group_floats_advance(engines, unknown, 1.0), "no float set with id")
        refused(lambda: e.floats_settle(unknown), "no float set with id")
    refused(lambda: group_floats_advance(engines, fid, 1.0), "does not migrate")
    refused(lambda: e.floats_release(fid, [0]), "does not migrate")
    refused(lambda: e.floats_deliver(fid, 1, np.zeros((7, 1)), np.zeros((6, 1), np.int32)), "does not migrate")
    group_floats_migrate(engines, fid, True, 0.0)
    refused(lambda: group_floats_advance(engines, fid, 1.0), "no state on the device yet")
    refused(lambda: e.floats_release(fid, [xy.shape[1]]), "is outside 0..M-1")
    refused(lambda: e.floats_deliver(fid, 0, np.zeros((7, 1)), np.zeros((6, 1), np.int32)), "shares no processor face")
    rec = np.zeros((6, 1), np.int32)
    rec[:, 0] = [0, 1, 0, 1, 0, 0]                                  # gid, layer, stage, hops, dest = rank 0, pos
    for row, v in ((0, xy.shape[1]), (1, 0), (2, 2), (3, 0), (3, 5), (5, 10 ** 6)):
        bad = rec.copy()
        bad[row, 0] = v
        refused(lambda: e.floats_deliver(fid, 1, np.zeros((7, 1)), bad), "is no flight record")
    sets[1].destroy()
    refused(lambda: group_floats_migrate(engines, fid, True, 0.0), "no float set with id")
    for g in engines:
        g.close()
