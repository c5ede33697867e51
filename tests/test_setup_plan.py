"""The host-only setup plan of engine creation (h-numo_amd/csrc/setup_plan.h): descriptor validation
and every table the engine uploads, run on the CPU.

tests/setup_plan_main.cpp includes the header; this module compiles it once per session with
AddressSanitizer and UBSan into a temporary directory and runs it as a child process on descriptor
dumps written from hnumo.abi.Descriptors(case).keep (the record format is private to the two
files).  Nothing is loaded into Python.  The invariants below are derived from the input arrays
(face, imapl/imapr, the named statics) or from the property itself, not from the C++ loops.

Validation: every failure exit of build_setup_plan is reached by one mutated field of a valid dump
(test_rejected), but one: "face node orderings of neighbouring elements disagree".  No input reaches
it: the check compares an element side's enbr_node, built from the neighbour side's imap row, with
the neighbour's efmap, built from that same row (so an imapr row reversed on one interior face is
accepted)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="no g++ to compile tests/setup_plan_main.cpp with")

INVALID = 3  # exit status of setup_plan_main for HNUMO_ERR_INVALID


@pytest.fixture(scope="session")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("setup_plan") / "setup_plan_main")
    hip = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I" + hip, os.path.join(HERE, "setup_plan_main.cpp"), "-o", exe],
                   check=True)
    return exe


# ---------------------------------------------------------------- dumps
def fields_of(case, ncu=()):
    """name -> array of one descriptor dump, in a fixed order: mesh scalars, mesh arrays, statics,
    params, halo (multi-rank cases), ncu."""
    from hnumo import abi
    D = abi.Descriptors(case)
    d = {}
    for k in ("nelem", "npoin", "npoin_q", "nface", "ngl", "nq", "nlayers"):
        d[k] = np.array([getattr(D.mesh, k)], np.int32)
    for k, v in D.keep.items():
        d[k] = v
    for k, t in abi.Params._fields_:
        if k != "reserved":
            d[k] = np.array([getattr(D.params, k)], np.int32 if t is abi.C.c_int32 else np.float64)
    if getattr(case, "nranks", 1) > 1 or getattr(case, "fneighbours", None):
        H = abi.Halo(case)
        d["halo"] = np.array([1], np.int32)
        for k in ("rank", "nranks", "num_nbh", "nelem_owned"):
            d[k] = np.array([getattr(H.desc, k)], np.int32)
        for k, v in H.keep.items():
            if v.size:  # (an empty list is a NULL pointer, as in abi.Halo)
                d[k] = v
    d["ncu"] = np.array(list(ncu), np.int32)
    return d


def write_dump(path, d):
    with open(path, "wb") as f:
        for k, v in d.items():
            v = np.ascontiguousarray(v)
            assert v.dtype in (np.int32, np.float64), (k, v.dtype)
            f.write(struct.pack("<i", len(k)) + k.encode() + (b"i" if v.dtype == np.int32 else b"d"))
            f.write(struct.pack("<q", v.size) + v.tobytes())


def read_dump(path):
    out = {}
    with open(path, "rb") as f:
        b = f.read()
    o = 0
    while o < len(b):
        (nl,) = struct.unpack_from("<i", b, o)
        k = b[o + 4:o + 4 + nl].decode()
        t = b[o + 4 + nl:o + 5 + nl]
        (n,) = struct.unpack_from("<q", b, o + 5 + nl)
        o += 13 + nl
        dt, sz = (np.int32, 4) if t == b"i" else (np.float64, 8)
        out[k] = np.frombuffer(b, dt, n, o).copy()
        o += n * sz
    return out


def run_plan(exe, d, tmp):
    """(exit status, records) of one run; a sanitizer report fails the test."""
    write_dump(os.path.join(tmp, "in.bin"), d)
    r = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], capture_output=True, text=True)
    assert r.returncode in (0, INVALID) and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.returncode, read_dump(os.path.join(tmp, "out.bin"))


CONN = ["efaces", "eside", "ebc", "efmap", "enbr_node", "enbr_e", "enbr_lf", "fnodeL", "fnodeR", "fel", "fer", "fslotL",
        "fslotR", "fslotA", "erec"]


class Plan:
    """A case's inputs (Fortran-shaped views of the dump) and its plan tables."""

    def __init__(self, d, t):
        self.d, self.t = d, t
        self.E, self.F, self.ngl, self.nq = (int(d[k][0]) for k in ("nelem", "nface", "ngl", "nq"))
        self.P, self.Q = self.ngl ** 2, self.nq ** 2
        self.face = d["face"].reshape(8, self.F, order="F")
        self.face_halo, self.NS, self.EO, self.nb0, self.ERS, self.qstride = (int(x) for x in t["scalars"])
        off = [int(x) for x in t["conn_off"]] + [t["conn"].size]
        assert off == sorted(off) and off[0] == 0
        for i, k in enumerate(CONN):
            setattr(self, k if k != "fslotA" else "fslotA_conn", t["conn"][off[i]:off[i + 1]])
        self.fslotA = t["fslotA"]

    def imap(self, side):
        """[slotwise] element-local node j*ngl+i of face node n of every face, left (0) / right (1)"""
        m = self.d["imapl" if side == 0 else "imapr"].reshape(3, self.ngl, self.F, order="F")
        return ((m[1] - 1) * self.ngl + (m[0] - 1)).T  # [F][ngl]


def _cases():
    from hnumo.facepart import face_partition, self_neighbour
    from hnumo.partition import partition
    single = {
        "dg3x3": ("dg25L3", dict(nelx=3, nely=3), (4, 8)),
        "dg6x6": ("dg25L3", dict(nelx=6, nely=6), (4, 8)),
        "dg6x6xb": ("dg25L3", dict(nelx=6, nely=6, x_boundary=(2, 4)), (4, 8)),
        "dg25L3": ("dg25L3", {}, (256, 25)),
        "bump10": ("bump10", {}, (4,)),
        "dg8N7": ("dg25", dict(nelx=8, nely=8, nop=7, dt=180.0, dt_btp=9.0), (4,)),
        "qmbump8": ("qmbump8", {}, (4,)),
        "bump10q": ("bump10q", {}, (4,)),
    }
    multi = {
        "face_r0": lambda c: face_partition(c, 2, 0, "block"),
        "face_r1": lambda c: face_partition(c, 2, 1, "block"),
        "self_r1": lambda c: self_neighbour(face_partition(c, 2, 1, "block")),
        "ghost_r0": lambda c: partition(c, 2, 0),
        "ghost_r1": lambda c: partition(c, 2, 1),
    }
    return single, multi


SINGLE = ["dg3x3", "dg6x6", "dg6x6xb", "dg25L3", "bump10", "dg8N7", "qmbump8", "bump10q"]
MULTI = ["face_r0", "face_r1", "self_r1", "ghost_r0", "ghost_r1"]
_plans = {}


@pytest.fixture(scope="session")
def plan_of(plan_exe, case_factory, tmp_path_factory):
    """name -> Plan; every case's child process runs once per session."""
    def get(name):
        if name not in _plans:
            single, multi = _cases()
            if name in single:
                cfg, kw, ncu = single[name]
                d = fields_of(case_factory(cfg, **kw), ncu)
            else:
                d = fields_of(multi[name](case_factory("bump10")))
            rc, t = run_plan(plan_exe, d, str(tmp_path_factory.mktemp("plan_" + name)))
            assert rc == 0, t
            _plans[name] = Plan(d, t)
        return _plans[name]
    return get


ALL = SINGLE + MULTI


# ---------------------------------------------------------------- connectivity
@pytest.mark.parametrize("name", ALL)
def test_element_face_connectivity(name, plan_of):
    p = plan_of(name)
    E, F = p.E, p.F
    el, er = p.face[6] - 1, p.face[7]
    assert np.array_equal(p.fel, el) and np.array_equal(p.fer, er)
    assert p.efaces.size == 4 * E == F + np.count_nonzero(er > 0)
    assert np.all(np.diff(p.efaces.reshape(E, 4), axis=1) > 0)
    slots = np.arange(4 * E)
    f, s = p.efaces, p.eside
    # (efaces, eside) -> slot is fslotL/fslotR, and back
    assert np.array_equal(np.where(s == 0, p.fslotL[f], p.fslotR[f]), slots)
    assert np.all(p.fslotL >= 0) and np.array_equal(p.fslotR >= 0, er > 0)
    assert np.array_equal(p.efaces[p.fslotL], np.arange(F)) and np.all(p.eside[p.fslotL] == 0)
    R = np.flatnonzero(er > 0)
    assert np.array_equal(p.efaces[p.fslotR[R]], R) and np.all(p.eside[p.fslotR[R]] == 1)
    # the slot's element is the face's face(7) / face(8) element
    assert np.array_equal(slots // 4, np.where(s == 0, el[f], er[f] - 1))
    assert np.array_equal(p.ebc, er[f])
    # efmap: the imapl / imapr node of the slot's side
    mine = np.where((s == 0)[:, None], p.imap(0)[f], p.imap(1)[f])
    assert np.array_equal(p.efmap.reshape(4 * E, p.ngl), mine)


@pytest.mark.parametrize("name", ALL)
def test_neighbour_slots(name, plan_of):
    p = plan_of(name)
    E, ngl = p.E, p.ngl
    efmap, nbn = p.efmap.reshape(4 * E, ngl), p.enbr_node.reshape(4 * E, ngl)
    I = np.flatnonzero(p.ebc > 0)
    partner = 4 * p.enbr_e[I] + p.enbr_lf[I]
    assert np.all((p.enbr_lf[I] >= 0) & (p.enbr_lf[I] < 4) & (p.enbr_e[I] >= 0) & (p.enbr_e[I] < E))
    assert np.array_equal(p.efaces[partner], p.efaces[I]) and np.all(partner != I)
    assert np.all(p.ebc[partner] > 0) and np.array_equal(4 * p.enbr_e[partner] + p.enbr_lf[partner], I)
    assert np.array_equal(nbn[I], p.enbr_e[I][:, None] * p.P + efmap[partner])
    # physical boundaries have no neighbour; processor faces point to their send slot
    B = np.flatnonzero(p.ebc < 0)
    assert np.all(p.enbr_e[B] == -1) and np.all(p.enbr_lf[B] == -1)
    assert np.all(nbn[p.ebc <= 0] == -1)
    X = np.flatnonzero(p.ebc == 0)
    assert (X.size > 0) == bool(p.face_halo)
    assert np.array_equal(4 * p.enbr_e[X] + p.enbr_lf[X], 4 * E + p.t["face_slot"][p.efaces[X]])
    assert np.all((p.enbr_lf[X] >= 0) & (p.enbr_lf[X] < 4))


@pytest.mark.parametrize("name", ALL)
def test_face_nodes(name, plan_of):
    p = plan_of(name)
    efmap = p.efmap.reshape(4 * p.E, p.ngl)
    assert np.array_equal(p.fnodeL.reshape(p.F, p.ngl), p.fel[:, None] * p.P + efmap[p.fslotL])
    R = p.fer > 0
    fr = p.fnodeR.reshape(p.F, p.ngl)
    assert np.array_equal(fr[R], (p.fer[R] - 1)[:, None] * p.P + efmap[p.fslotR[R]]) and np.all(fr[~R] == -1)


@pytest.mark.parametrize("name", ALL)
def test_fslotA(name, plan_of):
    p = plan_of(name)
    assert np.array_equal(p.fslotA, p.fslotA_conn)
    el, er, EO = p.fel, p.fer, p.EO
    if name.startswith("ghost"):
        assert 0 < EO < p.E
        right = (el >= EO) & (er > 0) & (er - 1 < EO)
        assert right.any() == (name == "ghost_r1")  # (rank 0's ghosts lie to its right: they are face(8))
        assert np.array_equal(p.fslotA, np.where(right, p.fslotR, p.fslotL))
    else:
        assert EO == p.E and np.array_equal(p.fslotA, p.fslotL)
    acc = p.erec.reshape(p.E, p.ERS)[:, 20:24].reshape(-1)
    assert set(np.unique(acc)) <= {0, 1}
    per_face = np.bincount(p.efaces, weights=acc, minlength=p.F)
    owned = (el < EO) | ((er > 0) & (er - 1 < EO))
    assert np.all(per_face[owned] == 1)


@pytest.mark.parametrize("name", ALL)
def test_erec(name, plan_of):
    p = plan_of(name)
    E, ngl, P = p.E, p.ngl, p.P
    assert p.ERS == (24 + 4 * ngl + 2 * P + 3) // 4 * 4 and p.erec.size == E * p.ERS
    r = p.erec.reshape(E, p.ERS)
    for i, tab in enumerate([p.efaces, p.eside, p.ebc, p.enbr_e, p.enbr_lf]):
        assert np.array_equal(r[:, 4 * i:4 * i + 4], tab.reshape(E, 4)), i
    assert np.array_equal(r[:, 20:24], (p.fslotA[p.efaces] == np.arange(4 * E)).reshape(E, 4))
    efmap = p.efmap.reshape(E, 4 * ngl)
    assert np.array_equal(r[:, 24:24 + 4 * ngl], efmap)
    pf = r[:, 24 + 4 * ngl:24 + 4 * ngl + 2 * P].reshape(E, P, 2)
    want = np.full((E, P, 2), -1)
    for e in range(E):
        for node in range(P):
            at = np.flatnonzero(efmap[e] == node)  # ascending lf*ngl+n
            assert at.size <= 2
            want[e, node, :at.size] = at
    assert np.array_equal(pf, want)
    assert np.all(r[:, 24 + 4 * ngl + 2 * P:] == -1)


# ---------------------------------------------------------------- statics
def _rows(p):
    """the named input rows of the SoA blocks, in the order of engine_internal.h's enums"""
    d = p.d
    two = lambda k, c, n=2: d[k].reshape(n, -1, order="F")[c]  # noqa: E731
    qs = [d["jacq"], d["s_coriolis_quad"], two("s_tau_wind", 0), two("s_tau_wind", 1), two("s_grad_zbot_quad", 0),
          two("s_grad_zbot_quad", 1), d["s_one_over_pbprime"], d["ksiq_x"], d["ksiq_y"], d["etaq_x"], d["etaq_y"],
          d["s_pbprime"]]
    ns = [d["s_pbprime_df"], d["s_one_over_pbprime_df"], d["massinv"], d["jac"], d["ksi_x"], d["ksi_y"], d["eta_x"],
          d["eta_y"], d["s_zbot_df"], d["s_fdt2_bcl"], d["s_a_bcl"], d["s_b_bcl"]]
    fs = [two("normal_vector_q", 0, 3), two("normal_vector_q", 1, 3), d["jac_faceq"], d["s_coeff_pbpert_L"],
          d["s_coeff_pbpert_R"], d["s_coeff_pbub_LR"], d["s_coeff_mass_pbub_L"], d["s_coeff_mass_pbub_R"],
          d["s_coeff_mass_pbpert_LR"], d["s_one_over_pbprime_edge"], two("s_pbprime_face", 0), two("s_pbprime_face", 1),
          two("s_zbot_face", 0), two("s_zbot_face", 1)]
    fns = [two("normal_vector", 0, 3), two("normal_vector", 1, 3), d["jac_face"], two("s_pbprime_df_face", 0),
           two("s_pbprime_df_face", 1)]
    return qs, ns, fs, fns


@pytest.mark.parametrize("name", ALL)
def test_soa_statics(name, plan_of):
    p = plan_of(name)
    for key, rows in zip(("qs", "ns", "fs", "fns"), _rows(p)):
        blk = p.t[key].reshape(len(rows), -1)
        for i, row in enumerate(rows):
            assert np.array_equal(blk[i], row), (key, i)


def _qe_pos(c, q, Q):
    """engine_internal.h: W first, then (e_x, n_x) and (e_y, n_y) interleaved per quad point, then rows"""
    return {0: q, 1: Q + 2 * q, 3: Q + 2 * q + 1, 2: 3 * Q + 2 * q, 4: 3 * Q + 2 * q + 1}.get(c, c * Q + q)


@pytest.mark.parametrize("name", ALL)
def test_element_major_statics(name, plan_of):
    p = plan_of(name)
    E, F, ngl, nq, P, Q = p.E, p.F, p.ngl, p.nq, p.P, p.Q
    qs, ns, fs, fns = _rows(p)
    qe = [qs[i] for i in (0, 7, 8, 9, 10, 1, 2, 3, 4, 5, 6)]  # W e_x e_y n_x n_y cor tw1 tw2 gz1 gz2 1/pb
    ne = [ns[i] for i in (4, 5, 6, 7, 3, 1, 2, 0)]            # e_x e_y n_x n_y w 1/pb massinv pb
    assert p.qstride == (11 * Q + 1) // 2 * 2
    pos = np.array([[_qe_pos(c, q, Q) for q in range(Q)] for c in range(11)])
    assert np.array_equal(p.t["qe_pos"].reshape(11, Q), pos) and np.unique(pos).size == 11 * Q
    qsE = p.t["qsE"].reshape(E, p.qstride)
    for c in range(11):
        assert np.array_equal(qsE[:, pos[c]], qe[c].reshape(E, Q)), c
    nsE = p.t["nsE"].reshape(E, 8, P)
    for c in range(8):
        assert np.array_equal(nsE[:, c], ne[c].reshape(E, P)), c
    FBLK = 12 * nq + 5 * ngl
    efs = p.t["efs"].reshape(4 * E, FBLK)
    f = p.efaces
    for c in range(10):
        assert np.array_equal(efs[:, c * nq:(c + 1) * nq], fs[c].reshape(F, nq)[f]), c
    for c in range(5):
        assert np.array_equal(efs[:, 12 * nq + c * ngl:12 * nq + (c + 1) * ngl], fns[c].reshape(F, ngl)[f]), c
    # EF_PBLQ / EF_PBRQ: sum_n psiq(n,iq) * pbprime_df_face(s,n,f), n = 0..ngl-1 in that order (the
    # order is the contract: one add per n, no numpy reduction)
    psiq = p.d["psiq"].reshape(ngl, nq, order="F")
    pbf = p.d["s_pbprime_df_face"].reshape(2, ngl, F, order="F")
    for s in range(2):
        acc = np.zeros((4 * E, nq))
        for n in range(ngl):
            acc = acc + psiq[n][None, :] * pbf[s, n, f][:, None]
        assert np.array_equal(efs[:, (10 + s) * nq:(11 + s) * nq], acc), s


@pytest.mark.parametrize("name", ["dg3x3", "bump10", "dg8N7", "qmbump8"])
def test_basis(name, plan_of):
    p = plan_of(name)
    ngl, nq = p.ngl, p.nq
    hb, a, b = p.t["hb"], ngl * nq, ngl * ngl
    F = lambda k, n: p.d[k].reshape(ngl, n, order="F")  # noqa: E731
    assert p.nb0 == 2 * a + 2 * b and hb.size == p.nb0 + 2 * a + b
    assert np.array_equal(hb[:a].reshape(ngl, nq), F("psiq", nq))
    assert np.array_equal(hb[a:2 * a].reshape(ngl, nq), F("dpsiq", nq))
    assert np.array_equal(hb[2 * a:2 * a + b].reshape(ngl, ngl), F("dpsi", ngl))
    assert np.array_equal(hb[2 * a + b:p.nb0].reshape(ngl, ngl), F("psi", ngl))
    pd = hb[p.nb0:]
    assert np.array_equal(pd[:2 * a:2], hb[:a]) and np.array_equal(pd[1:2 * a:2], hb[a:2 * a])
    assert np.array_equal(pd[2 * a:], hb[2 * a:2 * a + b])


def test_fq(plan_of):
    p = plan_of("bump10q")
    F, nq, Q = p.F, p.nq, p.Q
    fq = p.t["fq"].reshape(2, F, nq)
    R = p.face[7] > 0
    assert np.all((fq[0] >= 0) & (fq[0] < Q)) and np.all((fq[1][R] >= 0) & (fq[1][R] < Q)) and np.all(fq[1][~R] == -1)
    for s, k in enumerate(("imapl_q", "imapr_q")):
        m = p.d[k].reshape(3, nq, F, order="F")
        want = ((m[1] - 1) * nq + (m[0] - 1)).T
        sel = slice(None) if s == 0 else R
        assert np.array_equal(fq[s][sel], want[sel])
    assert plan_of("bump10").t["fq"].size == 0


# ---------------------------------------------------------------- halo
@pytest.mark.parametrize("name", ["face_r0", "face_r1", "self_r1"])
def test_face_halo_lists(name, plan_of):
    p = plan_of(name)
    E, NS = p.E, p.NS
    num, lst = p.d["num_send_recv"], p.d["nbh_send_recv"] - 1
    assert p.face_halo == 1 and NS == lst.size and np.array_equal(p.t["sface"], lst)
    off = np.concatenate([[0], np.cumsum(num)[:-1]])
    assert np.array_equal(p.t["fnb"].reshape(-1, 3), np.stack([p.d["nbh_proc"] - 1, off, num], axis=1))
    slot = np.full(p.F, -1)
    slot[lst] = np.arange(NS)
    assert np.array_equal(p.t["face_slot"], slot)
    assert np.array_equal(np.flatnonzero(p.face[7] == 0), np.sort(lst))
    proc = p.ebc == 0
    assert np.array_equal(p.t["tsrc"], np.where(proc, 4 * E + NS + slot[p.efaces], np.arange(4 * E)))
    elB, elI = p.t["elB"], p.t["elI"]
    assert np.array_equal(elB, np.flatnonzero(proc.reshape(E, 4).any(axis=1)))
    assert np.array_equal(np.sort(np.concatenate([elB, elI])), np.arange(E)) and np.all(np.diff(elI) > 0)


@pytest.mark.parametrize("name", SINGLE[:3] + ["ghost_r0"])
def test_no_face_halo_tables_elsewhere(name, plan_of):
    p = plan_of(name)
    assert p.face_halo == 0 and p.NS == 0
    assert all(p.t[k].size == 0 for k in ("tsrc", "elB", "elI", "sface", "fnb")) and np.all(p.t["face_slot"] == -1)


@pytest.mark.parametrize("name", ["ghost_r0", "ghost_r1"])
def test_ghost_lists(name, plan_of):
    p = plan_of(name)
    E, EO = p.E, p.EO
    assert EO == int(p.d["nelem_owned"][0]) and np.array_equal(p.t["gnb_rank"], p.d["nbh_proc"])
    assert np.array_equal(p.t["gnb_nsend"], p.d["num_ghost_send"]) and np.array_equal(p.t["gnb_nrecv"], p.d["num_ghost_recv"])
    snd, rcv = p.t["gnb_send"], p.t["gnb_recv"]
    assert np.array_equal(snd, p.d["ghost_send"] - 1) and np.array_equal(rcv, p.d["ghost_recv"] - 1)
    assert snd.size and rcv.size and np.all((snd >= 0) & (snd < EO)) and np.all((rcv >= EO) & (rcv < E))


# ---------------------------------------------------------------- placement
@pytest.mark.parametrize("name,ncu", [("dg3x3", 4), ("dg3x3", 8), ("dg6x6", 4), ("dg6x6", 8), ("dg6x6xb", 8),
                                      ("dg25L3", 256), ("dg25L3", 25)])
def test_placement_perm(name, ncu, plan_of):
    p = plan_of(name)
    E = p.E
    perm = p.t[f"perm_{ncu}"]
    if E % ncu == 0:
        assert perm.size == 0
        return
    assert np.array_equal(np.sort(perm), np.arange(E))
    bnd = (p.face[7][p.efaces] < 0).reshape(E, 4).any(axis=1)
    light = np.arange(E) % ncu >= E % ncu  # blocks on the CUs that hold one block fewer
    # the light blocks take the boundary elements, ascending, until those run out; every other block
    # takes the interior elements, ascending (and boundary ones only once no interior one is left)
    pb = bnd[perm]
    assert bnd.any() and (~bnd).any() and pb[light].any()
    assert np.all(np.diff(perm[pb]) > 0) and np.all(np.diff(perm[~pb]) > 0)
    for b in range(E):
        if light[b] and not pb[b]:
            assert not pb[b:].any(), b  # no boundary element was left for this light block
        if not light[b] and pb[b]:
            assert pb[b:].all(), b      # no interior element was left for this heavy block


# ---------------------------------------------------------------- validation
def _set(k, v):
    def m(d):
        d[k] = np.array([v], d[k].dtype if k in d else np.int32)
    return m


def _drop(k):
    return lambda d: d.pop(k)


def _face(d):
    return d["face"].reshape(8, -1, order="F")


def _put_face(d, f):
    d["face"] = np.ascontiguousarray(f.ravel(order="F"))


def _edit_face(row, pick, val):
    """face(row+1, f) = val(d, f) for the first face f with pick(face)"""
    def m(d):
        f = _face(d).copy()
        j = int(np.flatnonzero(pick(f))[0])
        f[row, j] = val(d, f, j)
        _put_face(d, f)
    return m


def _split_neighbour(d):  # one neighbour's list as two entries for the same rank
    n = int(d["num_send_recv"][0])
    d["num_nbh"] = np.array([2], np.int32)
    d["nbh_proc"] = np.repeat(d["nbh_proc"][:1], 2)
    d["num_send_recv"] = np.array([n // 2, n - n // 2], np.int32)


def _negative_count(d):
    _split_neighbour(d)
    d["num_send_recv"] = np.array([-1, d["num_send_recv"].sum()], np.int32)


def _lst(i, val):
    def m(d):
        a = d["nbh_send_recv"].copy()
        a[i] = val(d, a)
        d["nbh_send_recv"] = a
    return m


def _both_kinds(d):
    d["num_ghost_send"] = np.ones(int(d["num_nbh"][0]), np.int32)


def _ghost_lists_one_rank(d):
    d.update(halo=np.array([1], np.int32), rank=np.array([0], np.int32), nranks=np.array([1], np.int32),
             num_nbh=np.array([1], np.int32), num_ghost_send=np.array([1], np.int32))


def _third_face_through_a_node(d):  # a boundary face takes the node map of another left face of its element
    ngl, F = int(d["ngl"][0]), int(d["nface"][0])
    f = _face(d)
    m = d["imapl"].reshape(3, ngl, F, order="F").copy()
    for j in np.flatnonzero(f[7] < 0):
        other = [g for g in np.flatnonzero(f[6] == f[6, j]) if g != j]
        if other:
            m[:, :, j] = m[:, :, other[0]]
            d["imapl"] = np.ascontiguousarray(m.ravel(order="F"))
            return
    raise AssertionError("no element with two left faces, one on the boundary")


def _psi(d):
    a = d["psi"].copy()
    a[1] = 0.5
    d["psi"] = a


def _arr(k, i, val):
    def m(d):
        a = d[k].copy()
        a[i] = val(d)
        d[k] = a
    return m


def _ghost_twice(d):
    d["num_nbh"] = np.array([2], np.int32)
    d["nbh_proc"] = np.repeat(d["nbh_proc"][:1], 2)
    for k in ("num_send_recv", "num_ghost_send", "num_ghost_recv"):  # (every per-neighbour array grows)
        d[k] = np.array([d[k][0], 0], np.int32)


def _both(*ms):
    def m(d):
        for x in ms:
            x(d)
    return m


E1 = lambda d: int(d["nelem"][0])  # noqa: E731
REJECTED = [
    ("null_mesh", "single", _set("null_mesh", 1), "null descriptor"),
    ("null_statics", "single", _set("null_statics", 1), "null descriptor"),
    ("null_params", "single", _set("null_params", 1), "null descriptor"),
    ("bad_rank", "face", _set("rank", 2), "bad rank"),
    ("negative_rank", "ghost", _set("rank", -1), "bad rank"),
    ("both_list_kinds", "face", _both_kinds, "not both"),
    ("face_halo_nelem_owned", "face", lambda d: _set("nelem_owned", E1(d) - 1)(d), "every local element is owned"),
    ("face_halo_no_nbh_proc", "face", _drop("nbh_proc"), "needs nbh_proc, num_send_recv, nbh_send_recv"),
    ("face_halo_no_list", "face", _drop("nbh_send_recv"), "needs nbh_proc, num_send_recv, nbh_send_recv"),
    ("nbh_proc_0_based", "face", _arr("nbh_proc", 0, lambda d: d["nbh_proc"][0] - 1), "1-based ranks expected"),
    ("nbh_proc_too_large", "face", _arr("nbh_proc", 0, lambda d: 3), "nbh_proc: bad neighbour rank"),
    ("neighbour_twice", "face", _split_neighbour, "nbh_proc: a neighbour rank is listed twice"),
    ("num_send_recv_negative", "face", _negative_count, "num_send_recv < 0"),
    ("face_id_0", "face", _lst(0, lambda d, a: 0), "face id out of range"),
    ("face_id_large", "face", _lst(-1, lambda d, a: int(d["nface"][0]) + 1), "face id out of range"),
    ("listed_not_processor_face", "face", _lst(0, lambda d, a: int(np.flatnonzero(_face(d)[7] != 0)[0]) + 1),
     "face(8) is not 0"),
    ("face_listed_twice", "face", _lst(1, lambda d, a: a[0]), "processor face is listed twice"),
    ("ghost_lists_one_rank", "single", _ghost_lists_one_rank, "ghost-element lists need nranks > 1"),
    ("nelem_owned_0", "ghost", _set("nelem_owned", 0), "nelem_owned must be in 1..nelem"),
    ("nelem_owned_large", "ghost", lambda d: _set("nelem_owned", E1(d) + 1)(d), "nelem_owned must be in 1..nelem"),
    ("visc1_without_imap_q", "single", _both(_set("method_visc", 1), _drop("imapr_q")), "needs imapl_q/imapr_q"),
    ("visc1_on_ghosts", "ghost", _set("method_visc", 1), "not on ghost elements"),
    ("shear_corrector", "single", _set("shear_corrector", 2), "shear_corrector must be"),
    ("nlayers_4", "single", _set("nlayers", 4), "nlayers must be 1..3"),
    ("nlayers_0", "single", _set("nlayers", 0), "nlayers must be 1..3"),
    ("order_nq", "single", lambda d: _set("nq", int(d["nq"][0]) + 1)(d), "unsupported polynomial order"),
    ("order_ngl", "single", _both(_set("ngl", 7), _set("nq", 13)), "unsupported polynomial order"),
    ("kstages", "single", _set("kstages", 6), "bad kstages/N_btp"),
    ("N_btp", "single", _set("N_btp", 0), "bad kstages/N_btp"),
    ("npoin", "single", lambda d: _set("npoin", int(d["npoin"][0]) + 1)(d), "npoin/npoin_q mismatch"),
    ("npoin_q", "single", lambda d: _set("npoin_q", int(d["npoin_q"][0]) - 1)(d), "npoin/npoin_q mismatch"),
    ("face7_0", "single", _edit_face(6, lambda f: f[7] > 0, lambda d, f, j: 0), "face(7) out of range"),
    ("face7_large", "single", _edit_face(6, lambda f: f[7] > 0, lambda d, f, j: E1(d) + 1), "face(7) out of range"),
    ("face8_large", "single", _edit_face(7, lambda f: f[7] > 0, lambda d, f, j: E1(d) + 1), "face(8) out of range"),
    ("processor_face_unlisted", "single", _edit_face(7, lambda f: f[7] < 0, lambda d, f, j: 0),
     "not in the halo's nbh_send_recv lists"),
    ("processor_face_unlisted_halo", "face", _edit_face(7, lambda f: f[7] < 0, lambda d, f, j: 0),
     "not in the halo's nbh_send_recv lists"),
    ("five_faces", "single", _edit_face(6, lambda f: f[7] < 0, lambda d, f, j: f[6, j] % E1(d) + 1),
     "every element needs exactly 4 faces"),
    ("node_on_three_faces", "single", _third_face_through_a_node, "a node lies on more than two faces"),
    ("psi_not_identity", "single", _psi, "psi is not the identity"),
    ("imapl_q_large", "singleq", _arr("imapl_q", 0, lambda d: int(d["nq"][0]) + 1), "imapl_q/imapr_q out of range"),
    ("imapr_q_0", "singleq", lambda d: _arr("imapr_q", 3 * int(d["nq"][0]) * int(np.flatnonzero(_face(d)[7] > 0)[0]) + 1,
                                           lambda d: 0)(d), "imapl_q/imapr_q out of range"),
    ("ghost_send_a_ghost", "ghost", _arr("ghost_send", 0, E1), "ghost_send must list owned elements"),
    ("ghost_send_0", "ghost", _arr("ghost_send", 0, lambda d: 0), "ghost_send must list owned elements"),
    ("ghost_recv_owned", "ghost", _arr("ghost_recv", 0, lambda d: 1), "ghost_recv must list ghost elements"),
    ("ghost_recv_large", "ghost", _arr("ghost_recv", -1, lambda d: E1(d) + 1), "ghost_recv must list ghost elements"),
    ("ghost_neighbour_self", "ghost", _arr("nbh_proc", 0, lambda d: d["rank"][0]), "bad neighbour rank"),
    ("ghost_neighbour_large", "ghost", _arr("nbh_proc", 0, lambda d: 2), "bad neighbour rank"),
    ("ghost_neighbour_twice", "ghost", _ghost_twice, "a neighbour rank is listed twice"),
]


@pytest.fixture(scope="session")
def valid_dumps(case_factory):
    from hnumo.facepart import face_partition
    from hnumo.partition import partition
    small = dict(nelx=3, nely=3)
    b = case_factory("bump10", **small)
    b4 = case_factory("bump10", nelx=4, nely=4)  # (3x3 does not split over two ranks)
    return {"single": fields_of(b), "singleq": fields_of(case_factory("bump10q", **small)),
            "face": fields_of(face_partition(b4, 2, 0, "block")), "ghost": fields_of(partition(b4, 2, 0))}


@pytest.mark.parametrize("base", ["single", "singleq", "face", "ghost"])
def test_valid_dumps_are_accepted(base, valid_dumps, plan_exe, tmp_path):
    rc, t = run_plan(plan_exe, dict(valid_dumps[base]), str(tmp_path))
    assert rc == 0, t


@pytest.mark.parametrize("name,base,mutate,fragment", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected(name, base, mutate, fragment, valid_dumps, plan_exe, tmp_path):
    """One mutated field of a valid dump (3x3 on one rank, or rank 0 of 4x4 on two): HNUMO_ERR_INVALID with
    the message the engine has always given."""
    d = dict(valid_dumps[base])
    mutate(d)
    rc, t = run_plan(plan_exe, d, str(tmp_path))
    assert rc == INVALID, (rc, sorted(t))
    msg = t["error"].tobytes().rstrip(b"\0").decode()
    assert fragment in msg, msg
