"""The host-only plan of a region set (h-numo_amd/csrc/region_plan.h): validation, the member list, and the
chunk descriptors of the segmented tree, run on the CPU.

tests/region_plan_main.cpp includes the header; this module compiles it once per session with
AddressSanitizer and UBSan into a temporary directory and runs it as a child process on dumps of labels and
partials (the record format of tests/test_sample_plan.py).  Nothing is loaded into Python.  Expectations
come from the labels themselves: the members of region r are flatnonzero(labels == r), and a region's value
is flowstats.tree_sum of its members' partials in that order -- the descriptors are judged both by their
invariants and by replaying them in numpy, and region_tree_host's walk of them bit for bit against tree_sum.

Region sizes: 0, 1, 1023, 1024, 1025 (the chunk boundary), 1100 beside 268 and 1 (two passes for one region,
one for the others, a ragged second chunk), and one region of 1024*1024 + 3 (three passes)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from hnumo.flowstats import tree_sum

HERE = os.path.dirname(os.path.abspath(__file__))
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="no g++ to compile tests/region_plan_main.cpp with")

INVALID = 3  # exit status of region_plan_main for HNUMO_ERR_INVALID
CHUNK = 1024
BIG = 1024 * 1024 + 3


@pytest.fixture(scope="session")
def region_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("region_plan") / "region_plan_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "region_plan_main.cpp"), "-o", exe], check=True)
    return exe


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


def run(exe, d, tmp):
    """(exit status, records) of one run; a sanitizer report fails the test."""
    tmp = str(tmp)
    write_dump(os.path.join(tmp, "in.bin"), d)
    r = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], capture_output=True, text=True)
    assert r.returncode in (0, INVALID) and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.returncode, read_dump(os.path.join(tmp, "out.bin"))


def i32(*v):
    return np.array(v, np.int32)


def labels_of(sizes, unlabelled, seed):
    """int32 labels with sizes[r-1] elements of region r and `unlabelled` zeros, shuffled"""
    lab = np.concatenate([np.full(n, r + 1, np.int32) for r, n in enumerate(sizes)] + [np.zeros(unlabelled, np.int32)])
    np.random.default_rng(seed).shuffle(lab)
    return lab


def inputs(lab, R, mask=1, **kw):
    d = {"labels": lab, "nelem_owned": i32(lab.size), "R": i32(R), "mask": i32(mask)}
    d.update(kw)
    return d


def passes(o):
    """[(nin, nout, desc (nchunks, 4))] of an output"""
    sizes, desc = o["pass_sizes"].reshape(-1, 3), o["desc"].reshape(-1, 4)
    out, at = [], 0
    for nch, nin, nout in sizes:
        out.append((int(nin), int(nout), desc[at:at + nch]))
        at += nch
    assert at == desc.shape[0]
    return out


def expected_passes(nmax):
    p, n = 1, -(-nmax // CHUNK)
    while n > 1:
        p, n = p + 1, -(-n // CHUNK)
    return p


CASES = [([0], 5), ([1], 3), ([1023], 0), ([1024], 7), ([1025], 2), ([1100, 268, 1], 40), ([5, 0, 1100, 0], 1), ([BIG], 11)]


@pytest.mark.parametrize("sizes,unlabelled", CASES)
def test_tables_descriptors_and_host_tree(region_exe, tmp_path, sizes, unlabelled):
    R = len(sizes)
    lab = labels_of(sizes, unlabelled, seed=sum(sizes) + R)
    ne = lab.size
    rng = np.random.default_rng(7)
    rows = 2
    # partials of mixed magnitude and sign per ELEMENT: any other order of adding them shows in the bits
    x = rng.standard_normal((rows, ne)) * 10.0 ** rng.integers(-6, 7, (rows, ne))
    members = [np.flatnonzero(lab == r) for r in range(1, R + 1)]
    mem = np.concatenate(members) if members else np.zeros(0, np.int64)
    rc, o = run(region_exe, inputs(lab, R, rows=i32(rows), part=np.ascontiguousarray(x[:, mem])), tmp_path)
    assert rc == 0
    assert o["scalars"].tolist() == [R, 1, CHUNK, 4, expected_passes(max(sizes)), 16]
    # the tables, from the labels
    assert np.array_equal(o["members"], mem)
    assert np.array_equal(o["offset"], np.concatenate([[0], np.cumsum(sizes)]))
    slot = np.full(ne, -1)
    slot[mem] = np.arange(mem.size)
    assert np.array_equal(o["slot"], slot)
    # the descriptors: invariants, and a replay in numpy
    ps = passes(o)
    assert len(ps) == expected_passes(max(sizes)) >= 1
    entry = np.full((rows, R), np.nan)
    finals = np.zeros(R, int)
    vals, nin_want = np.ascontiguousarray(x[:, mem]), mem.size
    span = {r: (int(o["offset"][r]), sizes[r]) for r in range(R)}       # region -> (start, count) in the pass' input
    for p, (nin, nout, desc) in enumerate(ps):
        assert nin == nin_want and (desc[:, 1] <= CHUNK).all() and (desc[:, 1] >= 0).all()
        read = np.zeros(nin, int)
        nxt = np.full((rows, nout), np.nan)
        wrote = np.zeros(nout, int)
        at = 0
        new_span = {}
        for r in range(R):
            start, cnt = span.get(r, (0, -1))
            if cnt < 0:
                continue                                                      # finished in an earlier pass: untouched
            if cnt == 0:
                assert p == 0 and desc[at].tolist() == [0, 0, r, 1]           # an empty region: one zero write
                entry[:, r], finals[r] = 0.0, finals[r] + 1
                at += 1
                continue
            nch = -(-cnt // CHUNK)
            for c in range(nch):
                s, n, out, fin = desc[at + c]
                assert s == start + c * CHUNK and n == min(CHUNK, cnt - c * CHUNK) and fin == (nch == 1)
                read[s:s + n] += 1
                v = [tree_sum(vals[row, s:s + n]) for row in range(rows)]
                if fin:
                    assert out == r
                    entry[:, r], finals[r] = v, finals[r] + 1
                else:
                    nxt[:, out], wrote[out] = v, wrote[out] + 1
                    if c == 0:
                        new_span[r] = (int(out), nch)
                    assert out == new_span[r][0] + c                          # a region's results lie side by side
            at += nch
        assert at == desc.shape[0]
        assert (read == 1).all()                                              # every input value read exactly once
        assert (wrote == 1).all()
        span, vals, nin_want = new_span, nxt, nout
    assert not span and (finals == 1).all() and ps[-1][1] == 0
    want = np.array([[tree_sum(x[row, m]) for m in members] for row in range(rows)])
    assert np.array_equal(entry, want)                                        # the descriptors are the tree
    got = o["entry"].reshape(rows, R)
    assert np.array_equal(got, want), (got, want)                             # region_tree_host, bit for bit
    for r, n in enumerate(sizes):
        if n == 0:
            assert not got[:, r].any() and not np.signbit(got[:, r]).any()    # +0.0
    assert o["levels"][0] >= max([1] + [nout for _, nout, _ in ps[0::2]])
    assert o["levels"][1] >= max([1] + [nout for _, nout, _ in ps[1::2]])


def test_order_within_a_region_is_the_element_order(region_exe, tmp_path):
    """Reversing which elements carry a region's partials changes the bits: the local position is the rank of
    the element number among the region's members, not the order of labelling."""
    lab = labels_of([37, 12], 9, seed=3)
    x = np.random.default_rng(1).standard_normal(lab.size) * 10.0 ** np.arange(lab.size)[::-1].clip(0, 12)
    mem = np.concatenate([np.flatnonzero(lab == 1), np.flatnonzero(lab == 2)])
    _, o = run(region_exe, inputs(lab, 2, rows=i32(1), part=np.ascontiguousarray(x[mem])), tmp_path)
    assert o["entry"][0] == tree_sum(x[lab == 1]) and o["entry"][1] == tree_sum(x[lab == 2])
    assert o["entry"][0] != tree_sum(x[lab == 1][::-1])


def err_text(o):
    return o["error"].tobytes().rstrip(b"\0").decode()


def test_each_failure_exit_names_the_call_and_the_value(region_exe, tmp_path):
    lab = labels_of([5, 3], 2, seed=0)
    good = inputs(lab, 2)
    assert run(region_exe, good, tmp_path)[0] == 0
    bad = lab.copy()
    bad[4] = 3
    neg = lab.copy()
    neg[7] = -1
    cases = [
        ({k: v for k, v in good.items() if k != "labels"} | {"n": i32(10)}, "region_of_elem is NULL"),
        (inputs(lab, 0), "nregions must be >= 1, got 0"),
        (inputs(lab, 2) | {"nelem_owned": i32(11)}, "n must be nelem_owned = 11, got 10"),
        (inputs(lab, 2, mask=0), "rows_mask must hold HNUMO_REGION_FLOW (1), HNUMO_REGION_VORT (2) or both, got 0"),
        (inputs(lab, 2, mask=4), "got 4"),
        (inputs(lab, 2, mask=7), "got 7"),
        (inputs(bad, 2), "region_of_elem(5) = 3 is outside 0..2"),
        (inputs(neg, 2), "region_of_elem(8) = -1 is outside 0..2"),
    ]
    for d, text in cases:
        rc, o = run(region_exe, d, tmp_path)
        assert rc == INVALID, text
        msg = err_text(o)
        assert msg.startswith("hnumo_regions_create: ") and text in msg, (msg, text)
    # the order is fixed: nregions before n before the mask before the labels
    rc, o = run(region_exe, inputs(bad, 0, mask=0) | {"nelem_owned": i32(11)}, tmp_path)
    assert "nregions" in err_text(o)
    rc, o = run(region_exe, inputs(bad, 2, mask=0) | {"nelem_owned": i32(11)}, tmp_path)
    assert "nelem_owned" in err_text(o)
    rc, o = run(region_exe, inputs(bad, 2, mask=0), tmp_path)
    assert "rows_mask" in err_text(o)
