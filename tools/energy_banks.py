#!/usr/bin/env python3
"""LDS banking of energy_sample_kernel's two interpolation passes (kernels_energy.hip), DESIGN.md §6.1.8.

    python tools/energy_banks.py > profiles/r18/energy_lds_banks.txt

Enumerates, for every ngl the engine accepts, every lane group of every LDS instruction of the two passes
and prints the worst number of distinct addresses that meet on one bank (1: conflict-free).  The rule is
the MI355X's: a ds_read_b64 is served in two groups of 32 lanes with bank = (byte address / 4) mod 64, so
two doubles conflict when their indices agree mod 32 and differ; a ds_write_b64 in four groups of 16
lanes with bank = (byte address / 4) mod 32, indices mod 16.  Equal addresses broadcast.

Pass 1, lane (e, n, iq) (iq fastest): reads tile[e*P + n*ngl + m] for m = 0..ngl-1 (down the column n of
the element's tile, lanes of different n lie ngl doubles apart) and writes t[e*TS + n*nq + iq].
Pass 2, lane (e, jq, iq): reads t[e*TS + n*nq + iq] for n = 0..ngl-1 (lanes of different jq read the same
address; a step of n moves every lane nq doubles).  TS = en_tstride(ngl) is the element stride of t.
"""
NGLS = (3, 4, 5, 6, 8)
BS = 256


def tstride(ngl, padded=True):
    """en_tstride of energy_plan.h"""
    nq = 2 * ngl - 1
    return nq * ngl + (16 if padded and ngl in (4, 6) else 0)


def worst(addr_of_lane, nlanes, group, mod):
    w = 1
    for g0 in range(0, BS, group):
        banks = {}
        for lane in range(g0, min(g0 + group, nlanes)):
            a = addr_of_lane(lane)
            banks.setdefault(a % mod, set()).add(a)
        w = max([w] + [len(s) for s in banks.values()])
    return w


def passes(ngl, padded):
    nq = 2 * ngl - 1
    P, Q, T1, TS = ngl * ngl, nq * nq, nq * ngl, tstride(ngl, padded)
    epg = BS // Q
    p1 = lambda lane: (lane // T1, (lane % T1) // nq, lane % nq)
    p2 = lambda lane: (lane // Q, (lane % Q) // nq, lane % nq)
    r1 = max(worst(lambda l: p1(l)[0] * P + p1(l)[1] * ngl + m, epg * T1, 32, 32) for m in range(ngl))
    w1 = worst(lambda l: p1(l)[0] * TS + p1(l)[1] * nq + p1(l)[2], epg * T1, 16, 16)
    r2 = max(worst(lambda l: p2(l)[0] * TS + n * nq + p2(l)[2], epg * Q, 32, 32) for n in range(ngl))
    return epg, TS, r1, w1, r2


if __name__ == "__main__":
    print(f"{'ngl':>3s} {'nq':>3s} {'elements/group':>14s} {'TS':>4s} {'pass 1 read':>12s} {'pass 1 write':>13s} {'pass 2 read':>12s}"
          f"   unpadded: {'TS':>4s} {'p1 write':>9s} {'p2 read':>8s}")
    for ngl in NGLS:
        epg, TS, r1, w1, r2 = passes(ngl, True)
        _, TS0, _, w10, r20 = passes(ngl, False)
        print(f"{ngl:3d} {2 * ngl - 1:3d} {epg:14d} {TS:4d} {r1:12d} {w1:13d} {r2:12d}             {TS0:4d} {w10:9d} {r20:8d}")
