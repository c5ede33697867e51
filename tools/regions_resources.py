#!/usr/bin/env python3
"""Resource table of the region sets' kernels from a build log.

    HNUMO_EXTRA_FLAGS=-Rpass-analysis=kernel-resource-usage h-numo_amd/csrc/build.sh 2> build.log
    python tools/regions_resources.py build.log > profiles/r19/regions_kernel_resources.txt

One line per instantiation of region_accumulate_kernel<NGL, L, ROWS> (ROWS 1: FLOW, 2: VORT, 3: both), and one
each for region_area_kernel, region_tree_kernel and stats_tree_kernel (which shares tree_halve with it): VGPRs,
SGPRs, scratch bytes per lane (must be 0), LDS bytes per workgroup and waves per SIMD, as the compiler reports
them for gfx950.  Exits 1 if an instantiation uses scratch.
"""
import re
import sys

PATTERNS = [
    (r"_ZN5hnumo24region_accumulate_kernelILi(\d)ELi(\d)ELi(\d)EE", "region_accumulate_kernel<{0},{1},{2}>"),
    (r"_ZN5hnumo18region_area_kernelE", "region_area_kernel"),
    (r"_ZN5hnumo18region_tree_kernelE", "region_tree_kernel"),
    (r"_ZN5hnumo17stats_tree_kernelE", "stats_tree_kernel"),
]


def main(path):
    text = open(path).read()
    rows = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", text)[1:]:
        name = b.split()[0]
        for pat, fmt in PATTERNS:
            m = re.match(pat, name)
            if m:
                get = lambda k: int(re.search(k + r": (\d+)", b).group(1))
                rows[fmt.format(*m.groups())] = (get("VGPRs"), get("SGPRs"), get(r"ScratchSize \[bytes/lane\]"),
                                                 get(r"LDS Size \[bytes/block\]"), get(r"Occupancy \[waves/SIMD\]"))
    print(f"{'kernel':40s} {'VGPRs':>6s} {'SGPRs':>6s} {'scratch':>8s} {'LDS B':>7s} {'waves/SIMD':>11s}")
    for k in sorted(rows):
        print(f"{k:40s} " + " ".join(f"{v:>{w}d}" for v, w in zip(rows[k], (6, 6, 8, 7, 11))))
    return 1 if not rows or any(r[2] for r in rows.values()) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
