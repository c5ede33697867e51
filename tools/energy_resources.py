#!/usr/bin/env python3
"""Resource table of the energy budget's kernel from a build log.

    HNUMO_EXTRA_FLAGS=-Rpass-analysis=kernel-resource-usage h-numo_amd/csrc/build.sh 2> build.log
    python tools/energy_resources.py build.log > profiles/r18/energy_kernel_resources.txt

One line per instantiation of energy_sample_kernel<NGL, L, BOTFR, SERIES> (SERIES 1: with the series' product
rows): VGPRs, SGPRs, scratch bytes per lane (must be 0), LDS bytes per
workgroup and waves per SIMD, as the compiler reports them for gfx950.  Exits 1 if an instantiation
uses scratch.
"""
import re
import sys

PATTERNS = [
    (r"_ZN5hnumo20energy_sample_kernelILi(\d)ELi(\d)ELi(\d)ELb(\d)EE", "energy_sample_kernel<{0},{1},{2},{3}>"),
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
