#!/usr/bin/env python3
"""Resource table of the eddy-covariance kernels from a build log.

    HNUMO_EXTRA_FLAGS=-Rpass-analysis=kernel-resource-usage h-numo_amd/csrc/build.sh 2> build.log
    python tools/cov_resources.py build.log > profiles/r17/cov_kernel_resources.txt

One line per instantiation of cov_accumulate_kernel<NGL, L>, cov_fields_kernel<L>, cov_integrals_kernel<L>
and sample_kernel<NGL, L, SP_SRC_COV>: VGPRs, SGPRs, scratch bytes per lane (must be 0), LDS bytes per
workgroup and waves per SIMD, as the compiler reports them for gfx950.  Exits 1 if an instantiation
uses scratch.
"""
import re
import sys

PATTERNS = [
    (r"_ZN5hnumo21cov_accumulate_kernelILi(\d)ELi(\d)EE", "cov_accumulate_kernel<{0},{1}>"),
    (r"_ZN5hnumo17cov_fields_kernelILi(\d)EE", "cov_fields_kernel<{0}>"),
    (r"_ZN5hnumo20cov_integrals_kernelILi(\d)EE", "cov_integrals_kernel<{0}>"),
    (r"_ZN5hnumo13sample_kernelILi(\d)ELi(\d)ELi3EE", "sample_kernel<{0},{1},SP_SRC_COV>"),
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
