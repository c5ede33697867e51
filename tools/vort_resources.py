#!/usr/bin/env python3
"""Resource table of the vorticity kernels from a build log.

    HNUMO_EXTRA_FLAGS=-Rpass-analysis=kernel-resource-usage h-numo_amd/csrc/build.sh 2> build.log
    python tools/vort_resources.py build.log > profiles/r12/vort_kernel_resources.txt

One line per instantiation of vort_kernel<NGL, L, SERIES> and of sample_kernel<NGL, L, SP_SRC_VORT>:
VGPRs, SGPRs, scratch bytes per lane (must be 0), LDS bytes per workgroup and waves per SIMD, as the
compiler reports them for gfx950.  Exits 1 if an instantiation uses scratch.
"""
import re
import sys


def main(path):
    text = open(path).read()
    rows = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", text)[1:]:
        name = b.split()[0]
        m = re.match(r"_ZN5hnumo11vort_kernelILi(\d)ELi(\d)ELb([01])E", name)
        s = re.match(r"_ZN5hnumo13sample_kernelILi(\d)ELi(\d)ELi2EE", name)
        if not m and not s:
            continue
        get = lambda k: int(re.search(k + r": (\d+)", b).group(1))
        key = (f"vort_kernel<{m[1]},{m[2]},{'true' if m[3] == '1' else 'false'}>" if m
               else f"sample_kernel<{s[1]},{s[2]},SP_SRC_VORT>")
        rows[key] = (get("VGPRs"), get("SGPRs"), get(r"ScratchSize \[bytes/lane\]"), get(r"LDS Size \[bytes/block\]"),
                     get(r"Occupancy \[waves/SIMD\]"))
    print(f"{'kernel':40s} {'VGPRs':>6s} {'SGPRs':>6s} {'scratch':>8s} {'LDS B':>7s} {'waves/SIMD':>11s}")
    for k in sorted(rows):
        print(f"{k:40s} " + " ".join(f"{v:>{w}d}" for v, w in zip(rows[k], (6, 6, 8, 7, 11))))
    return 1 if not rows or any(r[2] for r in rows.values()) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
