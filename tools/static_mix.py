"""Static instruction mix of one kernel in `hipcc -S` output, whole and for its widest loop (for
btp_subcycle_kernel that is the later-stage loop: the stage body inlined with FST = 2).

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -ffp-contract=off \
      --cuda-device-only -S -o engine.s h-numo_amd/csrc/engine.hip
  python tools/static_mix.py engine.s btp_subcycle_kernelILi5ELi9ELb0E

Instructions are classified by generic prefixes only (v_, s_, ds_, the _f64 suffix).  The counts
are static: not weighted by trip counts or active waves."""
import collections
import re
import sys


def kernel_lines(path, key):
    body, name = None, None
    for ln in open(path):
        if body is None:
            m = re.match(r"^(\w+):", ln)
            if m and key in m.group(1) and not m.group(1).startswith("."):
                body, name = [], m.group(1)
        else:
            if ln.startswith("\t.end_amdhsa_kernel") or ln.startswith(".Lfunc_end"):
                break
            body.append(ln.rstrip("\n"))
    if body is None:
        sys.exit(f"no kernel matching {key!r}")
    return name, body


def kernel_info(path, name):
    """the compiler's resource figures of the kernel ('; Kernel info:' block behind its code)"""
    seen, out = False, []
    for ln in open(path):
        if ln.startswith(name + ":"):
            seen = True
        elif seen and re.match(r"^; (TotalNumVgprs|NumVgprs|NumSgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize)", ln):
            out.append(ln[2:].split(" bytes")[0].strip())
            if ln.startswith("; LDSByteSize"):
                break
    return out


def classify(op):
    if op.startswith("v_"):
        return "f64 VALU" if "_f64" in op else "other VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "scalar loads"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("s_"):
        return "SALU / control"
    return "vector memory"


def mix(lines):
    c, ops = collections.Counter(), collections.Counter()
    for ln in lines:
        m = re.match(r"^\t([a-z]\w+)", ln)
        if not m:
            continue
        c["all"] += 1
        c[classify(m.group(1))] += 1
        ops[m.group(1)] += 1
    return c, ops


def widest_loop(lines):
    pos = {m.group(1): i for i, ln in enumerate(lines) if (m := re.match(r"^(\.LBB\w+):", ln))}
    best = (0, 0)
    for i, ln in enumerate(lines):
        m = re.match(r"^\ts_c?branch\w*\s+(\.LBB\w+)", ln)
        if m and pos.get(m.group(1), i) < i and i - pos[m.group(1)] > best[1] - best[0]:
            best = (pos[m.group(1)], i)
    return lines[best[0]:best[1] + 1]


def main():
    path, key = sys.argv[1], sys.argv[2]
    name, body = kernel_lines(path, key)
    print(name)
    print("  " + "  ".join(kernel_info(path, name)))
    for title, lines in (("whole kernel", body), ("widest loop", widest_loop(body))):
        c, ops = mix(lines)
        print(f"-- {title}")
        for k in ("all", "f64 VALU", "other VALU", "SALU / control", "scalar loads", "s_waitcnt", "LDS", "vector memory"):
            print(f"  {k:16s} {c[k]}")
        top = ", ".join(f"{o} {n}" for o, n in ops.most_common() if o.startswith(("v_cndmask", "v_add_u32", "v_lshl", "s_and_saveexec", "s_cbranch_execz", "v_mul_hi", "v_mad_u")))
        print(f"  index / control detail: {top}")


if __name__ == "__main__":
    main()
