#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly files, kernel by kernel.

    hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only -S pv_kernels.hip -o A.s    (likewise B.s)
    tools/kernel_isa_diff.py A.s B.s

The files are split at the symbols that `.amdhsa_kernel` names.  Of a kernel's body the instruction lines and labels are
compared -- comments, `.loc` / `.file` / `.cfi` and the other directives dropped, the function numbers of local labels
(`.LBB<n>_`) taken out, since they depend on the order of the kernels in the file -- and of its descriptor the
register counts and segment sizes.  Every kernel that differs or exists on one side only is printed; the exit status
is non-zero if there is any.  For a change that must leave the device code alone (host-side refactors).
"""
import re
import sys

DESCRIPTOR = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")


def _normalise(line):
    line = line.split(";", 1)[0].strip()
    if not line:
        return None
    if line.startswith(".") and not line.endswith(":"):  # a directive (.loc, .file, .cfi_*, .section, .p2align, ...)
        return None
    # .LBB12_7 -> .LBB_7, .Lfunc_end12 -> .Lfunc_end: the first number counts functions of the file
    return LOCAL_LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)


def kernels(path):
    """{symbol: (instruction lines, {descriptor field: value})}"""
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    wanted = set(names)
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", lines[i])
        if not m or m.group(1) not in wanted:
            i += 1
            continue
        name, body, desc, in_desc = m.group(1), [], {}, False
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            s = lines[i].strip()
            if s.startswith(".amdhsa_kernel "):
                in_desc = True
            elif s.startswith(".end_amdhsa_kernel"):
                in_desc = False
            elif in_desc:
                f = s.split()
                if len(f) == 2 and f[0].startswith(".amdhsa_") and f[0][len(".amdhsa_"):] in DESCRIPTOR:
                    desc[f[0][len(".amdhsa_"):]] = f[1]
            else:
                n = _normalise(lines[i])
                if n is not None:
                    body.append(n)
            i += 1
        out[name] = (body, desc)
    missing = wanted - set(out)
    if missing:
        sys.exit("%s: no body found for %d kernels, e.g. %s" % (path, len(missing), sorted(missing)[0]))
    return out


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(argv[1]), kernels(argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only in %s: %s" % (argv[2] if name not in a else argv[1], name))
            bad += 1
            continue
        (ia, da), (ib, db) = a[name], b[name]
        why = ["%s %s -> %s" % (k, da.get(k), db.get(k)) for k in DESCRIPTOR if da.get(k) != db.get(k)]
        if ia != ib:
            first = next((j for j, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            why.append("instructions %d -> %d, first difference at line %d of the body" % (len(ia), len(ib), first))
        if why:
            print("differs: %s: %s" % (name, "; ".join(why)))
            bad += 1
    print("%d kernels in %s, %d in %s, %d differ or exist on one side only" % (len(a), argv[1], len(b), argv[2], bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
