#!/usr/bin/env python3
"""Compare the kernel bodies of two `make asm` outputs of one source file.

    python scripts/asm_bodies.py PARENT.s THIS.s

A body is the text from a kernel's label line to its `.Lfunc_end` line, both
left out: the label carries the mangled name and `.Lfunc_end` the function's
ordinal, which move when a template gains a parameter or a kernel is added.
Bodies are compared line by line as they are, except that a kernel's own
mangled name (in its `.amdhsa_kernel` and `.section` lines) reads `@SELF`, and
the function's ordinal in its block labels (`.LBB26_4`, `Header=BB26_16`) reads
`@`: it moves, like `.Lfunc_end`'s, when kernels are emitted ahead of it.
Kernels are matched by their demangled name with the template arguments that
are `false` at the end of the list dropped, so `k_batch<1, false>` of one tree
meets `k_batch<1, false, false>` of the other.  Prints one markdown table row
per kernel and exits 1 if a kernel both trees have differs or one is gone.
"""
import re
import subprocess
import sys

ORDINAL = re.compile(r"BB\d+_(\d+)\b")


def bodies(path):
    lines = open(path).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):\s", lines[i] + " ")
        if m and i and ".type" in "".join(lines[max(0, i - 4):i]) and "@function" in "".join(lines[max(0, i - 4):i]):
            j = i + 1
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            out[m.group(1)] = [ORDINAL.sub(r"BB@_\1", ln.replace(m.group(1), "@SELF")) for ln in lines[i + 1:j]]
            i = j
        i += 1
    return out


def demangle(names):
    got = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, got.split("\n")))


def key(name):
    name = re.sub(r"^void ", "", name).replace("lpk::(anonymous namespace)::", "")
    name = re.sub(r"\(.*$", "", name)
    while name.endswith(", false>"):
        name = name[:-len(", false>")] + ">"
    return name


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    da, db = demangle(list(a)), demangle(list(b))
    ka = {key(da[s]): a[s] for s in a}
    kb = {key(db[s]): b[s] for s in b}
    bad = 0
    print("| kernel | lines, parent | lines, this tree | lines that differ |")
    print("|---|---|---|---|")
    for k in kb:
        if k not in ka:
            print(f"| `{k}` | (new) | {len(kb[k])} | |")
            continue
        x, y = ka[k], kb[k]
        d = sum(1 for p, q in zip(x, y) if p != q) + abs(len(x) - len(y))
        bad += d != 0
        print(f"| `{k}` | {len(x)} | {len(y)} | {d} |")
    for k in ka:
        if k not in kb:
            print(f"| `{k}` | {len(ka[k])} | (gone) | |")
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
