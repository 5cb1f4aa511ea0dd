#!/usr/bin/env python3
"""isa_equal.py BASE.s NEW.s: do two `hipcc -S` outputs hold the same code, function by function?

A function is the text from its label (one declared `.type NAME,@function`) to its resource summary:
the instructions, a kernel's .amdhsa_kernel descriptor and the .set lines of its register counts. It
is compared as text after dropping comments, .section/.globl/.type/.p2align lines and the per-function
numbers of local labels, which shift whenever a function is added or removed. The tables that list
every kernel (metadata, dynamic-LDS offsets) are not functions and are not compared.
Exit 1 if a function differs or NEW has one that BASE lacks (other than __hip_cuid_*).

A renamed function (a dropped template parameter changes the mangled name) counts as one that BASE
lacks. The report says when its text equals that of a function only BASE has, apart from the name
itself; to get exit 0 then, rename the symbol in a copy of BASE.s (sed 's/OLD/NEW/g') and compare
against the copy."""
import re
import sys

DECL = re.compile(r"^\s*\.type\s+(\S+),@function")
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
LOCAL = re.compile(r"\.(LBB|LJTI|Lfunc_end|Lfunc_begin|Ltmp)\d+")
DROP = re.compile(r"^\.(section|globl|type|p2align)\b")


def functions(path):
    out, declared, name = {}, set(), None
    for line in open(path):
        m = DECL.match(line)
        if m:
            declared.add(m.group(1))
        m = LABEL.match(line)
        if m:
            name = m.group(1) if m.group(1) in declared else None
            if name:
                out[name] = []
        if ".AMDGPU.csdata" in line:   # the function's (comment-only) summary follows: its text ends
            name = None
        line = LOCAL.sub(r".\1", line.split(";")[0]).strip()
        if name and line and not DROP.match(line):
            out[name].append(line)
    return out


def anonymous(name, lines):
    return [l.replace(name, "<self>") for l in lines]


base, new = functions(sys.argv[1]), functions(sys.argv[2])
gone = sorted(set(base) - set(new))
added = sorted(set(new) - set(base))
differ = sorted(f for f in set(base) & set(new) if base[f] != new[f])
print(f"functions: {len(base)} in BASE, {len(new)} in NEW, {len(differ)} differ")
for title, names in (("only in BASE", gone), ("only in NEW", added), ("DIFFER", differ)):
    for f in names:
        print(f"{title}: {f}")
        if title == "only in NEW":
            for g in gone:
                if anonymous(g, base[g]) == anonymous(f, new[f]):
                    print(f"  (same text as BASE's {g}, apart from the name: a rename)")
sys.exit(1 if differ or any(not f.startswith("__hip_cuid_") for f in added) else 0)
