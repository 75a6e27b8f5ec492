"""Developer tool (CPU): which kernels of two device assemblies of the library are the same instruction for instruction.

usage: python tools/isa_same_kernels.py [--mask-registers] OLD.s NEW.s

An assembly of the library is the concatenation of its translation units' (a kernel is instantiated in one unit, so none appears twice):
    make -C pbrs_amd/csrc asm ASMDIR=/tmp/new && cat /tmp/new/*.s > NEW.s
and the same in a checkout of the other tree.  A tree from before the split has one unit: hipcc <the Makefile's flags>
--cuda-device-only -S -o OLD.s pbrs_gpu.hip.

A counter file (profiles/*traffic*.json) is stamped with a hash of ALL kernel sources; a change to one header moves the hash although
most kernels compile to the same code.  This tool compares every kernel's body (label .. .Lfunc_end, local labels renumbered in order of
appearance, comments and debug directives dropped) and its resource directives (registers, scratch, LDS) and prints the kernels that
differ: a counter file may then name the new hash under `same_isa_as_measured` for the kernels this tool finds unchanged.

--mask-registers gives the kernels that differ a second comparison with every register number masked (v12, s3, a0, v[4:7] -> v#, s#, a#,
v[#+3]): the same opcodes in the same order on the same operands' kinds and widths, with equal resource directives — what a source-level
refactor may leave behind when two values swap their registers.  Those kernels are listed by name and are NOT unchanged for a counter file.
The exit status is 1 when a kernel is in neither class (without the option: when any kernel differs)."""
import hashlib
import re
import subprocess
import sys


def kernels(path):
    out, cur, name = {}, None, None
    for line in open(path, errors="replace"):
        s = line.split(";")[0].rstrip()
        if not s.strip():
            continue
        m = re.match(r"^(_Z\w+):", s)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if s.startswith(".Lfunc_end"):
                out[name] = cur
                cur = None
                continue
            t = s.strip()
            # (a template kernel's descriptor block stands before its .Lfunc_end: the two lines of it that name the kernel are no code)
            if t.startswith((".loc", ".file", ".cfi", ".p2align", ".amdhsa_kernel ", ".section")):
                continue
            cur.append(t)
    # resource directives: the .amdhsa_kernel blocks
    res, k = {}, None
    for line in open(path, errors="replace"):
        t = line.strip()
        if t.startswith(".amdhsa_kernel "):
            k = t.split()[1]
            res[k] = []
        elif t == ".end_amdhsa_kernel":
            k = None
        elif k:
            res[k].append(t)
    return out, res


MASK = "--mask-registers" in sys.argv[1:]
ARGS = [x for x in sys.argv[1:] if x != "--mask-registers"]
if len(ARGS) != 2:
    sys.exit(__doc__)


def mask(line):
    line = re.sub(r"\b([vsa])\[(\d+):(\d+)\]", lambda m: "%s[#+%d]" % (m.group(1), int(m.group(3)) - int(m.group(2))), line)
    return re.sub(r"\b([vsa])\d+\b", r"\1#", line)


def canon(body, masked=False):
    ids = {}

    def ren(m):
        return ids.setdefault(m.group(0), ".L%d" % len(ids))
    return hashlib.sha256("\n".join(re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", ren, mask(l) if masked else l) for l in body).encode()).hexdigest()[:16]


def demangle(names):
    try:
        return dict(zip(names, subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt"] + names, capture_output=True, text=True).stdout.splitlines()))
    except OSError:
        return {n: n for n in names}


a, ra = kernels(ARGS[0])
b, rb = kernels(ARGS[1])
names = sorted(set(a) | set(b))
dm = demangle(names)
short = {n: dm[n].split("(")[0] for n in names}
same, diff = [], []
for n in names:
    if n in a and n in b and canon(a[n]) == canon(b[n]) and ra.get(n) == rb.get(n):
        same.append(n)
    elif n in a and n in b:
        diff.append(n)
# a kernel on one side only may be a renamed one: pair the leftovers of the two sides whose body and resource directives are equal (a
# kernel's body does not name its own symbol), in name order where several are alike
renamed, left = [], {}
for n in sorted(set(b) - set(a)):
    left.setdefault((canon(b[n]), tuple(rb.get(n, ()))), []).append(n)
for n in sorted(set(a) - set(b)):
    twins = left.get((canon(a[n]), tuple(ra.get(n, ()))))
    if twins:
        renamed.append((n, twins.pop(0)))
    else:
        diff.append(n)
diff += [n for twins in left.values() for n in twins]
masked = [n for n in diff if MASK and n in a and n in b and canon(a[n], True) == canon(b[n], True) and ra.get(n) == rb.get(n)]
diff = [n for n in diff if n not in masked]
pairs = f" ({len(renamed)} of them renamed)" if renamed else ""
also = f", same once register numbers are masked {len(masked)}" if MASK else ""
print(f"kernels {len(same) + len(renamed) + len(masked) + len(diff)}: same {len(same) + len(renamed)}{pairs}{also}, different {len(diff)}")
for old, new in renamed:
    print("  renamed:", short[old], "->", short[new])
for n in sorted(masked):
    print("  same once masked:", dm[n].split("(")[0])
for n in sorted(diff):
    why = "only in one" if not (n in a and n in b) else f"{len(a[n])} -> {len(b[n])} lines"
    print("  differs:", short[n], f"({why})")
sys.exit(1 if diff else 0)
