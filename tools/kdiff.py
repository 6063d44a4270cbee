#!/usr/bin/env python3
"""Did moving code between translation units change any kernel?  Two sets of units in, the table out.

    python tools/kdiff.py OLD[,OLD...] NEW[,NEW...] [-DNAME=V ...] [--list]

Each side is a comma-separated list of sources: `path.hip` of this tree, `REV:path.hip` (the file as it is in that git
revision, compiled beside that revision's headers) or `path.s` (device assembly made elsewhere).  Sources are compiled the way
the library is (csrc/build.py FLAGS + the unit's UNIT_FLAGS, hipcc -S --cuda-device-only).  Kernels are matched by mangled
symbol; the four resource counts are read from each symbol's .amdhsa_next_free_vgpr / _next_free_sgpr /
_group_segment_fixed_size / _private_segment_fixed_size; instruction sequences are compared with branch labels masked and
comments dropped.  A symbol that every file of a side with several files carries (what fq_common.h gives each unit) is set
aside.  The comparison is of sequences and counts only: it knows no instruction by name.  Exit status 0: symbol sets equal,
every count equal, every sequence identical."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantization.mxnet_amd.csrc import build  # noqa: E402

CSRC = os.path.relpath(build.HERE, ROOT)
COUNTS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def assembly(spec, defs, tmp):
    """The device assembly text of one source of a side."""
    if spec.endswith(".s"):
        return open(spec).read()
    inc = build.HERE
    src = os.path.abspath(spec)
    if ":" in spec:                                            # REV:path - that revision's csrc, exported once per revision
        rev, path = spec.split(":", 1)
        inc = os.path.join(tmp, re.sub(r"\W", "_", rev))
        if not os.path.isdir(inc):
            os.makedirs(inc)
            tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC], check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", inc, "--strip-components=%d" % (CSRC.count(os.sep) + 1)], input=tar, check=True)
        src = os.path.join(inc, os.path.basename(path))
    unit = os.path.splitext(os.path.basename(src))[0]
    flags = [f for f in build.FLAGS[:-1] if f != "-fPIC"] + [inc] + build.UNIT_FLAGS.get(unit, [])
    out = os.path.join(tmp, "%s_%s.s" % (os.path.basename(inc), unit))
    subprocess.run([build.hipcc()] + flags + defs + ["-S", "--cuda-device-only", src, "-o", out], check=True, capture_output=True)
    return open(out).read()


def kernels(text):
    """{symbol: (counts, [instruction lines])} of one assembly file."""
    found = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        sym, desc = m.group(1), m.group(2)
        counts = tuple(int(re.search(r"\.amdhsa_%s (\d+)" % c, desc).group(1)) for c in COUNTS)
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), text, re.S | re.M).group(1)
        seq = []
        for line in body.splitlines():
            t = line.split(";")[0].strip()
            if not t or t.startswith(".") and not t.endswith(":"):
                continue
            seq.append(re.sub(r"\.LBB\d+_\d+", ".L", " ".join(t.split())))
        found[sym] = (counts, seq)
    return found


def side(specs, defs, tmp):
    files = [(s, kernels(assembly(s, defs, tmp))) for s in specs]
    common = set.intersection(*[set(k) for _, k in files]) if len(files) > 1 else set()
    where = collections.defaultdict(list)
    for s, ks in files:
        for sym in ks:
            if sym not in common:
                where[sym].append(s)
    merged = {sym: dict(files)[ss[0]][sym] for sym, ss in where.items()}
    return merged, where, common, files


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    defs = [a for a in sys.argv[1:] if a.startswith("-D")]
    with tempfile.TemporaryDirectory() as tmp:
        old, _, old_common, _ = side(args[0].split(","), defs, tmp)
        new, where, new_common, files = side(args[1].split(","), defs, tmp)
    for sym in old_common | new_common:                        # set aside on one side: on the other too
        old.pop(sym, None), new.pop(sym, None), where.pop(sym, None)
    for s, ks in files:
        print("%-40s %4d kernels" % (s, len([k for k in ks if k not in new_common])))
    if old_common or new_common:
        print("set aside (in every file of a side): %d old, %d new" % (len(old_common), len(new_common)))
    twice = sorted(sym for sym, ss in where.items() if len(ss) > 1)
    lost, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    print("symbols: %d old, %d new, %d lost, %d added, %d in two units" % (len(old), len(new), len(lost), len(added), len(twice)))
    for tag, syms in (("lost", lost), ("added", added), ("twice", twice)):
        for sym in syms:
            print("  %s %s" % (tag, sym))
    table, moved = collections.Counter(), []
    for sym in sorted(set(old) & set(new)):
        (c0, s0), (c1, s1) = old[sym], new[sym]
        if c0 != c1:
            moved.append((sym, c0, c1))
        ops0, ops1 = (collections.Counter(x.split()[0] for x in s) for s in (s0, s1))
        kind = "identical" if s0 == s1 else "renamed" if ops0 == ops1 else "differs"
        table[kind] += 1
        if kind != "identical" and "--list" in sys.argv:
            print("  %s %s" % (kind, sym))
    print("counts (%s): %d symbols moved one" % (", ".join(COUNTS), len(moved)))
    for sym, c0, c1 in moved:
        print("  %s %r -> %r" % (sym, c0, c1))
    print("  identical instruction sequence                        %4d" % table["identical"])
    print("  same opcode counts, registers renamed / order differs %4d" % table["renamed"])
    print("  instruction count or mix differs                      %4d" % table["differs"])
    ok = not (lost or added or twice or moved) and table["identical"] == len(old)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
