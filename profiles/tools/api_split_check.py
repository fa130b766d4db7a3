#!/usr/bin/env python3
"""Is a cut of the C ABI's host layer into api_internal.h + api_batch.h + api.hip + api_*.hip a pure move?  (DESIGN_OTHER_PATHS.md
section 4h.13)

    python profiles/tools/api_split_check.py PARENT [--asm]

PARENT: the host layer before the cut -- one file where it was api.hip alone (git show REV:ilupp_amd/csrc/api.hip > FILE), else a
directory that holds its files under their own names (git show REV:ilupp_amd/csrc/F > DIR/F for api.hip, every api_*.hip and every
api_*.h of REV: the units of the parent then include the parent's headers, not this tree's).

1. Lines.  The non-blank lines of the parent's files against those of the two headers, api.hip and the api_*.hip files of this tree, as
   multisets.  Every line that stands on one side only is put into a class; a '-' line and a '+' line that differ in nothing but a
   linkage keyword or a default argument are paired and printed side by side.  Lines no class takes are printed under UNCLASSIFIED:
   there must be none.
2. --asm: device code (needs hipcc).  The Makefile's flags plus --cuda-device-only -S -fuse-cuid=none on every translation unit of the parent
   and of the cut; each kernel's instruction stream, its .amdhsa_kernel block and its metadata entry are compared.
"""
import collections
import glob
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "ilupp_amd", "csrc")
UNITS = ["api.hip"] + sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "api_*.hip")))
HEADERS = ["api_internal.h", "api_batch.h"]
FILES = HEADERS + UNITS


def body(path):
    return [l.rstrip() for l in open(path) if l.strip()]


def norm(line):
    """a line without what the allowed edits of moved text touch"""
    s = re.sub(r"\b(static|inline) ", "", line.strip())
    return re.sub(r" = (nullptr|false)(?=[,)])", "", s)


def classify(sign, line, where):
    s = line.strip()
    if s.startswith("#include"):
        return "include"
    if s.startswith("#pragma"):
        return "pragma (visibility, once)"
    if re.fullmatch(r'(namespace( ilupp)? \{|\}  // namespace( ilupp)?|extern "C" \{|\}  // extern "C")', s):
        return 'namespace / extern "C" brace'
    if s.startswith("//"):
        return "file header / header comment"
    if sign == "+" and where in HEADERS and s.split("//")[0].rstrip().endswith(";"):
        return "declaration"
    return None


def parent_files(parent, pattern):
    """the parent's files that match `pattern` (a single file is api.hip)"""
    if os.path.isdir(parent):
        return sorted(glob.glob(os.path.join(parent, pattern)))
    return [parent] if pattern == "api*.hip" else []


def check_lines(parent):
    old = collections.Counter()
    for f in parent_files(parent, "api*.hip") + parent_files(parent, "api*.h"):
        old.update(body(f))
    new = collections.Counter()
    where = {}
    for f in FILES:
        for l in body(os.path.join(CSRC, f)):
            new[l] += 1
            where.setdefault(l, f)
    minus = list((old - new).elements())
    plus = list((new - old).elements())
    print("parent: %d non-blank lines; the cut: %d in %d files; %d lines on the parent's side only, %d on the cut's" %
          (sum(old.values()), sum(new.values()), len(FILES), len(minus), len(plus)))
    # pairs: the same line but for a linkage keyword / a default argument
    by_norm = collections.defaultdict(list)
    for l in minus:
        by_norm[norm(l)].append(l)
    pairs, rest_plus = [], []
    for l in plus:
        if by_norm.get(norm(l)) and classify("+", l, where[l]) is None:
            pairs.append((by_norm[norm(l)].pop(), l))
        else:
            rest_plus.append(l)
    rest_minus = [l for ls in by_norm.values() for l in ls]
    classes = collections.defaultdict(list)
    for sign, ls in (("-", rest_minus), ("+", rest_plus)):
        for l in ls:
            classes[classify(sign, l, where.get(l, "parent")) or "UNCLASSIFIED"].append((sign, l))
    print("\nclass counts ('-' parent only, '+' cut only):")
    print("  %-34s %3d pairs" % ("linkage keyword / default argument", len(pairs)))
    for c in sorted(classes):
        print("  %-34s -%d +%d" % (c, sum(s == "-" for s, _ in classes[c]), sum(s == "+" for s, _ in classes[c])))
    print("\nthe pairs (parent, then the cut):")
    for a, b in pairs:
        print("  - " + a.strip()[:150])
        print("  + " + b.strip()[:150] + "      [" + where[b] + "]")
    for c in ("declaration", "UNCLASSIFIED"):
        if classes.get(c):
            print("\n%s:" % c)
            for s, l in classes[c]:
                print("  %s %s" % (s, l.strip()[:170]))
    return not classes.get("UNCLASSIFIED")


def kernels(asm):
    """{kernel name without decoration: (instructions, .amdhsa_kernel block, metadata entry)}"""
    text = open(asm).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        sym = m.group(1)
        plain = re.sub(r"\.intern\.[0-9a-f]+|\.static\.[0-9a-f]+", "", sym)
        code = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), text, re.S | re.M).group(1)
        code = "\n".join(l.split(";")[0].rstrip() for l in code.split("\n") if l.strip() and not l.strip().startswith(";"))
        code = re.sub(r"\.LBB\d+_", ".LBB_", code)      # (block labels carry the function's number in its file)
        meta = [e for e in re.split(r"(?m)^  (?=- \.agpr_count:)", text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")])
                if re.search(r"\.name:\s+%s\n" % re.escape(sym), e)]
        meta = meta[0].replace(sym, plain) if meta else ""
        out[plain] = (code.replace(sym, plain), m.group(2), meta)
    return out


def check_asm(parent):
    flags = "-O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -Wall -Wno-unused-result --cuda-device-only -S -fuse-cuid=none".split()
    flags += ["-I" + os.path.join(CSRC, "..", "..", "include"), "-I" + CSRC]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        old, new, home = {}, {}, {}
        for i, u in enumerate(parent_files(parent, "api*.hip")):
            subprocess.check_call([hipcc] + flags + ["-x", "hip", u, "-o", os.path.join(d, "parent%d.s" % i)])
            for k, v in kernels(os.path.join(d, "parent%d.s" % i)).items():
                assert k not in old, k
                old[k] = v
        for u in UNITS:
            subprocess.check_call([hipcc] + flags + [os.path.join(CSRC, u), "-o", os.path.join(d, u + ".s")])
            for k, v in kernels(os.path.join(d, u + ".s")).items():
                assert k not in new, k
                new[k] = v
                home[k] = u
    ok = sorted(old) == sorted(new)
    print("\nkernels: parent %d, the cut %d" % (len(old), len(new)))
    for k in sorted(old):
        same = k in new and [old[k][i] == new[k][i] for i in range(3)]
        print("  %-40s %-14s instructions %s, .amdhsa_kernel %s, metadata %s (%d instruction lines)" % (
            k, home.get(k, "MISSING"), *(("same" if s else "DIFFER") for s in (same or [False] * 3)), len(old[k][0].split("\n"))))
        ok = ok and same and all(same)
    return ok


if __name__ == "__main__":
    good = check_lines(sys.argv[1])
    if "--asm" in sys.argv[2:]:
        good = check_asm(sys.argv[1]) and good
    sys.exit(0 if good else 1)
