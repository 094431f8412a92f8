#!/usr/bin/env python3
"""Compare the device ISA of HIP sources kernel by kernel (the gate of a refactor that must not change code generation).

    python3 tools/isa_diff.py OLD NEW                      # two .s listings, or two .hip files (compiled here)
    python3 tools/isa_diff.py OLD -- NEW1 NEW2 ...         # several files a side (a unit that was split): the union of their functions
    python3 tools/isa_diff.py --rev HEAD --into a.hip,b.hip nanocaller_amd/csrc/nc_pipe.hip      # FILE at REV against the units it was split into
    python3 tools/isa_diff.py old/nc_indel.hip old/nc_msa.hip -- nc_indel.hip nc_indel_tiles.hip nc_indel_accum.hip nc_msa.hip   # code that moved between units too
    python3 tools/isa_diff.py --rev HEAD nanocaller_amd/csrc/nc_cnn_h3.hip ...   # each file at REV against the working tree
    python3 tools/isa_diff.py --ignore-kernarg-size --rev HEAD FILE              # ... an appended, unread kernel argument does not count

A .hip file is compiled with `hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only`; with --rev the sources of REV
(nanocaller_amd/csrc and include, from `git archive`) are compiled in a temporary directory.  Each listing is split into
per-function bodies (from `<mangled name>:` to `.Lfunc_end`, the kernel descriptor included, plus the `.set <name>.*` resource
lines); label numbers (.LBB<n>_<m>, .Ltmp<n>, .Lfunc_end<n>) are normalised and comments (`;` to the end of the line) dropped.
Prints the functions that exist on one side only (a new name whose code equals a removed function's, the name substituted, counts
as renamed) and every function whose body or resources differ; exits 1 if any function was added or changed.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only"]
RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def compile_listing(src, out_dir):
    out = os.path.join(out_dir, os.path.basename(src) + ".s")
    src = os.path.abspath(src)
    subprocess.run([HIPCC, *FLAGS, "-Wno-pass-failed", src, "-o", out], check=True, cwd=os.path.dirname(src))
    return out


def functions(path):
    """{mangled name: normalised body lines}"""
    lines = open(path).read().splitlines()
    out, name, body = {}, None, []
    for ln in lines:
        code = ln.split(";", 1)[0].rstrip()
        if name is None:
            m = re.match(r"^([A-Za-z_.$][\w.$]*):$", code)
            if m and not code.startswith(".L"):
                name, body = m.group(1), []
            elif code.startswith("\t.set ") or code.startswith(".set "):
                m = re.match(r"\s*\.set\s+([\w.$]+)\.(\w+),", code)
                if m and m.group(1) in out:
                    out[m.group(1)].append(code.strip())
            continue
        if re.match(r"^\.Lfunc_end\d+:", code):
            out[name] = normalise(body)
            name = None
            continue
        if code.strip():
            body.append(code.strip())
    return out


def normalise(body):
    tmp = {}

    def ltmp(m):
        return ".Ltmp_%d" % tmp.setdefault(m.group(0), len(tmp))

    res = []
    for ln in body:
        ln = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", ln)
        ln = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", ln)
        ln = re.sub(r"\.Ltmp\d+", ltmp, ln)
        res.append(ln)
    return res


def resources(body):
    r = {}
    for ln in body:
        m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", ln)
        if m and m.group(1) in RESOURCES:
            r[m.group(1)] = m.group(2)
        m = re.match(r"\.set\s+[\w.$]+\.(num_vgpr|num_agpr|numbered_sgpr|private_seg_size),\s*(\S+)", ln)
        if m:
            r[m.group(1)] = m.group(2)
    return r


def union(paths):
    out = {}
    for p in paths:
        out.update(functions(p))
    return out


IGNORE_KERNARG = False


def compare(old_s, new_s, label):
    """old_s / new_s: a listing or a list of listings"""
    a, b = union([old_s] if isinstance(old_s, str) else old_s), union([new_s] if isinstance(new_s, str) else new_s)
    if IGNORE_KERNARG:                                                   # (an argument appended that the kernel never loads: the instructions decide)
        a, b = ({n: [ln for ln in body if not ln.startswith(".amdhsa_kernarg_size")] for n, body in d.items()} for d in (a, b))
    bad = renamed = 0
    gone, new = set(a) - set(b), set(b) - set(a)
    for n in sorted(new):
        # a function whose mangled name changed (a template parameter dropped, say) but whose code did not
        twin = next((m for m in sorted(gone) if [ln.replace(m, n) for ln in a[m]] == b[n]), None)
        if twin:
            print(f"{label}: renamed  {twin} -> {n}, identical")
            gone.discard(twin)
            renamed += 1
        else:
            print(f"{label}: added    {n}")
            bad += 1
    for n in sorted(gone):
        print(f"{label}: removed  {n}")
    same = 0
    for n in sorted(set(a) & set(b)):
        if a[n] == b[n]:
            same += 1
            continue
        bad += 1
        ra, rb = resources(a[n]), resources(b[n])
        diff = {k: (ra.get(k), rb.get(k)) for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)}
        print(f"{label}: CHANGED  {n}  ({len(a[n])} -> {len(b[n])} lines){'  ' + str(diff) if diff else ''}")
    print(f"{label}: {same} identical, {renamed} renamed, {len(gone)} removed, {bad} added or changed")
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rev", help="compare each FILE at this git revision against the working tree")
    ap.add_argument("--into", help="with --rev: comma-separated working-tree files that replace FILE (default: FILE itself)")
    ap.add_argument("--ignore-kernarg-size", action="store_true", help="leave the .amdhsa_kernarg_size line out of the comparison")
    ap.add_argument("files", nargs="+")
    args = ap.parse_args()
    global IGNORE_KERNARG
    IGNORE_KERNARG = args.ignore_kernarg_size
    bad = 0
    with tempfile.TemporaryDirectory() as td:
        if args.rev:
            root = subprocess.run(["git", "rev-parse", "--show-toplevel"], check=True, capture_output=True, text=True).stdout.strip()
            old_tree = os.path.join(td, "old")
            os.makedirs(old_tree)
            arc = subprocess.run(["git", "-C", root, "archive", args.rev, "nanocaller_amd/csrc", "include"], check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", old_tree], input=arc, check=True)
            for f in args.files:
                rel = os.path.relpath(os.path.abspath(f), root)
                od, nd = os.path.join(td, "a"), os.path.join(td, "b")
                os.makedirs(od, exist_ok=True)
                os.makedirs(nd, exist_ok=True)
                new = args.into.split(",") if args.into else [f]
                bad += compare(compile_listing(os.path.join(old_tree, rel), od), [compile_listing(n, nd) for n in new], os.path.basename(f))
        else:
            if "--" in sys.argv:                                         # (argparse drops the separator: find the split in the raw arguments)
                cut = sys.argv[sys.argv.index("--") + 1:]
                old, new = args.files[:len(args.files) - len(cut)], cut
            elif len(args.files) == 2:
                old, new = args.files[:1], args.files[1:]
            else:
                ap.error("without --rev give OLD NEW, or OLD... -- NEW...")
            if not old or not new:
                ap.error("a side is empty")
            for sub in ("a", "b"):
                os.makedirs(os.path.join(td, sub))
            old = [compile_listing(f, os.path.join(td, "a")) if f.endswith(".hip") else f for f in old]
            new = [compile_listing(f, os.path.join(td, "b")) if f.endswith(".hip") else f for f in new]
            bad += compare(old, new, os.path.basename(args.files[-1]))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
