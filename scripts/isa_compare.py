#!/usr/bin/env python3
"""Is the device code of two revisions the same, kernel by kernel?

    scripts/isa_compare.py REV_A REV_B [file.hip ...]

A revision is anything `git archive` takes (HEAD~1, a tag, a hash) or `WORKTREE` for the files as they stand.  For each kernel
source (default: the sources of the Makefile's OBJS in REV_B) both revisions' fastgen_amd/csrc and include are put into a temporary
directory and the device side alone is compiled to assembly with that revision's own CXXFLAGS (`--cuda-device-only -S`).  The
assembly is split into functions; comments, `.file` / `.ident` lines and the per-file numbering of local labels are dropped; a
function is "same" when its instruction stream and, for a kernel, its `.amdhsa_*` descriptor block (registers, LDS, scratch) are
equal line by line.  Prints one line per source and one per function that differs or exists on one side only; exits 1 if any does.
Needs no GPU.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "fastgen_amd/csrc"


def checkout(rev, dst):
    """fastgen_amd/csrc and include of `rev` under dst"""
    if rev == "WORKTREE":
        tar = subprocess.Popen(["tar", "-c", "--exclude=*.o", "--exclude=timing", CSRC, "include"], cwd=ROOT, stdout=subprocess.PIPE)
    else:
        tar = subprocess.Popen(["git", "archive", rev, CSRC, "include"], cwd=ROOT, stdout=subprocess.PIPE)
    subprocess.run(["tar", "-x", "-C", dst], stdin=tar.stdout, check=True)
    if tar.wait() != 0:
        sys.exit(f"cannot read revision {rev}")


def make_var(tree, name):
    """the value of a variable of the revision's own Makefile"""
    out = subprocess.run(["make", "-s", "-C", os.path.join(tree, CSRC), "--eval", f"isa-print: ; @echo $({name})", "isa-print"],
                         check=True, capture_output=True, text=True)
    return out.stdout.split()


def compile_asm(tree, src):
    d = os.path.join(tree, CSRC)
    if not os.path.exists(os.path.join(d, src)):
        return None
    out = os.path.join(d, src + ".s")
    hipcc = make_var(tree, "HIPCC")
    r = subprocess.run(hipcc + make_var(tree, "CXXFLAGS") + ["-w", "--cuda-device-only", "-S", src, "-o", out], cwd=d, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{src}: hipcc failed\n{r.stderr}")
    with open(out) as f:
        return f.read()


LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+(_\d+)?")  # .LBB12_3 -> .LBB_3, .Lfunc_end12 -> .Lfunc_end, .Ltmp7 -> .Ltmp


def parse(asm):
    """{function: {"kernel": bool, "code": [lines], "desc": [lines]}}"""
    funcs, cur, desc = {}, None, None
    for raw in asm.splitlines():
        line = raw.split(";", 1)[0].split("//", 1)[0].strip()
        if not line or line.startswith((".file", ".ident")):
            continue
        line = LOCAL_LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), " ".join(line.split()))
        if line.startswith(".amdhsa_kernel "):
            desc = funcs.setdefault(line.split()[1], {"kernel": True, "code": [], "desc": []})
            desc["kernel"] = True
        elif line == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            desc["desc"].append(line)
        elif line.startswith(".type ") and line.endswith(",@function"):
            cur = funcs.setdefault(line.split()[1].split(",")[0], {"kernel": False, "code": [], "desc": []})
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and not line.startswith((".section", ".p2align", ".globl", ".weak", ".protected", ".hidden")):
            cur["code"].append(line)
    return funcs


def field(f, key):
    for line in f["desc"]:
        if line.startswith(".amdhsa_" + key + " "):
            return line.split()[1]
    return "-"


def demangle(names):
    if not names:
        return {}
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev_a")
    ap.add_argument("rev_b")
    ap.add_argument("files", nargs="*", help="kernel sources under fastgen_amd/csrc (default: the Makefile's OBJS)")
    ap.add_argument("--diff", action="store_true", help="print a unified diff of every function that differs")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1), help="parallel compiles")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        trees = []
        for i, rev in enumerate((args.rev_a, args.rev_b)):
            trees.append(os.path.join(tmp, "ab"[i]))
            os.mkdir(trees[-1])
            checkout(rev, trees[-1])
        files = [os.path.basename(f) for f in args.files] or [o[:-2] + ".hip" for o in make_var(trees[1], "OBJS")]
        with concurrent.futures.ThreadPoolExecutor(args.j) as pool:
            asm = {(t, f): pool.submit(compile_asm, t, f) for f in files for t in trees}
            asm = {k: v.result() for k, v in asm.items()}
    bad = 0
    print(f"{'source':<16} {'kernels':>7} {'same':>5} {'differ':>6} {'only ' + args.rev_a:>12} {'only ' + args.rev_b:>12} {'other functions same/differ':>28}")
    for f in files:
        a, b = (parse(asm[(t, f)]) if asm[(t, f)] is not None else None for t in trees)
        if a is None or b is None:
            print(f"{f:<16} exists only in {args.rev_b if a is None else args.rev_a}")
            bad += 1
            continue
        names = demangle(sorted(set(a) | set(b)))
        rows, count = [], {(k, s): 0 for k in (True, False) for s in ("same", "differ", "only_a", "only_b")}
        for n in sorted(names):
            fa, fb = a.get(n), b.get(n)
            kernel = (fa or fb)["kernel"]
            if fa is None or fb is None:
                state = "only_b" if fa is None else "only_a"
                rows.append(f"    {state.replace('_a', ' ' + args.rev_a).replace('_b', ' ' + args.rev_b)}: {names[n]}")
            elif fa["code"] == fb["code"] and fa["desc"] == fb["desc"]:
                state = "same"
            else:
                state = "differ"
                what = [w for w, k in (("instructions", "code"), ("descriptor", "desc")) if fa[k] != fb[k]]
                regs = " ".join(f"{k.split('_')[-1] if 'free' in k else k.split('_')[0]} {field(fa, k)}->{field(fb, k)}" for k in
                                ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size"))
                rows.append(f"    differs ({', '.join(what)}; {len(fa['code'])}->{len(fb['code'])} lines; {regs}): {names[n]}")
                if args.diff:
                    rows += ["        " + l for l in difflib.unified_diff(fa["code"] + fa["desc"], fb["code"] + fb["desc"], args.rev_a, args.rev_b, lineterm="")]
            count[(kernel, state)] += 1
        k = {s: count[(True, s)] for s in ("same", "differ", "only_a", "only_b")}
        o = {s: count[(False, s)] for s in ("same", "differ", "only_a", "only_b")}
        print(f"{f:<16} {sum(k.values()):>7} {k['same']:>5} {k['differ']:>6} {k['only_a']:>12} {k['only_b']:>12} "
              f"{str(o['same']) + '/' + str(o['differ'] + o['only_a'] + o['only_b']):>28}")
        print("\n".join(rows), end="\n" if rows else "")
        bad += sum(k.values()) + sum(o.values()) - k["same"] - o["same"]
    print("every function identical" if not bad else f"{bad} functions differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
