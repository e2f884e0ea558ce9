#!/usr/bin/env python3
"""Device code of two source trees, compared per kernel symbol (needs hipcc, no GPU).

    python tools/isa_diff.py PARENT_TREE TREE [--pair=OLD=NEW ...] [FILE.hip ...] > profiles/<change>/isa_parent_vs_tree.txt

Every csrc/*.hip of both trees (or only the files named) is compiled with the product flags plus `--offload-device-only -S`.  A kernel's text is
its body (label to .Lfunc_end) and its .amdhsa_kernel block (registers, LDS, scratch), with comment lines and
.file / .ident dropped and local label numbers normalised, so a kernel that only moved to another file or position
compares equal.  One line per kernel: identical, or the number of differing lines.

A kernel that changed its symbol on purpose (a merged template, a new template argument) is paired explicitly: --pair=OLD=NEW
rewrites the parent's symbols with re.sub(OLD, NEW) -- in its kernels' text as well -- before the comparison; the pairs are
listed at the head of the output.
"""
import concurrent.futures as cf
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ms_gat_amd.build import ARCH, _hipcc  # noqa: E402


def _asm(tree, src, out):
    csrc = os.path.join(tree, "ms_gat_amd", "csrc")
    flags = ["-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", f"--offload-arch={ARCH}",
             "-I" + os.path.join(tree, "include"), "-I" + csrc]
    subprocess.run([_hipcc(), *flags, "--offload-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    return out


def _norm(line):
    line = re.sub(r"\s*;.*$", "", line.rstrip())
    line = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)
    return line


def kernels(tree, tmp, only):
    """{symbol: (file, [normalised lines])} over every csrc/*.hip of the tree"""
    srcs = sorted(glob.glob(os.path.join(tree, "ms_gat_amd", "csrc", "*.hip")))
    srcs = [s for s in srcs if not only or os.path.basename(s) in only]
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        outs = list(ex.map(lambda s: _asm(tree, s, os.path.join(tmp, os.path.basename(s) + ".s")), srcs))
    found = {}
    for src, out in zip(srcs, outs):
        text = open(out).read().splitlines()
        names = [m.group(1) for ln in text if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
        for name in names:
            body, on = [], False
            for ln in text:
                s = ln.strip()
                if _norm(ln) == name + ":" or s.startswith(".amdhsa_kernel " + name):
                    on = True
                if on and s and not s.startswith((";", ".file", ".ident")) and _norm(ln):
                    body.append(_norm(ln))
                if on and (s.startswith(".Lfunc_end") or s.startswith(".end_amdhsa_kernel")):
                    on = False
            found[name] = (os.path.basename(src), body)
    return found


def renamed(found, pairs):
    """the parent's kernels under the symbols the tree gives them"""
    out = {}
    for name, (src, body) in found.items():
        new = name
        for old, repl in pairs:
            new = re.sub(old, repl, new)
        if new != name:
            body = [ln.replace(name, new) for ln in body]
        out[new] = (src, body)
    return out


def main():
    parent, tree = sys.argv[1], sys.argv[2]
    pairs = [tuple(a[len("--pair="):].split("=", 1)) for a in sys.argv[3:] if a.startswith("--pair=")]
    only = [a for a in sys.argv[3:] if not a.startswith("--pair=")]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = renamed(kernels(parent, ta, only), pairs), kernels(tree, tb, only)
    for old, repl in pairs:
        print(f"# parent symbols paired with the tree's: {old} -> {repl}")
    differing = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: only in the {'tree' if name in b else 'parent'}")
            differing += 1
            continue
        where = b[name][0] if a[name][0] == b[name][0] else f"{a[name][0]} -> {b[name][0]}"
        n = 0 if a[name][1] == b[name][1] else sum(
            1 for d in difflib.unified_diff(a[name][1], b[name][1], n=0, lineterm="") if d[0] in "+-" and d[:3] not in ("+++", "---"))
        differing += n > 0
        print(f"{where} {name}: {'identical' if n == 0 else f'{n} lines differ'} ({len(b[name][1])} lines)")
    print(f"# {len(set(a) | set(b))} kernels, {differing} not identical")


if __name__ == "__main__":
    main()
