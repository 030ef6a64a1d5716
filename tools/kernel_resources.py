#!/usr/bin/env python3
"""Registers, spills, scratch and LDS of every kernel of a HIP source, from hipcc's own remarks (no GPU needed):
    python tools/kernel_resources.py inpaintnet_amd/csrc/decode_b1.hip [more.hip ...] [--ref <git rev>]
--ref REV compiles the same files as of that revision next to the working tree and prints only the kernels whose numbers moved.
--ref REV --asm compares the gfx950 assembly of the two instead: a host-only change must leave it identical.  Per file the whole-file
verdict, then per kernel (matched by symbol across ALL the files given, so a kernel may change files): identical | identical, moved
a.hip -> b.hip | DIFFERS | only in REV | only in tree.  A file that exists on one side only counts as an empty kernel set there; the last
line counts the symbols of both sides."""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "inpaintnet_amd", "csrc")


def resources(src, incdir):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", src, "-o", "/dev/null",
           "-Rpass-analysis=kernel-resource-usage", "-I", incdir, "-I", os.path.join(REPO, "include")]
    err = subprocess.run(cmd, capture_output=True, text=True, cwd=incdir).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "").replace("void ", ""))
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def device_asm(src, incdir):
    """The file's device assembly without the lines that carry its content hash (__hip_cuid_*: they move with any edit)."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "--cuda-device-only", "-S", src,
           "-o", "-", "-I", incdir, "-I", os.path.join(REPO, "include")]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=incdir, check=True).stdout
    return [l for l in out.splitlines() if "__hip_cuid_" not in l]


def functions(lines):
    """{symbol: its lines from `.globl SYM` / `.protected SYM` to `.Lfunc_endN:`} without the function's index in its file (block labels, func_begin / end) and the file's count of long branches (post_getpc)"""
    out, sym = {}, None
    for l in lines:
        m = re.match(r"\s*\.(globl|protected)\s+(\S+).*-- Begin function", l)      # (.protected leads where the kernel has external linkage)
        if m:
            sym = m.group(2)
            out[sym] = []
        if sym is not None:
            l = re.sub(r"\.L(func_begin|func_end|post_getpc)\d+", r".L\1", re.sub(r"BB\d+_", "BB_", l))
            out[sym].append(re.sub(r"\s+", " ", l))            # (the comment column behind a label moves with the index's width)
            if l.startswith(".Lfunc_end:"):
                sym = None
    return out


def pretty(sym):
    name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "").replace("void ", ""))


def compare_asm(srcs, ref):
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call(f"git -C {REPO} archive {ref} inpaintnet_amd/csrc include | tar -x -C {tmp}", shell=True)
        old_dir = os.path.join(tmp, "inpaintnet_amd", "csrc")
        # a file that exists on one side only (a kernel's new or former home) is an empty kernel set on the other
        old = {os.path.basename(src): device_asm(os.path.join(old_dir, os.path.basename(src)), old_dir)
               if os.path.exists(os.path.join(old_dir, os.path.basename(src))) else [] for src in srcs}
    new = {os.path.basename(src): device_asm(src, CSRC) if os.path.exists(src) else [] for src in srcs}
    where = [{}, {}]                                            # symbol -> (file, lines), in REV and in the tree
    for side, files in zip(where, (old, new)):
        for f, lines in files.items():
            side.update({sym: (f, body) for sym, body in functions(lines).items()})
    for f in new:
        o, n = old[f], new[f]
        first = next((i + 1 for i, (a, b) in enumerate(zip(o, n)) if a != b), None if len(o) == len(n) else min(len(o), len(n)) + 1)
        print(f"{f}: device code " + (f"only in the tree ({len(n)} lines)" if not o else f"only in {ref} ({len(o)} lines)" if not n else
                                      f"identical to {ref} ({len(n)} lines)" if first is None else
                                      f"DIFFERS from {ref} (first at line {first}; {len(o)} -> {len(n)} lines)"))
        for sym in sorted(s for side in where for s, (g, _) in side.items() if g == f and (side is where[1] or s not in where[1])):
            (fo, bo), (fn, bn) = where[0].get(sym, (None, None)), where[1].get(sym, (None, None))
            verdict = ("only in tree" if fo is None else f"only in {ref}" if fn is None else "DIFFERS" if bo != bn else
                       "identical" if fo == fn else f"identical, moved {fo} -> {fn}")
            print(f"    {pretty(sym)}: {verdict}")
    print(f"{len(where[0])} kernels in {ref}, {len(where[1])} in the tree")


def fmt(r):
    return " ".join(f"{k}={v}" for k, v in r.items())


def main():
    args = sys.argv[1:]
    ref = None
    if "--ref" in args:
        i = args.index("--ref")
        ref = args[i + 1]
        del args[i:i + 2]
    asm = "--asm" in args
    if asm:
        args.remove("--asm")
        if ref is None:
            sys.exit("--asm compares with a revision: give --ref REV")
    if asm:
        return compare_asm([os.path.abspath(src) for src in args], ref)
    for src in args:
        src = os.path.abspath(src)
        new = resources(src, CSRC)
        if ref is None:
            for k, v in new.items():
                print(f"{os.path.basename(src)}: {k}: {fmt(v)}")
            continue
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call(f"git -C {REPO} archive {ref} inpaintnet_amd/csrc include | tar -x -C {tmp}", shell=True)
            old = resources(os.path.join(tmp, "inpaintnet_amd", "csrc", os.path.basename(src)), os.path.join(tmp, "inpaintnet_amd", "csrc"))
        for k in sorted(set(new) | set(old)):
            if new.get(k) != old.get(k):
                print(f"{os.path.basename(src)}: {k}\n    {ref}: {fmt(old.get(k, {}))}\n    tree: {fmt(new.get(k, {}))}")
        print(f"{os.path.basename(src)}: {len(new)} kernels, the rest unchanged")


if __name__ == "__main__":
    main()
