#!/usr/bin/env python3
"""Where a kernel's machine code comes from: instructions and code bytes per source file and line range.  No GPU.

    python tools/kernel_code_map.py vp_k_pitch_ws [vp_k_pitch_ws_l ...] [--tu K] [--lines 50] [--top 0]

The unit (csrc/vp_kernels.hip with the build's own flags, -DVP_TU=K to keep one group of kernels: 6 for vp_k_pitch_ws, 10 for
vp_k_pitch_ws_l; 0, the default, compiles all of them) is compiled for gfx950 with `-gline-tables-only -S --offload-device-only` into a
temporary directory; every instruction between the kernel's label and its end is attributed to the `.loc` record in force, i.e. to
the innermost inlined source line.  Instructions are counted exactly; the assembly listing carries no encodings, so bytes are the
kernel's `codeLenInByte` shared out by instruction count (the mean is ~5.7 bytes per instruction) -- good to a few per cent per row.
Line tables move the schedule a little: totals differ from the product build's by well under one per cent."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compile_listing(tu, tmp):
    from vocoderproject_amd import build
    out = os.path.join(tmp, "k.s")
    cmd = build.compile_command() + [f"-DVP_TU={tu}", "-gline-tables-only", "-S", "--offload-device-only", "-Wno-unused-command-line-argument",
                                     os.path.join(build.CSRC, "vp_kernels.hip"), "-o", out]
    subprocess.run(cmd, check=True)
    with open(out) as f:
        return f.read()


def code_map(listing, kernel, lines=50):
    """-> (code bytes, instructions, {(file, first line of the range): instructions}) of `kernel` in an assembly listing."""
    files = {}
    for m in re.finditer(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', listing, re.M):
        files[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
    label = re.search(r"^(_Z%d%s\w*):" % (len(kernel), re.escape(kernel)), listing, re.M)
    if not label:
        raise SystemExit(f"{kernel}: no such kernel in the listing")
    body = listing[label.end():]
    end = re.search(r"^\.Lfunc_end\d+:", body, re.M)
    tail = body[end.end():end.end() + 20000]
    body = body[:end.start()]
    size = re.search(r"; codeLenInByte = (\d+)", tail)
    counts, cur, n = {}, ("?", 0), 0
    for ln in body.split("\n"):
        s = ln.strip()
        if not s or s.startswith(";") or s.endswith(":"):
            continue
        if s.startswith("."):
            m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
            if m:
                line = int(m.group(2))
                cur = (files.get(int(m.group(1)), "?"), (max(line, 1) - 1) // lines * lines + 1)
            continue
        counts[cur] = counts.get(cur, 0) + 1
        n += 1
    return (int(size.group(1)) if size else 0), n, counts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("kernels", nargs="+")
    ap.add_argument("--tu", type=int, default=0)
    ap.add_argument("--lines", type=int, default=50, help="lines per range")
    ap.add_argument("--top", type=int, default=0, help="only the N largest rows per kernel (0: all, in file order)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="vp_map_") as tmp:
        listing = compile_listing(a.tu, tmp)
    for k in a.kernels:
        size, n, counts = code_map(listing, k, a.lines)
        per = size / n if n else 0.0
        print(f"{k}: {size} code bytes, {n} instructions ({per:.2f} bytes per instruction)")
        print("  %-26s %-13s %12s %10s %6s" % ("file", "lines", "instructions", "~bytes", "%"))
        rows = sorted(counts.items(), key=(lambda kv: -kv[1]) if a.top else (lambda kv: kv[0]))
        for (f, l0), c in rows[:a.top or None]:
            print("  %-26s %-13s %12d %10d %6.1f" % (f, f"{l0}-{l0 + a.lines - 1}", c, round(c * per), 100.0 * c / n))
        byfile = {}
        for (f, _), c in counts.items():
            byfile[f] = byfile.get(f, 0) + c
        for f, c in sorted(byfile.items(), key=lambda kv: -kv[1]):
            print("  %-26s %-13s %12d %10d %6.1f" % (f, "all", c, round(c * per), 100.0 * c / n))
        print()


if __name__ == "__main__":
    main()
