"""CPU-side checks of the lean pitch-kernel build (vp_k_pitch_ws_l): its resources in the built library's code objects, and the
one predicate the host and the generic kernels share (vp_common.h vp_ws_vec_ok) against a restatement, swept by a stand-alone
host program."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_lean_build_has_no_scratch_fits_the_registers_and_is_no_larger_than_the_generic_build():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    lib = build.build()
    res = kernel_resources.kernel_resources(lib)
    assert "vp_k_pitch_ws_l" in res and "vp_k_pitch_ws" in res, sorted(res)[:8]
    r = res["vp_k_pitch_ws_l"]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["vgpr"] <= 168, r
    # the dynamic LDS starts behind the static part; the kernel reads and writes it sixteen bytes at a time (the FFT's complex doubles)
    assert r["lds"] % 16 == 0, r
    size = kernel_resources.kernel_code_bytes(lib)
    assert 0 < size["vp_k_pitch_ws_l"] <= size["vp_k_pitch_ws"], (size["vp_k_pitch_ws_l"], size["vp_k_pitch_ws"])


SWEEP = r"""
#include "vp_common.h"
#include <cstdio>
#include <cstring>
int main()
{
    // N, inCounter, outCounter, currCounter, nSteps, latency, nt, the two pointers' offsets in bytes: one line per case
    const int Ns[] = {256, 512, 1024, 1000, 258, 1280, 2048};
    const int offs[] = {0, 4, 16};
    const int nts[] = {768, 512};
    const int lats[] = {1024, 1026, 2048};
    long n = 0;
    for (int N : Ns) for (int lat : lats) for (int nt : nts) for (int nSteps = 1; nSteps <= 5; nSteps++)
        for (int ic = 0; ic < 6; ic++) for (int oc = 0; oc < 4; oc++) for (int cc = 0; cc < 6; cc++) for (int ox : offs) for (int ov : offs) {
            VpGeom g;
            memset(&g, 0, sizeof g);
            g.N = N; g.F = 1024; g.C = 256; g.toKeep = 1024; g.latency = lat; g.inSize = g.toKeep + N + lat; g.outSize = N + lat;
            VpCall c;
            memset(&c, 0, sizeof c);
            // counters: multiples of N as the host advances them, and a few that are not multiples of four / two
            c.inCounter = (ic < 3 ? ic * N : ic - 2) % g.inSize; c.outCounter = (oc < 2 ? oc * N : oc - 1) % g.outSize;
            c.currCounter = (cc < 3 ? cc * N : cc - 2) % g.inSize; c.nSteps = nSteps; c.pStart = 0;
            const size_t base = 4096;
            printf("%d %d %d %d %d %d %d %d %d %d\n", N, lat, nt, nSteps, c.inCounter, c.outCounter, c.currCounter, ox, ov,
                   (int)vp_ws_vec_ok(g, c, nt, vp_ws_p0(g, c), base + ox, base + ov));
            n++;
        }
    fprintf(stderr, "%ld cases\n", n);
    return 0;
}
"""


def _vec_ok(N, lat, nt, nSteps, inC, outC, curC, ox, ov, F=1024, C=256):
    """The prologue's four-samples-per-lane condition, restated: every quantity it cuts into groups of four floats (two doubles) is a
    multiple of four (two), one trip covers the ring, the voice window and the accumulator slice, both rows are 16-byte aligned."""
    toKeep = F
    inSize, outSize = toKeep + N + lat, N + lat
    idx0 = 0 - toKeep
    span = toKeep + F + (nSteps - 1) * C
    p0 = (curC + idx0 + inSize) % inSize
    fours = [N, inSize, inC, p0, idx0 - lat, span]
    twos = [outC, outSize, N + C]
    return (all(v % 4 == 0 for v in fours) and all(v % 2 == 0 for v in twos) and inSize <= 4 * nt and span <= 4 * nt
            and N + C <= 2 * nt and (4096 + ox) % 16 == 0 and (4096 + ov) % 16 == 0)


def test_shared_vec_predicate_against_its_restatement(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "sweep.cpp"
    src.write_text(SWEEP)
    exe = tmp_path / "sweep"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vocoderproject_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    assert len(rows) > 100000
    seen = set()
    for r in rows:
        want = _vec_ok(*r[:9])
        assert bool(r[9]) == want, r
        seen.add(want)
    assert seen == {True, False}
