"""CPU-side check of the two time-stretch kernels' budgets, from the built library (no GPU, no compiler run): each exists, uses no scratch,
spills no vector register and fits the 512 registers a lane has at one wavefront per SIMD (tools/kernel_resources.py reads the code
object's metadata); their dynamic LDS is their parent build's (the positions need none of their own: the launcher passes the parents'
sizes, checked here against the ceiling); and the kernels they were copied from are still there under their names, with no scratch."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# stretch build -> the build it is a copy of
KERNELS = {"vp_k_stft_pv_stretch": "vp_k_stft_fused<true, false>", "vp_k_stft_pv2k_stretch": "vp_k_stft_pv2k"}
LDS_CEILING = 160 * 1024 - 512
CSRC = os.path.join(ROOT, "vocoderproject_amd", "csrc")


@pytest.fixture(scope="module")
def resources():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    return kernel_resources.kernel_resources(build.build())


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_each_stretch_kernel_is_built_without_scratch_within_512_registers(resources, kernel):
    assert kernel in resources, sorted(k for k in resources if "stft" in k)
    r = resources[kernel]
    print(f"PV STRETCH resources {kernel} {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    # (on this target the metadata's vgpr_count already contains the AGPRs, so the sum asks more than the hardware does)
    assert r["vgpr"] + r["agpr"] <= 512, r
    assert r["lds"] == 0, r                                    # no static LDS: everything is the dynamic carve of the parent
    parent = resources[KERNELS[kernel]]
    print(f"PV STRETCH resources {KERNELS[kernel]} {parent}")
    assert parent["scratch"] == 0, (KERNELS[kernel], parent)


def test_the_parents_keep_their_names_and_the_copies_their_poison_prologue():
    src = open(os.path.join(CSRC, "vp_stft.hip")).read()
    assert re.search(r"template <bool PV, bool MAG>\s*__global__ __launch_bounds__\(64 \* NWV\) void vp_k_stft_fused\(VpStftArgs A\)", src)
    assert "void vp_k_stft_pv2k(VpStftArgs A)" in src and '#include "vp_stft_stretch.inc"' in src
    inc = open(os.path.join(CSRC, "vp_stft_stretch.inc")).read()
    for k in KERNELS:
        assert f"void {k}(" in inc, k
    assert inc.count("#ifdef VP_POISON_LDS") == 2
    curve = open(os.path.join(CSRC, "vp_stft_curve.inc")).read()
    assert "stretch" not in curve                              # a file of their own


def test_dynamic_lds_is_the_parents_and_fits_the_ceiling():
    from vocoderproject_amd import build
    lib = C.CDLL(build.build())
    base = getattr(lib, "_Z17vp_stft_lds_bytesiii")            # size_t vp_stft_lds_bytes(int F, int hop, int f32)
    base.restype, base.argtypes = C.c_size_t, [C.c_int, C.c_int, C.c_int]
    pv2k = getattr(lib, "_Z22vp_stft_pv2k_lds_bytesi")
    pv2k.restype, pv2k.argtypes = C.c_size_t, [C.c_int]
    pv_arrays = (4 * 2 + 5 + 4 + 1) * 513 * 8                  # ana, phPrev, inc, sum of the 1024-point stage (PvLds)
    sizes = {(1024, hop): base(1024, hop, 0) + pv_arrays for hop in (64, 128, 256, 512)}
    sizes.update({(2048, hop): pv2k(hop) for hop in (128, 256, 512, 1024)})
    print(f"PV STRETCH dynamic LDS {sizes}")
    for k, b in sizes.items():
        assert 4 * 8192 < b <= LDS_CEILING, (k, b)
    # the launcher of csrc/vp_stft_stretch.inc passes exactly the parents' expressions
    inc = open(os.path.join(CSRC, "vp_stft_stretch.inc")).read()
    assert "vp_k_stft_pv2k_stretch, grid, block, lds + pv2k_lds_bytes()" in inc
    assert "vp_k_stft_pv_stretch, grid, block, lds + pv_lds_bytes()" in inc
