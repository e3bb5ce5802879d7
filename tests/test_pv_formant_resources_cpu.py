"""CPU-side check of the two formant kernels' budgets, from the built library (no GPU, no compiler run): each exists, uses no scratch,
spills no vector register and fits the 512 registers a lane has at one wavefront per SIMD (tools/kernel_resources.py reads the code
object's metadata); they have no static LDS and their dynamic LDS is their curve parents' (the envelope lives in the wavefront's exchange
buffer: the launchers pass the parents' sizes, checked here against the ceiling at every hop); the four kernels they descend from are
still there under their names; and both keep the VP_POISON_LDS prologue."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# formant build -> the curve build it is a copy of -> that build's parent
KERNELS = {"vp_k_stft_pv_formant": ("vp_k_stft_pv_curve", "vp_k_stft_fused<true, false>"), "vp_k_pv_stream_formant": ("vp_k_pv_stream_curve", "vp_k_pv_stream")}
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
def test_each_formant_kernel_is_built_without_scratch_within_512_registers(resources, kernel):
    assert kernel in resources, sorted(k for k in resources if "stft" in k or "pv_" in k)
    r = resources[kernel]
    print(f"PV FORMANT resources {kernel} {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    # (on this target the metadata's vgpr_count already contains the AGPRs, so the sum asks more than the hardware does)
    assert r["vgpr"] + r["agpr"] <= 512, r
    assert r["lds"] == 0, r                                    # no static LDS: everything is the dynamic carve of the parent
    for parent in KERNELS[kernel]:
        assert parent in resources and resources[parent]["scratch"] == 0, (parent, resources.get(parent))


def test_the_parents_keep_their_names_and_the_copies_their_poison_prologue():
    src = open(os.path.join(CSRC, "vp_stft.hip")).read()
    assert re.search(r"template <bool PV, bool MAG>\s*__global__ __launch_bounds__\(64 \* NWV\) void vp_k_stft_fused\(VpStftArgs A\)", src)
    assert "void vp_k_pv_stream(VpPvArgs A)" in src
    assert src.rstrip().endswith('#include "vp_stft_formant.inc"')
    curve = open(os.path.join(CSRC, "vp_stft_curve.inc")).read()
    assert "void vp_k_stft_pv_curve(VpStftArgs A, const double *ratioTab)" in curve and "void vp_k_pv_stream_curve(VpPvArgs A, const double *ratioTab)" in curve
    inc = open(os.path.join(CSRC, "vp_stft_formant.inc")).read()
    for k in KERNELS:
        assert f"void {k}(" in inc, k
    assert inc.count("#ifdef VP_POISON_LDS") == 2
    assert inc.count("formant:") >= 10                        # what differs from the parents is marked
    from vocoderproject_amd import build
    assert "vp_stft_formant.inc" in build.DEPS


def test_dynamic_lds_is_the_parents_and_fits_the_ceiling():
    from vocoderproject_amd import build
    lib = C.CDLL(build.build())
    base = getattr(lib, "_Z17vp_stft_lds_bytesiii")            # size_t vp_stft_lds_bytes(int F, int hop, int f32)
    base.restype, base.argtypes = C.c_size_t, [C.c_int, C.c_int, C.c_int]
    stream = getattr(lib, "_Z15vp_pv_lds_bytesv")
    stream.restype = C.c_size_t
    # the stage's arrays (PvLds), from the library: the streaming carve is four 8 KB exchange buffers, the ring (VP_PV_RING = 4096 floats)
    # and the history (1024 floats) in front of them (pv_stream_lds_bytes, csrc/vp_stft.hip)
    pv_arrays = stream() - (4 * 8192 + (4096 + 1024) * 4)
    assert pv_arrays > 0 and pv_arrays % (513 * 8) == 0, pv_arrays
    sizes = {hop: base(1024, hop, 0) + pv_arrays for hop in (64, 128, 256, 512)}
    sizes["stream"] = stream()
    print(f"PV FORMANT dynamic LDS {sizes}")
    for k, b in sizes.items():
        assert 4 * 8192 < b <= LDS_CEILING, (k, b)
    # the launchers of csrc/vp_stft_formant.inc pass exactly the parents' expressions and request the same ceiling
    inc = open(os.path.join(CSRC, "vp_stft_formant.inc")).read()
    assert "vp_k_stft_pv_formant, grid, block, lds + pv_lds_bytes()" in inc
    assert "vp_k_pv_stream_formant, dim3(a.S), dim3(64 * NWV), vp_pv_lds_bytes()" in inc
    assert inc.count("hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512") == 2
