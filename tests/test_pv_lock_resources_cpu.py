"""CPU-side check of the two peak-locked kernels' budgets, from the built library (no GPU, no compiler run): each exists, uses no scratch,
spills no vector register and fits the 512 registers a lane has at one wavefront per SIMD (tools/kernel_resources.py reads the code
object's metadata); they have no static LDS; their dynamic LDS -- the curve parents' carve plus the locked stage's masks, owners and map
-- stays under the ceiling at every hop and for the stream; the kernels they descend from are still there under their names with the
figures profiles/pv_curve_resources.txt records for them; and both keep the VP_POISON_LDS prologue."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# locked build -> the curve build it is a copy of -> that build's parent
KERNELS = {"vp_k_stft_pv_lock": ("vp_k_stft_pv_curve", "vp_k_stft_fused<true, false>"), "vp_k_pv_stream_lock": ("vp_k_pv_stream_curve", "vp_k_pv_stream")}
# registers of the parents as the existing resource tests print them on the parent commit (vgpr, agpr)
PARENT_FIGURES = {"vp_k_stft_pv_curve": (346, 90), "vp_k_pv_stream_curve": (334, 78), "vp_k_stft_fused<true, false>": (341, 85), "vp_k_pv_stream": (337, 81)}
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
def test_each_locked_kernel_is_built_without_scratch_within_512_registers(resources, kernel):
    assert kernel in resources, sorted(k for k in resources if "stft" in k or "pv_" in k)
    r = resources[kernel]
    print(f"PV LOCK resources {kernel} {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    # (on this target the metadata's vgpr_count already contains the AGPRs, so the sum asks more than the hardware does)
    assert r["vgpr"] + r["agpr"] <= 512, r
    assert r["lds"] == 0, r                                    # no static LDS: everything is the dynamic carve
    for parent in KERNELS[kernel]:
        assert parent in resources and resources[parent]["scratch"] == 0, (parent, resources.get(parent))
        print(f"PV LOCK resources parent {parent} {resources[parent]}")
        assert (resources[parent]["vgpr"], resources[parent]["agpr"]) == PARENT_FIGURES[parent], (parent, resources[parent])


def test_the_parents_keep_their_names_and_the_copies_their_poison_prologue():
    src = open(os.path.join(CSRC, "vp_stft.hip")).read()
    assert re.search(r"template <bool PV, bool MAG>\s*__global__ __launch_bounds__\(64 \* NWV\) void vp_k_stft_fused\(VpStftArgs A\)", src)
    assert "void vp_k_pv_stream(VpPvArgs A)" in src
    assert src.index('#include "vp_stft_curve.inc"') < src.index('#include "vp_stft_lock.inc"') < src.index('#include "vp_stft_formant.inc"')
    curve = open(os.path.join(CSRC, "vp_stft_curve.inc")).read()
    assert "void vp_k_stft_pv_curve(VpStftArgs A, const double *ratioTab)" in curve and "void vp_k_pv_stream_curve(VpPvArgs A, const double *ratioTab)" in curve
    inc = open(os.path.join(CSRC, "vp_stft_lock.inc")).read()
    for k in KERNELS:
        assert f"void {k}(" in inc, k
    assert inc.count("#ifdef VP_POISON_LDS") == 2
    assert inc.count("lock:") >= 10                           # what differs from the parents is marked
    assert "atomic" not in inc.lower()                        # the stage is a gather: no scatter, no LDS atomics
    from vocoderproject_amd import build
    assert "vp_stft_lock.inc" in build.DEPS


def test_dynamic_lds_fits_the_ceiling_at_every_hop():
    from vocoderproject_amd import build
    lib = C.CDLL(build.build())
    base = getattr(lib, "_Z17vp_stft_lds_bytesiii")            # size_t vp_stft_lds_bytes(int F, int hop, int f32)
    base.restype, base.argtypes = C.c_size_t, [C.c_int, C.c_int, C.c_int]
    stream = getattr(lib, "_Z15vp_pv_lds_bytesv")
    stream.restype = C.c_size_t
    one = getattr(lib, "_Z22vp_stft_lock_lds_bytesi")          # size_t vp_stft_lock_lds_bytes(int hop)
    one.restype, one.argtypes = C.c_size_t, [C.c_int]
    lstream = getattr(lib, "_Z20vp_pv_lock_lds_bytesv")        # size_t vp_pv_lock_lds_bytes()
    lstream.restype = C.c_size_t
    pv_arrays = stream() - (4 * 8192 + (4096 + 1024) * 4)      # the parents' stage arrays (PvLds)
    extra = lstream() - stream()                               # what the locked stage adds: per wavefront two masks of 10 words, two maps of 520 ints
    assert extra == 4 * (2 * 10 * 8 + 2 * 520 * 4), extra
    sizes = {hop: one(hop) for hop in (64, 128, 256, 512)}
    for hop, b in sizes.items():
        assert b == base(1024, hop, 0) + pv_arrays + extra, (hop, b)
    sizes["stream"] = lstream()
    print(f"PV LOCK dynamic LDS {sizes}")
    for k, b in sizes.items():
        assert 4 * 8192 < b <= LDS_CEILING, (k, b)
    # the launchers pass exactly these sizes and request the ceiling
    inc = open(os.path.join(CSRC, "vp_stft_lock.inc")).read()
    assert "vp_k_stft_pv_lock, grid, block, vp_stft_lock_lds_bytes(a.hop)" in inc
    assert "vp_k_pv_stream_lock, dim3(a.S), dim3(64 * NWV), vp_pv_lock_lds_bytes()" in inc
    assert inc.count("hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512") == 2
