"""CPU-side check of the locked time-stretch kernel's budget, from the built library (no GPU, no compiler run): it exists, uses no scratch,
spills no vector register, fits the 512 registers a lane has at one wavefront per SIMD and has no static LDS (tools/kernel_resources.py
reads the code object's metadata); its launch passes the locked build's dynamic LDS, vp_stft_lock_lds_bytes(a.hop), and requests the
ceiling once; it keeps the VP_POISON_LDS prologue; it is a file of its own behind vp_stft_lock.inc; and the kernels it descends from are
still there under their names with the register figures their own resource tests pin."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "vp_k_stft_pv_stretch_lock"
# registers of the parents as their resource tests print them on the parent commit (vgpr, agpr)
PARENT_FIGURES = {"vp_k_stft_pv_lock": (361, 105), "vp_k_stft_pv_stretch": (346, 90), "vp_k_stft_pv_curve": (346, 90), "vp_k_stft_fused<true, false>": (341, 85)}
LDS_CEILING = 160 * 1024 - 512
CSRC = os.path.join(ROOT, "vocoderproject_amd", "csrc")


@pytest.fixture(scope="module")
def resources():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    return kernel_resources.kernel_resources(build.build())


def test_the_kernel_is_built_without_scratch_within_512_registers(resources):
    assert KERNEL in resources, sorted(k for k in resources if "stft" in k)
    r = resources[KERNEL]
    print(f"PV STRETCH LOCK resources {KERNEL} {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 512, r
    assert r["lds"] == 0, r                                    # no static LDS: everything is the dynamic carve


def test_the_parents_keep_their_register_figures(resources):
    for parent, want in PARENT_FIGURES.items():
        assert parent in resources and resources[parent]["scratch"] == 0, (parent, resources.get(parent))
        print(f"PV STRETCH LOCK resources parent {parent} {resources[parent]}")
        assert (resources[parent]["vgpr"], resources[parent]["agpr"]) == want, (parent, resources[parent])


def test_the_copy_is_a_file_of_its_own_with_the_poison_prologue_and_the_locked_carve():
    src = open(os.path.join(CSRC, "vp_stft.hip")).read()
    order = [src.index(f'#include "{f}"') for f in ("vp_stft_curve.inc", "vp_stft_stretch.inc", "vp_stft_lock.inc", "vp_stft_stretch_lock.inc", "vp_stft_formant.inc")]
    assert order == sorted(order)
    inc = open(os.path.join(CSRC, "vp_stft_stretch_lock.inc")).read()
    assert "void vp_k_stft_pv_stretch_lock(VpStftArgs A, const double *ratioTab, const int *posTab, int nIn)" in inc
    assert inc.count("#ifdef VP_POISON_LDS") == 1
    assert inc.count("stretch:") >= 10                         # what differs from vp_k_stft_pv_lock is marked
    assert "atomic" not in inc.lower()                         # the stage is a gather: no scatter, no LDS atomics
    for helper in ("pv_lock_mask(", "pv_lock_nearest(", "pv_lock_turn(", "pv_lock_gather(", "pv_lock_carve(", "pv_stretch_frame("):
        assert helper in inc, helper
    assert "__device__ __forceinline__ bool pv_stretch_lock_plan(" in inc and "pv_lock_plan(" not in inc.replace("pv_stretch_lock_plan(", "")
    # the launch passes the locked build's size, no carve of its own; one request of the ceiling, made where the others are
    assert "vp_k_stft_pv_stretch_lock, grid, block, vp_stft_lock_lds_bytes(a.hop)" in inc
    assert "const dim3 grid(1, nStreams), block(64 * NWV);" in inc
    assert inc.count("hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512") == 1
    capi = open(os.path.join(CSRC, "vp_capi.hip")).read()
    assert "vp_stft_lock_prepare_device() == hipSuccess && vp_stft_stretch_lock_prepare_device() == hipSuccess" in capi
    # the parents' files are as they were: their own tests count these
    assert open(os.path.join(CSRC, "vp_stft_lock.inc")).read().count("#ifdef VP_POISON_LDS") == 2
    assert open(os.path.join(CSRC, "vp_stft_stretch.inc")).read().count("#ifdef VP_POISON_LDS") == 2
    from vocoderproject_amd import build
    assert "vp_stft_stretch_lock.inc" in build.DEPS


def test_the_dynamic_lds_fits_the_ceiling_at_every_hop():
    from vocoderproject_amd import build
    lib = C.CDLL(build.build())
    one = getattr(lib, "_Z22vp_stft_lock_lds_bytesi")          # size_t vp_stft_lock_lds_bytes(int hop)
    one.restype, one.argtypes = C.c_size_t, [C.c_int]
    sizes = {hop: one(hop) for hop in (64, 128, 256, 512)}
    print(f"PV STRETCH LOCK dynamic LDS {sizes}")
    for hop, b in sizes.items():
        assert 4 * 8192 < b <= LDS_CEILING, (hop, b)
