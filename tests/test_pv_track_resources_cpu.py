"""CPU-side check of the pitch tracker's kernel budget, from the built library (no GPU, no compiler run): vp_k_yin_track exists, uses no
scratch, spills nothing, needs no static LDS and stays within the 128 registers that let four wavefronts share a SIMD (DESIGN.md section
4.6; tools/kernel_resources.py reads the code object's metadata); its dynamic LDS is what the launcher's formula says and lets several
workgroups share a compute unit; and the phase-vocoder kernels beside it keep the figures they had before the tracker joined the
library."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "vp_k_yin_track"
REGISTER_BOUND = 128
# (vgpr, agpr, sgpr, scratch, static LDS) of the fixed-shift, curve, stretch and streaming kernels as tools/kernel_resources.py printed them
# for the library without the tracker: the tracker is a translation unit of its own and must not move them
NEIGHBOURS = {
    "vp_k_stft_fused<true, false>": (341, 85, 106, 0, 0),
    "vp_k_stft_pv2k": (374, 118, 92, 0, 0),
    "vp_k_stft_pv_curve": (346, 90, 106, 0, 0),
    "vp_k_stft_pv2k_curve": (370, 114, 83, 0, 0),
    "vp_k_stft_pv_stretch": (346, 90, 106, 0, 0),
    "vp_k_stft_pv2k_stretch": (378, 122, 92, 0, 0),
    "vp_k_pv_stream": (337, 81, 106, 0, 0),
    "vp_k_pv_stream_curve": (334, 78, 106, 0, 0),
}


@pytest.fixture(scope="module")
def resources():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    return kernel_resources.kernel_resources(build.build())


def test_tracker_kernel_is_built_without_scratch_within_128_registers(resources):
    assert KERNEL in resources, sorted(k for k in resources if "stft" in k or "track" in k)
    r = resources[KERNEL]
    print(f"PV TRACK resources {KERNEL} {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["agpr"] == 0 and r["vgpr"] <= REGISTER_BOUND, r
    assert r["lds"] == 0, r                                    # no static LDS: the wavefronts' slices are the launch's dynamic LDS


@pytest.mark.parametrize("kernel", sorted(NEIGHBOURS))
def test_phase_vocoder_kernels_keep_their_figures(resources, kernel):
    r = resources[kernel]
    assert (r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"]) == NEIGHBOURS[kernel], (kernel, r)


def test_dynamic_lds_follows_the_frame_length():
    from vocoderproject_amd import build
    lib = C.CDLL(build.build())
    f = getattr(lib, "_Z18vp_track_lds_bytesi")                # size_t vp_track_lds_bytes(int F)
    f.restype, f.argtypes = C.c_size_t, [C.c_int]
    # four wavefronts, each F / 8 + 64 rows of eight samples in nine words
    assert f(1024) == 4 * (1024 // 8 + 64) * 9 * 4 == 27648 and f(2048) == 4 * (2048 // 8 + 64) * 9 * 4 == 46080
    # a slice also holds the normalised function (513 doubles), and at least three workgroups (twelve wavefronts) fit a compute unit's 160 KB
    assert f(1024) // 4 >= 513 * 8 and 3 * f(2048) <= 160 * 1024
