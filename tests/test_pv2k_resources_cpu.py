"""CPU-side check of the 2048-point phase-vocoder kernel's two budgets, from the built library (no GPU, no compiler run):
vp_k_stft_pv2k exists, uses no scratch and fits the 512 registers a lane has at one wavefront per SIMD (tools/kernel_resources.py reads
the code object's metadata), and its dynamic LDS stays under the ceiling vp_stft_prepare_device sets at every hop."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "vp_k_stft_pv2k"
LDS_CEILING = 160 * 1024 - 512


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
    print(f"PV2K resources {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    # (on this target the metadata's vgpr_count already contains the AGPRs, so the sum asks more than the hardware does)
    assert r["vgpr"] + r["agpr"] <= 512, r


def test_dynamic_lds_fits_the_ceiling_at_every_hop():
    from vocoderproject_amd import build
    lib = C.CDLL(build.build())
    fn = getattr(lib, "_Z22vp_stft_pv2k_lds_bytesi")          # size_t vp_stft_pv2k_lds_bytes(int hop), a C++ symbol like vp_pv_lds_bytes()
    fn.restype, fn.argtypes = C.c_size_t, [C.c_int]
    sizes = {hop: fn(hop) for hop in (128, 256, 512, 1024)}
    print(f"PV2K dynamic LDS {sizes}")
    for hop, b in sizes.items():
        # at least the slots, the carry and one (magnitude, frequency) pair, two phases and the accumulator per bin
        assert 4 * 8192 + (2048 - hop) * 4 + 1025 * 8 * 5 <= b <= LDS_CEILING, (hop, b)
    assert sizes[128] > sizes[256] > sizes[512] > sizes[1024]
