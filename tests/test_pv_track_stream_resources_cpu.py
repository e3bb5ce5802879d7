"""CPU-side check of the streaming pitch tracker's kernel budget, from the built library (no GPU, no compiler run): both new kernels
exist; vp_k_yin_track_stream uses no scratch, spills nothing, needs no AGPRs and no static LDS and stays within the 128 registers that let
four wavefronts share a SIMD, like the batch kernel whose body it includes; its dynamic LDS is the batch kernel's formula; and the batch
tracker and the phase-vocoder kernels beside it keep the figures tests/test_pv_track_resources_cpu.py pins."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_pv_track_resources_cpu as BATCH  # noqa: E402

KERNEL, FOLLOW = "vp_k_yin_track_stream", "vp_k_track_follow"


@pytest.fixture(scope="module")
def resources():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    return kernel_resources.kernel_resources(build.build())


def test_both_kernels_are_built_and_the_tracker_stays_within_128_registers(resources):
    assert KERNEL in resources and FOLLOW in resources, sorted(k for k in resources if "track" in k)
    r = resources[KERNEL]
    print(f"PV TRACK STREAM resources {KERNEL} {r}")
    print(f"PV TRACK STREAM resources {FOLLOW} {resources[FOLLOW]}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["agpr"] == 0 and r["vgpr"] <= BATCH.REGISTER_BOUND, r
    assert r["lds"] == 0, r                                    # no static LDS: the wavefronts' slices are the launch's dynamic LDS
    f = resources[FOLLOW]
    assert f["scratch"] == 0 and f["vgpr_spill"] == 0 and f["sgpr_spill"] == 0, f


def test_batch_tracker_and_neighbours_keep_their_figures(resources):
    r = resources[BATCH.KERNEL]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["agpr"] == 0 and r["lds"] == 0, r
    # as tools/kernel_resources.py printed them for the library without the streaming tracker (the two kernels share a translation unit and a body)
    assert (r["vgpr"], r["sgpr"]) == (72, 54), r
    for kernel, want in BATCH.NEIGHBOURS.items():
        n = resources[kernel]
        assert (n["vgpr"], n["agpr"], n["sgpr"], n["scratch"], n["lds"]) == want, (kernel, n)


def test_dynamic_lds_is_the_batch_kernels():
    """The launcher passes vp_track_lds_bytes(F), the formula tests/test_pv_track_resources_cpu.py pins: one slice per wavefront, four per
    workgroup, whatever the block size."""
    src = open(os.path.join(ROOT, "vocoderproject_amd", "csrc", "vp_track.hip")).read()
    launch = src[src.index("hipError_t vp_track_stream_launch"):]
    launch = launch[:launch.index("\n}\n")]
    assert "vp_k_yin_track_stream, dim3(grid), dim3(64 * VP_TRACK_WAVES), vp_track_lds_bytes(a.F), st, a" in launch, launch
    BATCH.test_dynamic_lds_follows_the_frame_length()
