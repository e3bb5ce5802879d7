"""CPU-side check of the two sub-bin peak-locked kernels' budgets, from the built library (no GPU, no compiler run): each exists, uses no
scratch, spills no vector register and fits the 512 registers a lane has at one wavefront per SIMD (tools/kernel_resources.py reads the
code object's metadata); they have no static LDS; their dynamic LDS is the locked parents', byte for byte (a peak's offset lies in a free
slot of the locked stage's rows), under the 163 328-byte ceiling at every hop and for the stream; the locked kernels they are copies of
are still there with no scratch; and both copies keep the VP_POISON_LDS prologue."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = {"vp_k_stft_pv_lockf": "vp_k_stft_pv_lock", "vp_k_pv_stream_lockf": "vp_k_pv_stream_lock"}
LDS_CEILING = 160 * 1024 - 512
assert LDS_CEILING == 163328
CSRC = os.path.join(ROOT, "vocoderproject_amd", "csrc")


@pytest.fixture(scope="module")
def resources():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    return kernel_resources.kernel_resources(build.build())


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_each_subbin_kernel_is_built_without_scratch_within_512_registers(resources, kernel):
    assert kernel in resources, sorted(k for k in resources if "stft" in k or "pv_" in k)
    r = resources[kernel]
    print(f"PV LOCKF resources {kernel} {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    # (on this target the metadata's vgpr_count already contains the AGPRs, so the sum asks more than the hardware does)
    assert r["vgpr"] + r["agpr"] <= 512, r
    assert r["lds"] == 0, r                                    # no static LDS: everything is the dynamic carve
    parent = KERNELS[kernel]
    assert parent in resources and resources[parent]["scratch"] == 0, (parent, resources.get(parent))
    print(f"PV LOCKF resources parent {parent} {resources[parent]}")


def test_the_copies_are_marked_included_behind_their_parent_and_listed_for_the_build():
    # (it enters vp_stft.hip directly behind the locked family's file, from that file's last line: the list of parts that vp_stft.hip
    # itself includes is pinned by tests/test_pv_cross_resources_cpu.py)
    assert '#include "vp_stft_lock.inc"' in open(os.path.join(CSRC, "vp_stft.hip")).read()
    parent = open(os.path.join(CSRC, "vp_stft_lock.inc")).read()
    assert parent.rstrip().endswith('#include "vp_stft_lockf.inc"') and parent.count("#include") == 1
    inc = open(os.path.join(CSRC, "vp_stft_lockf.inc")).read()
    for k in KERNELS:
        assert f"void {k}(" in inc, k
    assert inc.count("#ifdef VP_POISON_LDS") == 2
    assert inc.count("lockf:") >= 8                            # what differs from the parents is marked
    assert "atomic" not in inc.lower()                         # the stage is a gather: no scatter, no LDS atomics
    assert inc.count("asm volatile") == 2                      # the parents' one empty statement each, nothing more
    from vocoderproject_amd import build
    assert "vp_stft_lockf.inc" in build.DEPS


def test_dynamic_lds_is_the_locked_parents_and_fits_the_ceiling_at_every_hop():
    from vocoderproject_amd import build
    lib = C.CDLL(build.build())
    one = getattr(lib, "_Z23vp_stft_lockf_lds_bytesi")         # size_t vp_stft_lockf_lds_bytes(int hop)
    one.restype, one.argtypes = C.c_size_t, [C.c_int]
    parent = getattr(lib, "_Z22vp_stft_lock_lds_bytesi")       # size_t vp_stft_lock_lds_bytes(int hop)
    parent.restype, parent.argtypes = C.c_size_t, [C.c_int]
    fstream = getattr(lib, "_Z21vp_pv_lockf_lds_bytesv")       # size_t vp_pv_lockf_lds_bytes()
    fstream.restype = C.c_size_t
    lstream = getattr(lib, "_Z20vp_pv_lock_lds_bytesv")        # size_t vp_pv_lock_lds_bytes()
    lstream.restype = C.c_size_t
    sizes = {hop: one(hop) for hop in (64, 128, 256, 512)}
    for hop, b in sizes.items():
        assert b == parent(hop), (hop, b, parent(hop))
    sizes["stream"] = fstream()
    assert fstream() == lstream() == 144400
    print(f"PV LOCKF dynamic LDS {sizes}")
    for k, b in sizes.items():
        assert 4 * 8192 < b < LDS_CEILING, (k, b)
    # the launchers pass exactly these sizes and request the ceiling
    inc = open(os.path.join(CSRC, "vp_stft_lockf.inc")).read()
    assert "vp_k_stft_pv_lockf, grid, block, vp_stft_lockf_lds_bytes(a.hop)" in inc
    assert "vp_k_pv_stream_lockf, dim3(a.S), dim3(64 * NWV), vp_pv_lockf_lds_bytes()" in inc
    assert inc.count("hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512") == 2
