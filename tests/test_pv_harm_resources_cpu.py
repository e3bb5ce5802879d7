"""CPU-side check of the two harmonizer kernels' budgets, from the built library and the sources (no GPU, no compiler run): each exists
and uses no scratch (tools/kernel_resources.py reads the code object's metadata) within the 512 registers a lane has at one wavefront
per SIMD; they have no static LDS; their dynamic LDS -- the locked parents' carve plus three more angle arrays -- stays under the
163 328-byte ceiling at every hop and for the stream with all four voices; the locked kernels they are copies of, and those kernels'
parents, keep the figures profiles/pv_lock_resources.txt records; the new part is entered behind the locked family and known to the
build; the entry points that need no device answer as documented; the C++ mirror compiles with -Wall -Werror and links; and the Python
front ends raise before any launch."""
import ast
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = {"vp_k_stft_harm": "vp_k_stft_pv_lock", "vp_k_hz_stream": "vp_k_pv_stream_lock"}
LDS_CEILING = 160 * 1024 - 512
assert LDS_CEILING == 163328
EXTRA = 3 * 513 * 8                                            # the angle arrays of voices 1 .. 3
CSRC = os.path.join(ROOT, "vocoderproject_amd", "csrc")


@pytest.fixture(scope="module")
def resources():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    return kernel_resources.kernel_resources(build.build())


@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    return C.CDLL(build.build())


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_each_harmonizer_kernel_is_built_without_scratch(resources, kernel):
    assert kernel in resources, sorted(k for k in resources if "stft" in k or "hz_" in k)
    r = resources[kernel]
    print(f"PV HARM resources {kernel} {r}")
    assert r["scratch"] == 0, r
    # (on this target the metadata's vgpr_count already contains the AGPRs, so the sum asks more than the hardware does)
    assert r["vgpr"] <= 512, r
    assert r["lds"] == 0, r                                    # no static LDS: everything is the dynamic carve
    assert "vp_k_hz_update" in resources and resources["vp_k_hz_update"]["scratch"] == 0


def test_the_locked_kernels_and_their_parents_keep_their_recorded_figures(resources):
    txt = open(os.path.join(ROOT, "profiles", "pv_lock_resources.txt")).read()
    rows = dict(re.findall(r"^(vp_k_\S+(?: \S+>)?)\s+(\{.*\})$", txt, re.M))
    assert len(rows) == 6 and set(KERNELS.values()) <= set(rows), sorted(rows)
    for k, rec in rows.items():
        assert k in resources, k
        assert resources[k] == ast.literal_eval(rec), (k, resources[k], rec)


def test_dynamic_lds_is_the_locked_carve_plus_three_angle_arrays_under_the_ceiling(lib):
    one = getattr(lib, "_Z22vp_stft_harm_lds_bytesi")          # size_t vp_stft_harm_lds_bytes(int hop)
    one.restype, one.argtypes = C.c_size_t, [C.c_int]
    parent = getattr(lib, "_Z22vp_stft_lock_lds_bytesi")       # size_t vp_stft_lock_lds_bytes(int hop)
    parent.restype, parent.argtypes = C.c_size_t, [C.c_int]
    hstream = getattr(lib, "_Z15vp_hz_lds_bytesv")             # size_t vp_hz_lds_bytes()
    hstream.restype = C.c_size_t
    lstream = getattr(lib, "_Z20vp_pv_lock_lds_bytesv")        # size_t vp_pv_lock_lds_bytes()
    lstream.restype = C.c_size_t
    sizes = {hop: one(hop) for hop in (64, 128, 256, 512)}
    for hop, b in sizes.items():
        assert b == parent(hop) + EXTRA, (hop, b, parent(hop))
    sizes["stream"] = hstream()
    assert hstream() == lstream() + EXTRA == 144400 + 12312
    assert sizes[64] == 127760 + 12312
    print(f"PV HARM dynamic LDS {sizes}")
    for k, b in sizes.items():
        assert 4 * 8192 < b <= LDS_CEILING, (k, b)
    # the launchers pass exactly these sizes (whatever the number of voices: the carve is for four) and request the ceiling
    inc = open(os.path.join(CSRC, "vp_stft_harm.inc")).read()
    assert "vp_k_stft_harm, grid, block, vp_stft_harm_lds_bytes(a.hop)" in inc
    assert "vp_k_hz_stream, dim3(a.S), dim3(64 * NWV), vp_hz_lds_bytes()" in inc
    assert inc.count("hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512") == 2
    assert "#define VP_HARM_MAX_VOICES 4" in open(os.path.join(CSRC, "vp_stft.h")).read()
    assert "#define VP_HARM_MAX_VOICES 4" in open(os.path.join(ROOT, "include", "vp_amd.h")).read()


def test_the_copies_are_marked_entered_behind_the_locked_family_and_listed_for_the_build():
    # (the list of parts vp_stft.hip itself includes is pinned by tests/test_pv_cross_resources_cpu.py, and vp_stft_lock.inc's one include by
    # tests/test_pv_lockf_resources_cpu.py: the new part enters from the last line of vp_stft_lockf.inc)
    tail = open(os.path.join(CSRC, "vp_stft_lockf.inc")).read()
    assert tail.rstrip().endswith('#include "vp_stft_harm.inc"') and tail.count("#include") == 1
    inc = open(os.path.join(CSRC, "vp_stft_harm.inc")).read()
    for k in KERNELS:
        assert f"void {k}(" in inc, k
    assert inc.count("#ifdef VP_POISON_LDS") == 2
    assert inc.count("harm:") >= 10                            # what differs from the parents is marked
    assert "atomic" not in inc.lower()                         # the stage is a gather: no scatter, no LDS atomics
    assert inc.count("asm volatile") == 2                      # the parents' one empty statement each, nothing more
    assert inc.count("#pragma nounroll") == 2                  # the voice loop is a run-time loop in both kernels
    assert "while" not in inc                                  # no wait that can spin: the bounded loops are the parents'
    # the parents' text is as it was: their helpers are still what their kernels call
    lock = open(os.path.join(CSRC, "vp_stft_lock.inc")).read()
    for name in ("pv_lock_plan", "pv_lock_turn", "pv_lock_gather"):
        assert lock.count(name + "(") == 3, name               # one definition, two kernels
        assert name + "(" not in inc, name                     # the new kernels call the split helpers of their own file
    from vocoderproject_amd import build
    assert "vp_stft_harm.inc" in build.DEPS
    assert re.search(r'"vp_stft\.hip": \[[^\]]*"vp_stft_harm\.inc"', open(os.path.join(ROOT, "vocoderproject_amd", "build.py")).read())


def test_the_recorded_figures_are_the_built_ones(resources):
    txt = open(os.path.join(ROOT, "profiles", "pv_harm_resources.txt")).read()
    rows = dict(re.findall(r"^(vp_k_\S+)\s+(\{.*\})$", txt, re.M))
    for k in KERNELS:
        assert k in rows and resources[k] == ast.literal_eval(rows[k]), (k, resources[k], rows.get(k))


def test_null_handles_and_bad_arguments_answer_without_a_device(lib):
    lib.vp_hz_debug_alloc_count.restype = C.c_long
    lib.vp_hz_debug_alloc_count.argtypes = [C.c_void_p]
    assert lib.vp_hz_debug_alloc_count(None) == -1
    lib.vp_hz_get_latency.argtypes = lib.vp_hz_destroy.argtypes = [C.c_void_p]
    lib.vp_hz_reset.argtypes = [C.c_void_p, C.c_int]
    assert lib.vp_hz_get_latency(None) == -1 and lib.vp_hz_reset(None, 0) == -1 and lib.vp_hz_destroy(None) == -1
    lib.vp_stft_harmonize.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4
    assert lib.vp_stft_harmonize(None, 8, 8, 1, 8, None, None, None) == -1
    lib.vp_hz_process_blocks_device.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    assert lib.vp_hz_process_blocks_device(None, 8, 8, 8, None, None, 1, None) == -1
    # voice count and geometry are refused before a device is looked for
    lib.vp_hz_create.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    for V in (0, 5, -1):
        assert lib.vp_hz_create(0, 2, 256, 1024, 256, V, C.byref(h)) == -1 and not h.value
    assert lib.vp_hz_create(0, 2, 256, 2048, 512, 3, C.byref(h)) == -4 and not h.value       # VP_ERR_GEOMETRY
    assert lib.vp_hz_create(0, 2, 256, 1024, 1024, 3, C.byref(h)) == -4 and not h.value
    assert lib.vp_hz_create(0, 0, 256, 1024, 256, 3, C.byref(h)) == -1 and lib.vp_hz_create(0, 2, 256, 1024, 256, 3, None) == -1


def test_cpp_mirror_compiles_with_werror_and_links(tmp_path):
    import shutil
    import subprocess
    from vocoderproject_amd import build
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    lib = build.build()
    src = tmp_path / "t.cpp"
    src.write_text(r"""
#include "vp_amd.hpp"
#include <cstdio>
int main() {
    if (vp_hz_debug_alloc_count(nullptr) != -1) return 2;
    static_assert(VP_HARM_MAX_VOICES == 4, "voices");
    try {
        vp::StreamingHarmonizer hz(0, 4, 256, 3, 128);
        hz.reset();
        hz.reset(3);
        std::printf("latency %d allocs %ld\n", hz.latency(), hz.debugAllocCount());
        try { hz.processBlocksDevice(nullptr, nullptr, nullptr, nullptr, nullptr, 1); return 3; } catch (const vp::Error &e) { if (e.code != VP_ERR_INVALID_ARG) return 4; }
        return hz.latency() == 1024 - 128 && hz.handle() ? 0 : 5;
    } catch (const vp::Error &e) {
        std::printf("vp::Error %d\n", e.code);
        return e.code == VP_ERR_NO_DEVICE ? 42 : 1;
    }
}
""")
    exe = tmp_path / "t"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), lib,
                           "-Wl,-rpath," + os.path.dirname(lib)])
    import torch
    assert subprocess.call([str(exe)]) == (0 if torch.cuda.is_available() else 42)


# ---- the Python front ends: every check raises before a launch (the library is a stand-in whose entry points fail the test) ----------------
class _NoLaunch:
    def __getattr__(self, name):
        raise AssertionError(f"{name} called: the check must come before any launch")


class _Tensor:
    """What the checks look at of a torch tensor."""

    def __init__(self, shape, dtype=None, cuda=True, contiguous=True, ptr=4096):
        import torch
        self.shape, self.dtype, self.is_cuda, self._c, self._p = tuple(shape), dtype or torch.float32, cuda, contiguous, ptr
        self.device = "cuda:0"

    def is_contiguous(self):
        return self._c

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        return self._p


def test_python_front_ends_raise_before_any_launch():
    import torch
    from vocoderproject_amd import HarmonizerStream, StftRoundTrip
    import vocoderproject_amd
    assert "HarmonizerStream" in dir(vocoderproject_amd)
    st = StftRoundTrip.__new__(StftRoundTrip)
    st.L, st.h, st.S, st.T, st.F, st.hop, st.n_frames, st._curve_tables = _NoLaunch(), None, 3, 4096, 1024, 256, 13, {}
    ok = lambda p, shape=(3, 4096): _Tensor(shape, ptr=p)     # noqa: E731
    bad = [lambda: st.harmonize(_Tensor((3, 4096), torch.float64), ok(2), semitones=[4.0]),
           lambda: st.harmonize(ok(1), _Tensor((3, 4096), cuda=False), semitones=[4.0]),
           lambda: st.harmonize(ok(1), _Tensor((3, 4096), contiguous=False), semitones=[4.0]),
           lambda: st.harmonize(ok(1), ok(2, (3, 4097)), semitones=[4.0]),
           lambda: st.harmonize(ok(1), ok(2)),
           lambda: st.harmonize(ok(1), ok(2), semitones=[4.0], d_ratio=_Tensor((3, 1, 13), torch.float64)),
           lambda: st.harmonize(ok(1), ok(2), semitones=[1.0, 2.0, 3.0, 4.0, 5.0]),
           lambda: st.harmonize(ok(1), ok(2), semitones=np.zeros((2, 12))),
           lambda: st.harmonize(ok(1), ok(2), semitones=np.zeros((2, 2, 13))),
           lambda: st.harmonize(ok(1), ok(2), semitones=4.0),
           lambda: st.harmonize(ok(1), ok(2), d_ratio=_Tensor((3, 5, 13), torch.float64)),
           lambda: st.harmonize(ok(1), ok(2), d_ratio=_Tensor((3, 2, 13), torch.float32)),
           lambda: st.harmonize(ok(1), ok(2), d_ratio=_Tensor((3, 2, 12), torch.float64)),
           lambda: st.harmonize(ok(1), ok(2), d_ratio=_Tensor((3, 2, 13), torch.float64), gains=[1.0, 1.0, 1.0]),
           lambda: st.harmonize(ok(1), ok(2), d_ratio=_Tensor((3, 2, 13), torch.float64), dry=[1.0, 1.0])]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    hz = HarmonizerStream.__new__(HarmonizerStream)
    hz.L, hz.h, hz.S, hz.N, hz.V, hz.F, hz.hop, hz.device, hz._tables = _NoLaunch(), None, 3, 256, 2, 1024, 256, 0, {}
    blk = lambda p, shape=(2, 3, 256): _Tensor(shape, ptr=p)  # noqa: E731
    bad = [lambda: hz.process_device(blk(1), blk(2), n_blocks=0, semitones=[4.0, 7.0]),
           lambda: hz.process_device(blk(1, (3, 256)), blk(2, (3, 256)), n_blocks=2, semitones=[4.0, 7.0]),      # [S][N] is one block
           lambda: hz.process_device(blk(1), blk(2), n_blocks=2),
           lambda: hz.process_device(blk(1), blk(2), n_blocks=2, semitones=[4.0, 7.0, 9.0]),
           lambda: hz.process_device(blk(1), blk(2), n_blocks=2, semitones=np.zeros((3, 3, 2))),
           lambda: hz.process_device(blk(1), blk(2), n_blocks=2, d_ratio=_Tensor((2, 3, 3), torch.float64)),
           lambda: hz.process_device(blk(1), _Tensor((2, 3, 256), torch.float16), n_blocks=2, semitones=[4.0, 7.0])]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    z = np.zeros((3, 700), np.float32)
    for x, stv in ((z[:2], [4.0, 7.0]), (z[0], [4.0, 7.0]), (z, [4.0]), (z, np.zeros((2, 3, 2)))):
        hz.L = type("L", (), {"vp_hz_get_latency": staticmethod(lambda h: 768)})()
        with pytest.raises(ValueError):
            hz.run(x, stv)
    hz.h = st.h = None                                         # (nothing to destroy)
