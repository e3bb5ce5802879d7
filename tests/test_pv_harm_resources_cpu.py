"""CPU-side checks of the harmonizer's host layers, from the built library (no GPU): the entry points that need no device answer as
documented; the C++ mirror compiles with -Wall -Werror and links; and the Python front ends raise before any launch.  (The kernels'
budgets and the part's place in the build are rows of tests/test_stft_parts_cpu.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    return C.CDLL(build.build())


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
