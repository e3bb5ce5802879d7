"""CPU-side checks of the cross-synthesis host layers, from the built library (no GPU): vp_xs_debug_alloc_count(NULL) is -1; the argument
checks that need no device answer as documented; the C++ mirror compiles with -Wall -Werror and links; and the Python front ends raise
before any launch.  (The kernels' budgets and the part's place in the build are rows of tests/test_stft_parts_cpu.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    return C.CDLL(build.build())


def test_null_handles_answer_without_a_device(lib):
    lib.vp_xs_debug_alloc_count.restype = C.c_long
    lib.vp_xs_debug_alloc_count.argtypes = [C.c_void_p]
    assert lib.vp_xs_debug_alloc_count(None) == -1
    lib.vp_xs_get_latency.argtypes = lib.vp_xs_destroy.argtypes = [C.c_void_p]
    lib.vp_xs_reset.argtypes = [C.c_void_p, C.c_int]
    assert lib.vp_xs_get_latency(None) == -1 and lib.vp_xs_reset(None, 0) == -1 and lib.vp_xs_destroy(None) == -1
    lib.vp_stft_cross_synth.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    assert lib.vp_stft_cross_synth(None, 8, 8, 8, None, 32, None) == -1
    lib.vp_xs_process_blocks_device.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p]
    assert lib.vp_xs_process_blocks_device(None, 8, 8, 8, None, 32, 1, None) == -1
    # the geometry is refused before a device is looked for
    lib.vp_xs_create.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert lib.vp_xs_create(0, 2, 256, 2048, 512, C.byref(h)) == -4 and not h.value        # VP_ERR_GEOMETRY
    assert lib.vp_xs_create(0, 2, 256, 1024, 1024, C.byref(h)) == -4 and not h.value
    assert lib.vp_xs_create(0, 0, 256, 1024, 256, C.byref(h)) == -1 and lib.vp_xs_create(0, 2, 256, 1024, 256, None) == -1


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
    if (vp_xs_debug_alloc_count(nullptr) != -1) return 2;
    try {
        vp::StreamingCrossSynth xs(0, 4, 256, 128);
        xs.reset();
        xs.reset(3);
        std::printf("latency %d allocs %ld\n", xs.latency(), xs.debugAllocCount());
        try { xs.processBlocksDevice(nullptr, nullptr, nullptr, nullptr, 1); return 3; } catch (const vp::Error &e) { if (e.code != VP_ERR_INVALID_ARG) return 4; }
        return xs.latency() == 1024 - 128 && xs.handle() ? 0 : 5;
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


def _bad_calls(call, shape):
    import torch
    ok = lambda p: _Tensor(shape, ptr=p)                       # noqa: E731
    other = tuple(shape[:-1]) + (shape[-1] + 1,)
    yield "dtype", lambda: call(_Tensor(shape, torch.float64), ok(2), ok(3), lifter=32)
    yield "dtype", lambda: call(ok(1), ok(2), _Tensor(shape, torch.float16, ptr=3), lifter=32)
    yield "host", lambda: call(ok(1), _Tensor(shape, cuda=False, ptr=2), ok(3), lifter=32)
    yield "strided", lambda: call(ok(1), ok(2), _Tensor(shape, contiguous=False, ptr=3), lifter=32)
    yield "mismatch", lambda: call(ok(1), _Tensor(other, ptr=2), ok(3), lifter=32)
    yield "shape", lambda: call(_Tensor(other, ptr=1), _Tensor(other, ptr=2), ok(3), lifter=32)
    yield "out shape", lambda: call(ok(1), ok(2), _Tensor(other, ptr=3), lifter=32)
    yield "alias", lambda: call(ok(1), ok(2), ok(2), lifter=32)
    yield "lifter 3", lambda: call(ok(1), ok(2), ok(3), lifter=3)
    yield "lifter 65", lambda: call(ok(1), ok(2), ok(3), lifter=65)
    yield "depth count", lambda: call(ok(1), ok(2), ok(3), depth=[1.0] * (shape[-2] + 1))
    yield "depth nan", lambda: call(ok(1), ok(2), ok(3), depth=float("nan"))
    yield "d_depth", lambda: call(ok(1), ok(2), ok(3), d_depth=_Tensor((shape[-2],), torch.float32))


def test_python_front_ends_raise_before_any_launch():
    from vocoderproject_amd import CrossSynthStream, StftRoundTrip
    import vocoderproject_amd
    assert "CrossSynthStream" in dir(vocoderproject_amd)
    st = StftRoundTrip.__new__(StftRoundTrip)
    st.L, st.h, st.S, st.T, st.F, st.hop = _NoLaunch(), None, 3, 4096, 1024, 256
    for what, bad in _bad_calls(st.cross_synth, (3, 4096)):
        with pytest.raises(ValueError):
            bad()
    xs = CrossSynthStream.__new__(CrossSynthStream)
    xs.L, xs.h, xs.S, xs.N, xs.F, xs.hop, xs.device = _NoLaunch(), None, 3, 256, 1024, 256, 0
    for what, bad in _bad_calls(lambda v, c, o, **kw: xs.process_device(v, c, o, n_blocks=2, **kw), (2, 3, 256)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        xs.process_device(_Tensor((3, 256), ptr=1), _Tensor((3, 256), ptr=2), _Tensor((3, 256), ptr=3), n_blocks=0)
    with pytest.raises(ValueError):
        xs.process_device(_Tensor((3, 256), ptr=1), _Tensor((3, 256), ptr=2), _Tensor((3, 256), ptr=3), n_blocks=2)     # [S][N] is one block
    z = np.zeros((3, 700), np.float32)
    for v, c, kw in ((z, z[:2], {}), (z, z[:, :699], {}), (z[0], z[0], {}), (z, z, dict(lifter=3)), (z, z, dict(lifter=65))):
        with pytest.raises(ValueError):
            xs.run(v, c, **kw)
    xs.h = st.h = None                                         # (nothing to destroy)
