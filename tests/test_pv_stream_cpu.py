"""CPU-side checks of the streaming phase vocoder (include/vp_amd.h vp_pv_*): symbols, argument checks before the device is touched,
the C++ adapter, and the semantics on the NumPy restatement (tests/pv_stream_reference.py) -- equivalence with the one-shot
restatement delayed by the latency, and the latency's minimality.  The kernel itself is checked on the GPU
(tests/test_gpu_pv_stream.py)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_stream_reference as P  # noqa: E402
import stft_reference as R  # noqa: E402

SYMBOLS = ["vp_pv_create", "vp_pv_destroy", "vp_pv_get_latency", "vp_pv_set_semitones", "vp_pv_get_semitones", "vp_pv_reset",
           "vp_pv_process_block", "vp_pv_process_blocks_device", "vp_pv_debug_alloc_count"]


@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    L = C.CDLL(build.build())
    L.vp_pv_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    return L


def test_every_new_symbol_is_exported(lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    txt = open(os.path.join(ROOT, "include", "vp_amd.h")).read()
    for s in SYMBOLS:
        assert s + "(" in txt, s
    assert lib.vp_abi_version() == 3


@pytest.mark.parametrize("args,rc", [
    ((0, 4, 256, 1000, 256), -4), ((0, 4, 256, 2048, 512), -4), ((0, 4, 256, 1024, 1024), -4), ((0, 4, 256, 1024, 32), -4),
    ((0, 4, 256, 1024, 200), -4),
    ((0, 0, 256, 1024, 256), -1), ((0, 4, 0, 1024, 256), -1), ((0, 4, -5, 1024, 256), -1), ((0, 4, 256, 1024, 0), -1),
    ((0, -1, 256, 1024, 256), -1),
])
def test_create_rejects_bad_arguments_before_the_device(lib, args, rc):
    h = C.c_void_p()
    assert lib.vp_pv_create(*args, C.byref(h)) == rc
    assert not h.value
    assert lib.vp_pv_create(0, 4, 256, 1024, 256, None) == -1


def test_null_handle_calls_fail(lib):
    lib.vp_pv_set_semitones.argtypes = [C.c_void_p, C.c_int, C.c_double]
    lib.vp_pv_debug_alloc_count.restype = C.c_long
    assert lib.vp_pv_destroy(None) == -1
    assert lib.vp_pv_get_latency(None) == -1
    assert lib.vp_pv_set_semitones(None, 0, 1.0) == -1
    assert lib.vp_pv_reset(None, -1) == -1
    assert lib.vp_pv_process_block(None, None, None) == -1
    assert lib.vp_pv_debug_alloc_count(None) == -1


def test_create_without_gpu_is_no_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for hop in (64, 128, 256, 512):
        h = C.c_void_p()
        assert lib.vp_pv_create(0, 4, 100, 1024, hop, C.byref(h)) == -6 and not h.value
    from vocoderproject_amd import PhaseVocoderStream, VpError
    with pytest.raises(VpError) as e:
        PhaseVocoderStream(4, 256)
    assert e.value.code == -6


def test_cpp_streaming_pitch_shifter_compiles_links_and_throws(tmp_path):
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
#include <vector>
int main() {
    try {
        vp::StreamingPitchShifter ps(0, 2, 256, 128);
        ps.setSemitones(7.0);
        ps.setSemitones(-5.0, 1);
        std::vector<float> in(2 * 256, 0.f), out(2 * 256);
        ps.processBlock(in.data(), out.data());
        ps.reset(1);
        std::printf("latency %d semitones %g\n", ps.latency(), ps.semitones(1));
        return ps.latency() == 896 && ps.semitones(1) == -5.0 ? 0 : 1;
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
    rc = subprocess.call([str(exe)])
    assert rc == (0 if torch.cuda.is_available() else 42)


def test_latency_formula():
    assert [P.latency(N, 256) for N in (1024, 4096, 64, 100, 256, 1000)] == [768, 768, 960, 1020, 768, 1016]
    assert P.latency(100, 128) == 1020 and P.latency(1024, 128) == 896 and P.latency(512, 512) == 512


@pytest.mark.parametrize("hop", [64, 128, 256, 512])
@pytest.mark.parametrize("N", [17, 64, 100, 256, 1000, 1024, 4096])
def test_restatement_equals_one_shot_delayed_by_latency(N, hop):
    rng = np.random.default_rng(N + hop)
    T = N * max(6, -(-7000 // N))
    x = rng.standard_normal(T).astype(np.float32).astype(np.float64)
    ratio = 2.0 ** (-5 / 12)
    y, s = P.stream(x, N, hop, ratio, calls=[1, 3, 2])
    L = s.L
    assert L == 1024 - math.gcd(N, hop)
    ref = R.stft_roundtrip(x, 1024, hop, ratio)
    assert np.all(y[:L] == 0)
    assert np.abs(y[L:] - ref[:T - L]).max() <= 1e-12
    # grouping of the calls does not matter
    y1, _ = P.stream(x, N, hop, ratio)
    assert np.array_equal(y, y1)


@pytest.mark.parametrize("hop", [64, 128, 256, 512])
@pytest.mark.parametrize("N", [17, 64, 100, 256, 1000, 1024, 4096])
def test_latency_is_minimal(N, hop):
    """With L every emitted sample is finished when it leaves; with L - 1 some emitted sample is not, within hop / gcd(N, hop)
    blocks (+ the blocks before the first frame)."""
    s = P.PvStreamRef(N, hop, ratio=1.0)
    L = s.L
    n_blocks = hop // math.gcd(N, hop) + -(-1024 // N) + 2
    late = []
    for _ in range(n_blocks):
        s.process(np.zeros(N))
        emitted_end = s.n - L                      # one-shot samples [.., s.n - L) have left
        assert emitted_end <= max(0, s.finished_before()) or emitted_end <= 0
        late.append(s.n - (L - 1) > s.finished_before() and s.n - (L - 1) > 0)
    assert any(late), "L - 1 would have been enough"


class _DelayStream:
    """PhaseVocoderStream's interface (set_semitones, latency, process), the DSP replaced by a delay of `latency` samples."""

    def __init__(self, S, N, latency=960):
        self.S, self.N, self._lat, self.semi = S, N, latency, {}
        self.hist = np.zeros((S, latency), np.float32)

    def set_semitones(self, v, stream=-1):
        self.semi[stream] = v

    @property
    def latency(self):
        return self._lat

    def process(self, x):
        assert x.shape == (self.S, self.N) and x.flags.c_contiguous
        cat = np.concatenate([self.hist, x], axis=1)
        self.hist = cat[:, -self._lat:]
        return cat[:, :self.N]


def test_pvshift_flow_aligns_output_with_input():
    from vocoderproject_amd import offline
    v = [np.arange(1, 2501, dtype=np.float32) / 4096, np.linspace(-1, 1, 700).astype(np.float32), np.zeros(0, np.float32)]
    p = _DelayStream(3, 256, latency=960)
    out = offline.pv_shift(v, [7, -5, 0], N=256, processor=p)
    assert p.semi == {0: 7.0, 1: -5.0, 2: 0.0}
    assert [o.shape for o in out] == [(2, 2500), (2, 700), (2, 0)]
    for o, x in zip(out, v):
        np.testing.assert_array_equal(o[0], x)
        np.testing.assert_array_equal(o[1], x)
    with pytest.raises(ValueError):
        offline.pv_shift(v, [1, 2], N=256, processor=_DelayStream(3, 256))


def test_pvshift_command_line_needs_a_shift(tmp_path):
    from vocoderproject_amd import offline
    f = str(tmp_path / "a.wav")
    offline.write_wav(f, 44100, np.zeros(100))
    with pytest.raises(SystemExit):
        offline.main(["pvshift", f, "--out-dir", str(tmp_path)])
