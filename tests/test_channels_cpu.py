"""CPU-side checks of the channel-pointer entry points (include/vp_amd.h: vp_process_block_channels, vp_process_block_channels_device,
vp_process_blocks_channels_device): declared, exported, argument errors that need no handle, and the C++ adapter's
processBlock(in, nIn, out, nOut) as a JUCE host would call it.  The comparisons against the packed entry points are in
tests/test_gpu_channels.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vp_process_block_channels", "vp_process_block_channels_device", "vp_process_blocks_channels_device")


@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    return C.CDLL(build.build())


def test_channel_symbols_are_declared_and_exported(lib):
    txt = open(os.path.join(ROOT, "include", "vp_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*vp_handle\s*\*\s*h\s*,\s*const\s+float\s*\*\s*const\s*\*" % s, txt), f"{s} not declared in include/vp_amd.h"
        assert hasattr(lib, s), f"{s} not exported"
    assert lib.vp_abi_version() == 3                                  # additions only


def test_channel_entry_points_refuse_a_null_handle(lib):
    tab = (C.c_void_p * 6)()
    lib.vp_process_block_channels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.vp_process_block_channels_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.vp_process_blocks_channels_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert lib.vp_process_block_channels(None, tab, 3, tab, 3) == -1
    assert lib.vp_process_block_channels_device(None, tab, 3, tab, 3, None) == -1
    assert lib.vp_process_blocks_channels_device(None, tab, 3, tab, 3, 1, None) == -1


def test_python_mirror_has_the_channel_methods():
    from vocoderproject_amd import BatchVocoderProcessor
    for m in ("process_channels", "channel_table", "process_channels_device"):
        assert callable(getattr(BatchVocoderProcessor, m))


def test_cpp_adapter_process_block_with_channel_pointers(tmp_path):
    """vp::BatchVocoderProcessor::processBlock(in, 3, out, 3) on three separately allocated vectors per stream, in place, one stream without
    a side chain: compiles warning-free as C++17, links, and -- on a GPU -- gives the samples of the packed processBlock(io) of a second
    processor, bit for bit (exit 0); without a GPU the constructor throws VP_ERR_NO_DEVICE (exit 42)."""
    from vocoderproject_amd import build
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    lib = build.build()
    src = tmp_path / "t.cpp"
    src.write_text(r"""
#include "vp_amd.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
int main() {
    try {
        const int S = 3, N = 256, blocks = 10;
        vp::BatchVocoderProcessor a(0), b(0);
        a.prepareToPlay(44100.0, N, S);
        b.prepareToPlay(44100.0, N, S);
        vp::ShardedBatchProcessor sh(std::vector<int>{0, 0});
        sh.prepareToPlay(44100.0, N, S);
        std::vector<std::vector<float>> ch(S * 3, std::vector<float>(N)), ch2(S * 3, std::vector<float>(N));
        std::vector<float> io(S * 3 * N);
        double energy = 0;
        for (int k = 0; k < blocks; k++) {
            for (int s = 0; s < S; s++)
                for (int c = 0; c < 3; c++)
                    for (int i = 0; i < N; i++) {
                        const double t = (double)(k * N + i) / 44100.0, f = c == 0 ? 150.0 + 40.0 * s : 110.0 * (c + s);
                        float v = (float)(0.3 * std::sin(6.283185307179586 * f * t) + 0.1 * std::sin(6.283185307179586 * 3 * f * t));
                        if (s == 1 && c > 0) v = 0.f;                      // stream 1 has no side chain
                        ch[s * 3 + c][i] = ch2[s * 3 + c][i] = io[(s * 3 + c) * N + i] = v;
                    }
            std::vector<const float *> in(S * 3), in2(S * 3);
            std::vector<float *> out(S * 3), out2(S * 3);
            for (int r = 0; r < S * 3; r++) {
                const bool none = r / 3 == 1 && r % 3 > 0;
                in[r] = out[r] = none ? nullptr : ch[r].data();            // getReadPointer / getWritePointer of an in-place buffer
                in2[r] = out2[r] = none ? nullptr : ch2[r].data();
            }
            a.processBlock(in.data(), 3, out.data(), 3);
            sh.processBlock(in2.data(), 3, out2.data(), 3);
            b.processBlock(io.data());
            for (int r = 0; r < S * 3; r++) {
                if (!out[r]) continue;
                if (std::memcmp(ch[r].data(), &io[r * N], N * sizeof(float)) != 0) { std::printf("block %d row %d differs\n", k, r); return 2; }
                if (std::memcmp(ch2[r].data(), &io[r * N], N * sizeof(float)) != 0) { std::printf("sharded: block %d row %d differs\n", k, r); return 3; }
                if (r % 3 < 2) for (int i = 0; i < N; i++) energy += (double)io[r * N + i] * io[r * N + i];
            }
        }
        std::printf("energy %g\n", energy);
        return energy > 1.0 ? 0 : 4;                                      // (a comparison of silences would show nothing)
    } catch (const vp::Error &e) {
        std::printf("vp::Error %d\n", e.code);
        return e.code == VP_ERR_NO_DEVICE ? 42 : 1;
    }
}
""")
    exe = tmp_path / "t"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-pthread"])
    import torch
    rc = subprocess.call([str(exe)])
    assert rc == (0 if torch.cuda.is_available() else 42)
