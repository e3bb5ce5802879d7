"""The wave-specialised pitch kernel's split FAST recursion (csrc/vp_filters.inc iir_block_park / iir_block_walk): the producers park
the routine's first pass block by block behind their gather trips, the recursion wavefront is left with the walk.

The definition is the phase kernels (`set_wave_specialised(False)`): they keep calling the one-piece routine, iir_block_wave_regs.
Every comparison is bit for bit -- output, tracker state of every stream, UB-site counters -- and no bounded wait may run out.
The whole GPU suite, this file included, is rerun on the LDS-poisoning twin by tests/test_gpu_parity.py: a parked sum that is read
before it is written is a NaN there.

The CPU test at the end pins which segments park (VpWsSched::segPark, ws_build_sched) against a restatement of the rule."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 44100.0
VP_ERR_TIMEOUT = -9

# (fs, N, F, H, W, h): the plugin's own grid (chunks of 256 samples) and tests/test_gpu_round5.py's other grids: 512, 128, 64 and 128 again
GRIDS = {
    "plugin_chunk_256": None,
    "two_chunks_per_frame": (44100.0, 1024, 1024, 512, 512, 256),
    "eight_chunks_per_frame": (44100.0, 512, 1024, 896, 512, 128),
    "sixteen_chunks_per_frame": (44100.0, 256, 1024, 960, 512, 128),
    "chunk_128_block_1024": (44100.0, 1024, 1024, 896, 1024, 256),
}


def _streams(S, T, **kw):
    from vocoderproject_amd.synth import make_streams
    return np.ascontiguousarray(make_streams(S, T, **kw).numpy())


def _edge_streams(T, fs=FS):
    """gate crossings, unvoiced bursts, silence, an octave jump, clipping (tests/test_gpu_round5.py's corpus) + plain streams"""
    rng = np.random.default_rng(11)
    base = _streams(9, T, fs=fs)
    x = base.copy()
    env = np.where((np.arange(T) // 9000) % 2 == 0, 1.0, 2e-5).astype(np.float32)
    x[0, 0] *= env
    noise = (rng.standard_normal(T) * 0.08).astype(np.float32)
    x[1, 0] = np.where((np.arange(T) // 7000) % 2 == 0, noise, base[1, 0])
    x[2, 0] = 0
    x[3, 1:] = 0
    t = np.arange(T) / fs
    x[4, 0] = (0.3 * np.sin(2 * np.pi * np.where(t < t[T // 2], 101.0, 640.0) * t)).astype(np.float32)
    x[5, 0] = np.clip(base[5, 0] * 8, -1, 1)
    return np.ascontiguousarray(x)


LOW_VOICES = (90.0, 101.0, 130.0)            # periods of 490, 437 and 339 samples at 44.1 kHz: under tauMax, longer than most chunks


def _corpus(T, fs=FS):
    """three low harmonic voices (streams 0..2), then the edge corpus: twelve streams"""
    edge = _edge_streams(T, fs)
    low = _streams(len(LOW_VOICES), T, fs=fs)
    t = np.arange(T) / fs
    rng = np.random.default_rng(5)
    for s, f0 in enumerate(LOW_VOICES):
        v = sum(np.sin(2 * np.pi * h * f0 * t + 0.3 * h) / h for h in range(1, 9))
        low[s, 0] = (0.22 * v + 0.002 * rng.standard_normal(T)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([low, edge]))


def _assert_equal(got, ref, what=""):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}, max abs {np.abs(got - ref).max()}"


def _state_key(p, s):
    d = p.pitch_state(s)
    d["a"] = d["a"].tobytes()
    return sorted(d.items())


def _timeouts(p):
    v = p.debug_stamps(reset=False)
    return [round(v[i] * 100.0) for i in (59, 60, 61)]


def _make(S, N, prepare=None, ws=True, order=15, shifts=None):
    from vocoderproject_amd import BatchVocoderProcessor
    p = BatchVocoderProcessor(vocBool=0, lpcPitch=order)
    if prepare:
        p.prepareExplicit(prepare[0], N, S, *prepare[2:])
    else:
        p.prepareToPlay(FS, N, S)
    p.set_iir_mode("fast")
    p.set_yin_mode("xcorr")
    p.set_wave_specialised(ws)
    if shifts:
        for s in range(S):
            p.setPitchShift(shifts[s % len(shifts)], stream=s)
    return p


def _both(x, N, prepare=None, order=15, shifts=None, each_block=None, kernel=None):
    """x through the wave-specialised kernel and through the phase kernels: identical output, state and UB-site counters, no timeouts.
    each_block(p, b): called after every block of the wave-specialised run."""
    S = x.shape[0]
    runs = {}
    for ws in (True, False):
        p = _make(S, N, prepare, ws, order, shifts)
        name = p.pitch_kernel_name()
        assert name.startswith("vp_k_pitch_ws") == ws, name
        if ws and kernel:
            assert name == kernel, name
        y = np.empty((S, 2, x.shape[2]), np.float32)
        for b in range(x.shape[2] // N):
            y[:, :, b * N:(b + 1) * N] = p.process(np.ascontiguousarray(x[:, :, b * N:(b + 1) * N]))
            if ws and each_block:
                each_block(p, b)
        runs[ws] = (y, [_state_key(p, s) for s in range(S)], p.ub_counters())
        assert _timeouts(p) == [0, 0, 0]
        p.close()
    _assert_equal(runs[True][0], runs[False][0], "wave-specialised vs phase kernels")
    assert runs[True][1] == runs[False][1]
    assert runs[True][2] == runs[False][2]
    assert not np.isnan(runs[True][0]).any()
    assert np.abs(runs[True][0]).max() > 0.05
    return runs[True][0]


def _chunks_without_a_mark_of_their_own(st, C, cpf):
    """From a frame's tracker state: chunks k >= 1 in which no synthesis mark falls due (psola(): the mark's chunk is the first k with
    stMark - T < (k + 1) C) although an earlier mark's grain -- it ends at stMark + T / beta -- reaches into them."""
    if not st["anMarks"] or not st["stMarks"]:
        return 0
    T = st["period"] if st["pitch"] > 1 else st["prevVoicedPeriod"]
    if T <= 0 or st["beta"] <= 0:
        return 0
    due = [max(0, (m - T) // C) if m - T >= 0 else 0 for m in st["stMarks"]]
    n = 0
    for k in range(1, cpf):
        if k in due:
            continue
        if any(d < k and m + T / st["beta"] > k * C for m, d in zip(st["stMarks"], due)):
            n += 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_sparse_marks_on_every_chunk_grid(grid):
    """Low voices (periods up to 490 samples) and the edge corpus on chunk grids of 256, 512, 128 and 64 samples: where chunks are
    shorter than a period many chunks have no mark of their own and carry only earlier grains' tails -- the instances that must never
    end up half parked.  That such chunks occurred is asserted from the tracker state read after every block (on the grid of 512 a
    chunk is longer than every period here, so nothing is asserted there)."""
    prepare = GRIDS[grid]
    N = prepare[1] if prepare else 1024
    F, H = (prepare[2], prepare[3]) if prepare else (1024, 768)
    C = F - H
    x = _corpus(N * (30 if N >= 1024 else 96), fs=prepare[0] if prepare else FS)
    seen = [0]

    def look(p, b):
        for s in range(len(LOW_VOICES)):
            seen[0] += _chunks_without_a_mark_of_their_own(p.pitch_state(s), C, F // C)

    _both(x, N, prepare, each_block=look)
    print(f"{grid}: {seen[0]} chunks without a mark of their own in the low voices' frames")
    if C < FS / max(LOW_VOICES):
        assert seen[0] > 0, grid


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 256])
def test_grain_length_at_both_ends(N):
    """+12 / -12 semitones on alternate streams: beta = 2 leaves blocks without a grain inside a covered stretch, beta = 0.5 gives
    grains of four periods that spill far beyond their chunk."""
    x = _corpus(N * (30 if N == 1024 else 96))
    _both(x, N, shifts=(12.0, -12.0))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [100, 256, 512, 768, 1024])
def test_block_sizes(N):
    """launches without an instance (N = 100 between the chunk grid's points), with one, two, three and four chunk steps"""
    x = _corpus(N * (96 if N <= 256 else 48 if N <= 768 else 30))
    _both(x, N)


@pytest.mark.gpu
@pytest.mark.parametrize("order,kernel", [(2, "vp_k_pitch_ws"), (15, "vp_k_pitch_ws"), (16, "vp_k_pitch_ws_o24"), (17, "vp_k_pitch_ws_o24")])
def test_orders(order, kernel):
    """lpcPitch 2, 15 and 16 take the split path (16 in the _o24 build); 17 still launches the untouched history-matrix path of the
    same kernel as before"""
    x = _corpus(1024 * 30)
    _both(x, 1024, order=order, kernel=kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [2, 3, 8, 16])
def test_several_blocks_per_call(nb):
    """process_blocks_mono_device with 2, 3, 8 and 16 blocks per call (vp_k_pitch_ws_mb: the same body, the same parked segments per
    block) against block by block: identical output, state and counters."""
    import torch
    N, B = 1024, 32 if nb != 3 else 30
    x = _corpus(N * B)
    S = x.shape[0]
    xd = torch.from_numpy(np.ascontiguousarray(x[:, 0])).cuda().view(S, B, N).permute(1, 0, 2).contiguous()      # [B][S][N]
    ref_p = _make(S, N)
    assert ref_p.pitch_kernel_name() == "vp_k_pitch_ws"
    ref = torch.empty((B, S, 2, N), dtype=torch.float32, device="cuda")
    for b in range(B):
        ref_p.process_mono_device(xd[b], ref[b])
    ref_p.synchronize()
    p = _make(S, N)
    p.reserve_blocks(nb)
    out = torch.empty((B, S, 2, N), dtype=torch.float32, device="cuda")
    for b in range(0, B, nb):
        p.process_blocks_mono_device(xd[b:b + nb].contiguous(), out[b:b + nb])
    p.synchronize()
    got, want = out.cpu().numpy(), ref.cpu().numpy()
    _assert_equal(got, want, f"{nb} blocks per call vs block by block")
    assert [_state_key(p, s) for s in range(S)] == [_state_key(ref_p, s) for s in range(S)]
    assert p.ub_counters() == ref_p.ub_counters()
    assert _timeouts(p) == [0, 0, 0] and _timeouts(ref_p) == [0, 0, 0]
    assert not np.isnan(got).any() and np.abs(got).max() > 0.05
    p.close()
    ref_p.close()


@pytest.mark.gpu
def test_forced_timeout_is_an_error_not_a_hang():
    """With the poll limit at 1 the kernel's waits run out (the recursion's for its parked chunks among them): the call returns
    VP_ERR_TIMEOUT, it does not hang."""
    from vocoderproject_amd import VpError
    N, S = 1024, 6
    x = _streams(S, N * 8)
    p = _make(S, N)
    assert p.pitch_kernel_name() == "vp_k_pitch_ws"
    p.debug_set_spin_limit(1)
    codes = []
    for b in range(6):
        try:
            p.process(np.ascontiguousarray(x[:, :, b * N:(b + 1) * N]))
            codes.append(0)
        except VpError as e:
            codes.append(e.code)
    assert VP_ERR_TIMEOUT in codes, codes
    assert all(c == VP_ERR_TIMEOUT for c in codes[codes.index(VP_ERR_TIMEOUT):]), codes
    assert sum(_timeouts(p)) > 0
    p.close()


# ---- CPU: which segments park ---------------------------------------------------------------------------------------------------

SRC = r"""
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "vp_common.h"
int main()
{
    printf("[");
    bool first = true;
    for (int cpf : {2, 4, 8, 16}) {
        VpGeom g;
        memset(&g, 0, sizeof g);
        g.F = 1024; g.cpf = cpf; g.C = g.F / cpf; g.N = 1024; g.tauMax = 512; g.toKeep = 1024;
        g.eLen = g.toKeep + g.F + (cpf - 1) * g.C;
        for (int nChunk0 = 0; nChunk0 < cpf; nChunk0++)
            for (int nSteps = 1; nSteps <= 2 * cpf + 1; nSteps++) {
                VpWsSched sc;
                memset(&sc, 0xff, sizeof sc);
                if (!ws_build_sched(g, nChunk0, nSteps, sc)) continue;
                printf("%s{\"cpf\":%d,\"nChunk0\":%d,\"nSteps\":%d,\"nSeg\":%d,\"park\":[", first ? "" : ",", cpf, nChunk0, nSteps, sc.nSeg);
                first = false;
                for (int q = 0; q <= WS_MAXS; q++) printf("%s%d", q ? "," : "", sc.segPark[q]);
                printf("],\"segA\":[");
                for (int q = 0; q < sc.nSeg; q++) printf("%s%d", q ? "," : "", sc.segA[q]);
                printf("]}");
            }
    }
    printf("]\n");
    return 0;
}
"""


def _reference_segments(cpf, n_chunk0, n_steps):
    """PitchProcess::process's chunk loop: the block's instances as (is_start,), split into segments -- a Start opens one, and so does
    the frame in flight at the block's entry."""
    segs = []
    n_chunk = n_chunk0
    for t in range(n_steps):
        if n_chunk != 0:
            if not segs:
                segs.append([False])
            else:
                segs[-1].append(False)
        if n_chunk == cpf - 1:
            n_chunk = 0
        if n_chunk == 0:
            segs.append([True])
        n_chunk += 1
    return segs


def test_schedule_parks_the_segments_from_the_last_start_on(tmp_path):
    """The rule that shipped: the segments from the block's last Start on park -- that is the one segment that Start opens --, a block
    without a Start parks nothing; entries beyond the block's segments are zero; the parked segments are a suffix.  For the plugin's
    three block types (four steps, entered at chunk 1, 2, 3) and the other grids' schedules."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = tmp_path / "dump.cpp"
    src.write_text(SRC)
    exe = tmp_path / "dump"
    subprocess.run([gxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "vocoderproject_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    cases = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert len(cases) > 100
    types = {}
    for cse in cases:
        segs = _reference_segments(cse["cpf"], cse["nChunk0"], cse["nSteps"])
        assert cse["nSeg"] == len(segs), cse
        starts = [q for q, sg in enumerate(segs) if sg[0]]
        want = [1 if starts and q >= starts[-1] else 0 for q in range(len(segs))]
        assert cse["park"][:len(segs)] == want, (cse, want)
        assert all(v == 0 for v in cse["park"][len(segs):]), cse
        assert sum(want) == (1 if starts else 0) and (not starts or want[-1] == 1)        # one segment, the last
        if cse["cpf"] == 4 and cse["nSteps"] == 4:
            types[cse["nChunk0"]] = (cse["segA"], want)
    # the plugin's block types: [C1 C2 C3][S C1], [C2 C3][S C1 C2], [C3][S C1 C2 C3][S]
    assert types[1] == ([0, 3], [0, 1]) and types[2] == ([0, 2], [0, 1]) and types[3] == ([0, 1, 5], [0, 0, 1])
