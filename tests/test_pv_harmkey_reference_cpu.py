"""CPU-side checks of the key-aware voices (no GPU): the definitions tests/pv_harmkey_reference.py and
tests/pv_harmkey_stream_reference.py -- the harmony tables, degree 0 against the tracker, the teeth of every mutant, the musical check, the
streaming form's independence of the call grouping and its equality with the mono follow stage --, the conditioning of
tests/pv_harmkey_cases.py, the host layers of the library (null handles, the C++ mirror, the Python front ends' checks before any
launch), the kernels' budgets from the built code object, and the offline flow and its command line."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import oracle_py as O  # noqa: E402
import pv_harmkey_cases as K  # noqa: E402
import pv_harmkey_reference as HR  # noqa: E402
import pv_harmkey_stream_reference as HSR  # noqa: E402
import pv_track_reference as R  # noqa: E402
import pv_track_stream_reference as SR  # noqa: E402


# ---- 1. the harmony tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", range(13))
def test_the_tracker_s_table_is_a_slice_of_the_harmony_table_with_twelve_steps_above_it(key):
    f, n = O.notes_build(key, 100.0, 800.0)
    H, hN = O.notes_build(key, 25.0, 3200.0)
    off = HR.harmony_table(key)[2]
    assert np.array_equal(H[off:off + n + 1].view(np.uint64), f[:n + 1].view(np.uint64))      # the popped slot too, bit for bit
    assert np.all(np.diff(H[:hN + 1]) > 0) and hN + 1 <= HR.STRIDE
    if key == 12:
        assert (n, hN, off, hN - 1 - (off + n)) == (36, 70, 10, 23)
    else:
        assert n == 21 and 41 <= hN <= 47 and 6 <= off <= 12 and hN - 1 - (off + n) == 13
    assert off + n + HR.MAX_DEGREE <= hN - 1                                                  # the upper bound never binds


# ---- 2. the batch definition ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_cases_reach_what_they_are_there_for_and_degree_zero_is_the_tracker_s_ratio(c):
    assert all(K.holds(c, s) for s in range(K.S)), [K.holds(c, s) for s in range(K.S)]
    x = K.batch_input(c)
    V = len(c.degrees[0])
    p, r = HR.track_harmony(x, c.fs, c.F, c.hop, np.zeros((K.S, V), np.int32), c.keys, None)
    tp, tr = R.track(x, c.fs, c.F, c.hop, c.keys)
    assert np.array_equal(p, tp) and np.array_equal(K.reference(c)[0], tp)
    for v in range(V):
        assert np.array_equal(r[:, v].view(np.uint64), tr.view(np.uint64))
    assert K.reference(c)[1].shape == (K.S, V, R.n_frames(c.T, c.F, c.hop)) and np.all(np.isfinite(K.reference(c)[1]))


def test_the_batch_shapes_are_the_ones_the_kernel_s_tail_guard_needs():
    c = K.BY_NAME["steady-v3"]
    assert R.n_frames(c.T, c.F, c.hop) == 13 and (K.S * 13) % 4 != 0
    assert R.tau_max(K.BY_NAME["fs8000"].fs) == 80 and K.BY_NAME["f2048"].F == 2048


def test_every_mutant_of_the_batch_definition_differs_on_a_named_case():
    killed = set()
    for c in K.CASES:
        for m in c.kills:
            p, r = HR.track_harmony(K.batch_input(c), c.fs, c.F, c.hop, K.degrees_of(c), c.keys, K.unvoiced_of(c), mutant=m)
            assert np.array_equal(p, K.reference(c)[0])
            assert not np.array_equal(r.view(np.uint64), K.reference(c)[1].view(np.uint64)), (c.name, m)
            killed.add(m)
    assert killed == set(HR.MUTANTS)


def test_the_lower_clamp_and_the_popped_slot_are_where_the_cases_say():
    H, hN, off = HR.harmony_table(11)
    c, idx = HR.chosen_index(44100.0 / K.P_LOW, 11)
    assert off + c - 7 == -1                                                                   # 104 Hz in key 11, seven degrees down
    assert HR.voice_ratios(K.P_LOW, 44100.0, 11, [-7])[0] == H[0] / (44100.0 / K.P_LOW)
    c12 = HR.chosen_index(44100.0 / K.P_LOW, 12)[0]
    assert HR.harmony_table(12)[2] + c12 - 12 < 0
    n = R.notes_table(0)[1]
    assert HR.chosen_index(44100.0 / 55, 0) == (n, n)                                           # the popped slot, returned


def test_a_sharp_a3_gets_the_notes_of_its_key():
    fs, pitch = 44100.0, 44100.0 / K.P_A3
    got = HR.voice_ratios(K.P_A3, fs, 0, [0, 2, 4, -3]) * pitch
    for g, want in zip(got, (220.0, 277.18, 329.63, 164.81)):
        assert abs(g - want) < 0.01, (g, want)
    H, _, off = HR.harmony_table(12)
    c = HR.chosen_index(pitch, 12)[0]
    got = HR.voice_ratios(K.P_A3, fs, 12, [0, 4, 7])
    assert [float(v) for v in got] == [float(H[off + c + d]) / pitch for d in (0, 4, 7)] and abs(float(H[off + c]) - 220.0) < 0.01
    assert abs(K.chord_notes()[0] - 277.18) < 0.01 and abs(K.chord_notes()[1] - 329.63) < 0.01


def test_unvoiced_values_and_the_nominal_intervals():
    assert HR.voice_ratios(0, 44100.0, 0, [1, 2, 3], None).tolist() == [1.0, 1.0, 1.0]
    assert HR.voice_ratios(0, 44100.0, 0, [1, 2, 3], [float("nan"), float("inf"), 0.75]).tolist() == [1.0, 1.0, 0.75]
    u = HR.nominal_unvoiced([0, 2, 4, -3], [0, 12, 99], 3)
    assert u[0].tolist() == [1.0, 2.0 ** (3 / 12), 2.0 ** (7 / 12), 2.0 ** (-5 / 12)]
    assert u[1].tolist() == u[2].tolist() == [1.0, 2.0 ** (2 / 12), 2.0 ** (4 / 12), 2.0 ** (-3 / 12)]


def test_the_chord_s_reference_distance_is_the_recorded_one():
    got, dist = K.chord_reference_distance()
    print(f"PVHARMKEY reference chord: maxima {got[0]:.3f}, {got[1]:.3f} Hz, distance {dist:.4f} Hz")
    assert abs(dist - K.CHORD_REF_DISTANCE_HZ) < 1e-3
    with open(os.path.join(ROOT, "profiles", "pv_harmkey_quality.txt")) as f:
        assert "CHORD_REF_DISTANCE_HZ = %.4f" % K.CHORD_REF_DISTANCE_HZ in f.read()
    assert K.chord_tolerance() == K.CHORD_BIN_HZ


# ---- 3. the streaming definition ---------------------------------------------------------------------------------------------------------------------
def test_how_blocks_are_grouped_into_calls_changes_nothing():
    """Every composition of 24 blocks would be 2^23 runs.  The definition carries its whole state from call to call (the raw tracker's
    history and count, tgt, cur, age), so a call boundary can only matter through what one boundary does to that state: every single
    boundary position is taken (all 23 splits in two), with one call, 24 calls of one and a seeded dozen of mixed groupings beside
    them."""
    x = K.stream_input()
    deg, unv = np.asarray(K.STREAM_DEGREES, np.int32), np.asarray(K.STREAM_UNVOICED)
    for hold, glide in K.STREAM_FOLLOW:
        want_p, want_r = K.stream_reference(hold, glide)
        for groups in K.all_partitions(K.STREAM_BLOCKS) + list(K.STREAM_GROUPINGS.values()):
            p, r = HSR.run(x, K.STREAM_FS, K.STREAM_F, deg, K.STREAM_KEYS, unv, hold, glide, groups=groups)
            assert np.array_equal(p, want_p) and np.array_equal(r.view(np.uint64), want_r.view(np.uint64)), groups


@pytest.mark.parametrize("glide", [1.0, 0.5])
@pytest.mark.parametrize("hold", [0, 3])
def test_degree_zero_and_unvoiced_one_is_the_mono_follow_stage(hold, glide):
    x = K.stream_input()
    p, r = HSR.run(x, K.STREAM_FS, K.STREAM_F, np.zeros((K.S, 3), np.int32), K.STREAM_KEYS, np.ones((K.S, 3)), hold, glide, groups=[5, 19])
    mp, mr = SR.run(x, K.STREAM_FS, K.STREAM_F, K.STREAM_KEYS, hold, glide)
    assert np.array_equal(p, mp) and np.any(p > 0) and np.any(p[K.FIRST_DECISION:] == 0)
    assert np.all(p[:K.FIRST_DECISION] == 0) and np.all(p[K.FIRST_DECISION, [0, 2]] > 0)
    for v in range(3):
        assert np.array_equal(r[:, :, v].view(np.uint64), mr.view(np.uint64))


def test_every_mutant_of_the_streaming_definition_differs():
    x = K.stream_input()
    deg, unv = np.asarray(K.STREAM_DEGREES, np.int32), np.asarray(K.STREAM_UNVOICED)
    want_p, want_r = K.stream_reference(3, 0.5)
    # shared_target: on the whole slab; age_per_call: a call boundary inside stream 1's unvoiced run, before the hold has run out
    silent = int(np.flatnonzero(want_p[K.FIRST_DECISION:, 1] == 0)[0]) + K.FIRST_DECISION
    for m, groups in (("shared_target", [24]), ("age_per_call", [silent + 2, 24 - silent - 2])):
        p, r = HSR.run(x, K.STREAM_FS, K.STREAM_F, deg, K.STREAM_KEYS, unv, 3, 0.5, groups=groups, mutant=m)
        assert np.array_equal(p, want_p) and not np.array_equal(r.view(np.uint64), want_r.view(np.uint64)), m
    assert set(HSR.MUTANTS) == {"shared_target", "age_per_call"}


# ---- 4. the library's host layers, without a device ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    return C.CDLL(build.build())


def test_null_handles_answer_before_a_device_is_looked_for(lib):
    """Without a device no handle exists, so what can be asked here is the null handle with every other argument bad in turn: the voice
    count (0 and 5), a null degree table, both outputs null.  The same arguments on real handles, and the 2048-point handle on
    vp_stft_harmonize_key, are tests/test_gpu_pv_harmkey.py's."""
    vp = C.c_void_p
    lib.vp_stft_track_harmony.argtypes = [vp, vp, C.c_double, vp, C.c_int, vp, vp, vp, vp, vp]
    lib.vp_stft_harmonize_key.argtypes = [vp, vp, vp, C.c_double, vp, C.c_int] + [vp] * 7
    lib.vp_pv_tracker_process_blocks_voices_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.vp_hz_autoharm_blocks_device.argtypes = [vp, vp, vp, vp] + [vp] * 7 + [C.c_int, vp]
    for V, deg, per, rat in ((3, 8, 8, 8), (0, 8, 8, 8), (5, 8, 8, 8), (3, None, 8, 8), (3, 8, None, None)):
        assert lib.vp_stft_track_harmony(None, 8, 44100.0, None, V, deg, None, per, rat, None) == -1
        assert lib.vp_stft_harmonize_key(None, 8, 8, 44100.0, None, V, deg, None, None, None, per, rat, None) == -1
        assert lib.vp_pv_tracker_process_blocks_voices_device(None, 8, None, V, deg, None, per, rat, 1, None) == -1
        assert lib.vp_hz_autoharm_blocks_device(None, None, 8, 8, None, deg, None, None, None, per, rat, 1, None) == -1
    lib.vp_abi_version.restype = C.c_int
    assert lib.vp_abi_version() == 3


def test_cpp_mirror_compiles_with_werror_and_links(tmp_path):
    import shutil
    import subprocess
    from vocoderproject_amd import build
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    so = build.build()
    src = tmp_path / "t.cpp"
    src.write_text(r"""
#include "vp_amd.hpp"
#include <cstdio>
int main() {
    if (vp_stft_track_harmony(nullptr, nullptr, 44100.0, nullptr, 3, nullptr, nullptr, nullptr, nullptr, nullptr) != VP_ERR_INVALID_ARG) return 2;
    if (vp_stft_harmonize_key(nullptr, nullptr, nullptr, 44100.0, nullptr, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != VP_ERR_INVALID_ARG) return 3;
    try {
        vp::StreamingHarmonizer hz(0, 4, 256, 3, 128);
        vp::StreamingPitchTracker trk(0, 4, 256, 44100.0);
        try { trk.processBlocksVoices(nullptr, nullptr, 3, nullptr, nullptr, nullptr, nullptr, 1); return 4; } catch (const vp::Error &e) { if (e.code != VP_ERR_INVALID_ARG) return 5; }
        try { hz.autoharmBlocks(trk, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1); return 6; }
        catch (const vp::Error &e) { if (e.code != VP_ERR_INVALID_ARG) return 7; }
        return 0;
    } catch (const vp::Error &e) {
        std::printf("vp::Error %d\n", e.code);
        return e.code == VP_ERR_NO_DEVICE ? 42 : 1;
    }
}
""")
    exe = tmp_path / "t"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), so,
                           "-Wl,-rpath," + os.path.dirname(so)])
    import torch
    assert subprocess.call([str(exe)]) == (0 if torch.cuda.is_available() else 42)


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
    from vocoderproject_amd import HarmonizerStream, StftRoundTrip, StreamingPitchTracker
    st = StftRoundTrip.__new__(StftRoundTrip)
    st.L, st.h, st.S, st.T, st.F, st.hop, st.n_frames, st._curve_tables = _NoLaunch(), None, 3, 4096, 1024, 256, 13, {}
    ok = lambda p, shape=(3, 4096): _Tensor(shape, ptr=p)     # noqa: E731
    bad = [lambda: st.harmonize(ok(1), ok(2), degrees=[2, 4], semitones=[4.0], sample_rate=44100.0),          # two of the three
           lambda: st.harmonize(ok(1), ok(2), degrees=[2, 4], d_ratio=_Tensor((3, 2, 13), torch.float64), sample_rate=44100.0),
           lambda: st.harmonize(ok(1), ok(2), degrees=[2, 4]),                                                 # no sample rate
           lambda: st.harmonize(ok(1), ok(2), semitones=[4.0], keys=0),                                        # keys without degrees
           lambda: st.harmonize(ok(1), ok(2), degrees=[1, 2, 3, 4, 5], sample_rate=44100.0),
           lambda: st.harmonize(ok(1), ok(2), degrees=[], sample_rate=44100.0),
           lambda: st.harmonize(ok(1), ok(2), degrees=[2.5], sample_rate=44100.0),
           lambda: st.harmonize(ok(1), ok(2), degrees=np.zeros((2, 2), np.int32), sample_rate=44100.0),
           lambda: st.harmonize(ok(1), ok(2), degrees=[2, 4], sample_rate=44100.0, unvoiced=[1.0]),
           lambda: st.harmonize(ok(1), ok(2, (3, 4097)), degrees=[2, 4], sample_rate=44100.0),
           lambda: st.track_harmony(_Tensor((3, 4096), torch.float64), 44100.0, [2, 4]),
           lambda: st.track_harmony(ok(1, (3, 4097)), 44100.0, [2, 4]),
           lambda: st.track_harmony(ok(1), 44100.0, [1, 2, 3, 4, 5]),
           lambda: st.track_harmony(ok(1), 44100.0, np.zeros((4, 2), np.int32)),
           lambda: st.track_harmony(ok(1), 44100.0, [2, 4], unvoiced=np.ones((3, 3))),
           lambda: st.track_harmony(ok(1), 44100.0, _Tensor((3, 2), torch.int64))]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert i >= 0
    trk = StreamingPitchTracker.__new__(StreamingPitchTracker)
    trk.L, trk.h, trk.S, trk.N, trk.F, trk.fs, trk.device = _NoLaunch(), None, 3, 256, 1024, 44100.0, 0
    blk = lambda p, shape=(2, 3, 256): _Tensor(shape, ptr=p)  # noqa: E731
    bad = [lambda: trk.process_voices_device(blk(1), [2, 4], n_blocks=0),
           lambda: trk.process_voices_device(blk(1, (3, 256)), [2, 4], n_blocks=2),
           lambda: trk.process_voices_device(blk(1), [1, 2, 3, 4, 5], n_blocks=2),
           lambda: trk.process_voices_device(blk(1), [2, 4], n_blocks=2, unvoiced=[1.0, 1.0, 1.0]),
           lambda: trk.process_voices_device(_Tensor((2, 3, 256), torch.float16), [2, 4], n_blocks=2)]
    hz = HarmonizerStream.__new__(HarmonizerStream)
    hz.L, hz.h, hz.S, hz.N, hz.V, hz.F, hz.hop, hz.device, hz._tables = _NoLaunch(), None, 3, 256, 2, 1024, 256, 0, {}
    other = StreamingPitchTracker.__new__(StreamingPitchTracker)
    other.L, other.h, other.S, other.N = _NoLaunch(), None, 4, 256
    bad += [lambda: hz.autoharm_device(trk, blk(1), blk(2), [2, 4], n_blocks=0),
            lambda: hz.autoharm_device(trk, blk(1), blk(2), [2, 4, 6], n_blocks=2),                            # the handle has two voices
            lambda: hz.autoharm_device(other, blk(1), blk(2), [2, 4], n_blocks=2),
            lambda: hz.autoharm_device(trk, blk(1), _Tensor((2, 3, 256), torch.float16), [2, 4], n_blocks=2),
            lambda: hz.run(np.zeros((3, 700), np.float32)),
            lambda: hz.run(np.zeros((3, 700), np.float32), semitones=[4.0, 7.0], degrees=[2, 4], autoharm=trk),
            lambda: hz.run(np.zeros((3, 700), np.float32), degrees=[2, 4])]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    hz.h = st.h = trk.h = other.h = None                       # (nothing to destroy)


# ---- 5. the kernels' budgets, from the built code object ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resources():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    return kernel_resources.kernel_resources(build.build())


@pytest.mark.parametrize("kernel", ["vp_k_yin_track_voices", "vp_k_yin_track_voices_stream"])
def test_the_new_yin_kernels_are_within_the_tracker_s_budget(resources, kernel):
    r = resources[kernel]
    print(f"PVHARMKEY resources {kernel} {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["agpr"] == 0 and r["vgpr"] <= 128 and r["lds"] == 0, r


def test_the_existing_kernels_keep_the_parent_commit_s_figures(resources):
    import test_pv_track_resources_cpu as T
    rows = {}
    with open(os.path.join(ROOT, "profiles", "pv_harmkey_resources.txt")) as f:
        for line in f:
            m = re.match(r"^(vp_k_\S+(?: \S+>)?)\s+((?:\d+\s+){5}|(?:-\s+){5})((?:\d+\s*){5})$", line)
            if m:
                rows[m.group(1)] = (None if "-" in m.group(2) else tuple(int(v) for v in m.group(2).split()), tuple(int(v) for v in m.group(3).split()))
    want = ["vp_k_yin_track", "vp_k_yin_track_stream", "vp_k_track_follow", "vp_k_track_reset"] + sorted(T.NEIGHBOURS)
    assert set(want) <= set(rows), sorted(set(want) - set(rows))
    for k in want:
        r = resources[k]
        assert rows[k][0] == rows[k][1] == (r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"]), (k, rows[k], r)
    for k in sorted(T.NEIGHBOURS):
        assert rows[k][0] == T.NEIGHBOURS[k]
    for k in ("vp_k_yin_track_voices", "vp_k_yin_track_voices_stream", "vp_k_track_follow_voices", "vp_k_track_reset_voices"):
        r = resources[k]
        assert rows[k][0] is None and rows[k][1] == (r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"]), (k, rows[k], r)


def test_the_new_sources_are_part_of_the_build():
    from vocoderproject_amd import build
    assert "vp_track_voices.inc" in build.DEPS and "vp_track_body.inc" in build.DEPS


# ---- 6. the offline flow and its command line ----------------------------------------------------------------------------------------------------------
class _Definition:
    """The flow's processor: the definitions in place of the GPU."""

    def __init__(self, hop=256, stream_N=None, hold=0, glide=1.0):
        self.hop, self.N, self.hold, self.glide, self.seen = hop, stream_N, hold, glide, []

    def run(self, x, fs, keys, degrees, gains, dry):
        import pv_harm_reference as PH
        self.seen.append((x.shape, fs, list(keys), degrees.copy(), gains.copy(), list(dry)))
        if self.N is None:
            p, r = HR.track_harmony(x, fs, 1024, self.hop, degrees, keys, HR.nominal_unvoiced(degrees, keys, x.shape[0]))
            y = PH.harmonize_batch(x, np.clip(r, 0.5, 2.0), gains, dry, 1024, self.hop)
            return y.astype(np.float32), p, r
        S, nb = x.shape[0], x.shape[1] // self.N
        blocks = np.ascontiguousarray(x.reshape(S, nb, self.N).transpose(1, 0, 2))
        p, r = HSR.run(blocks, fs, 1024, degrees, keys, HR.nominal_unvoiced(degrees, keys, S), self.hold, self.glide)
        return x.copy(), p, r                                  # (the harmonizer half is tests/test_offline_pvharm_cpu.py's; here: the tables)


def _voice(n, period, fs=44100.0):
    return (0.8 * np.sin(2.0 * np.pi * np.arange(n) / period + 0.3)).astype(np.float32)


def test_pv_harmonize_key_runs_end_to_end_on_the_definitions():
    from vocoderproject_amd import offline
    voices = [_voice(6000, K.P_A3), _voice(5000, 150)]
    p = _Definition()
    outs, period, ratio = offline.pv_harmonize_key(voices, 44100.0, [2, 4], key=0, gains=[1.0, 1.0], dry=0.0, processor=p, with_track=True)
    (shape, fs, keys, deg, gains, dry), = p.seen
    assert shape == (2, offline.tune_length(6000, 44100.0, 1024, 256)) and keys == [0, 0] and deg.tolist() == [[2, 4], [2, 4]] and dry == [0.0, 0.0]
    assert [o.shape for o in outs] == [(2, 6000), (2, 5000)] and period.shape[0] == 2 and ratio.shape[:2] == (2, 2)
    voiced = period[0] == K.P_A3
    assert np.count_nonzero(voiced) >= 10
    want = np.asarray(K.chord_notes()) / (44100.0 / K.P_A3)
    assert np.array_equal(ratio[0][:, voiced], np.repeat(want[:, None], np.count_nonzero(voiced), axis=1))
    assert np.all(np.isfinite(outs[0])) and np.abs(outs[0]).max() > 0.1
    # streamed: the tables per block
    p = _Definition(stream_N=256, hold=2, glide=0.5)
    outs, period, ratio = offline.pv_harmonize_key(voices, 44100.0, (2, 4, -3), key=[0, 12], stream=True, N=256, hold=2, glide=0.5, processor=p, with_track=True)
    T, lat = offline.stream_tune_length(6000, 256, 256)
    assert p.seen[0][0] == (2, T) and p.seen[0][2] == [0, 12] and period.shape == (T // 256, 2) and ratio.shape == (T // 256, 2, 3)
    assert [o.shape for o in outs] == [(2, 6000), (2, 5000)]


def test_pv_harmonize_key_refuses():
    from vocoderproject_amd import offline
    voices = [_voice(3000, 199)]
    for bad, msg in ((dict(degrees=[]), "degrees: 1 to 4 integers expected"), (dict(degrees=[1, 2, 3, 4, 5]), "degrees: 1 to 4 integers expected"),
                     (dict(degrees=[2.5]), "degrees: 1 to 4 integers expected"), (dict(degrees=[13]), r"degrees: steps within \+-12 expected"),
                     (dict(degrees=[2], gains=[1, 1]), "gains: one gain per voice expected"), (dict(degrees=[2], dry=5.0), "dry: values within"),
                     (dict(degrees=[2], key=13), "key: 0..12 expected"), (dict(degrees=[2], fs=7000.0), "sample rates from 8000"),
                     (dict(degrees=[2], stream=True, glide=0.0), "harmonize --stream")):
        kw = dict(fs=44100.0)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            offline.pv_harmonize_key(voices, kw.pop("fs"), kw.pop("degrees"), processor=_Definition(), **kw)


def test_command_line(tmp_path, monkeypatch):
    from vocoderproject_amd import offline
    fs = 44100
    a = str(tmp_path / "a.wav")
    offline.write_wav(a, fs, 0.5 * _voice(6000, K.P_A3))
    out = str(tmp_path / "o")
    seen = []
    real = offline.pv_harmonize_key

    def through_the_definition(voices, fs_, degrees, **kw):
        seen.append((degrees, dict(kw)))
        kw["processor"] = _Definition(stream_N=kw["N"] if kw["stream"] else None, hold=kw["hold"], glide=kw["glide"])
        return real(voices, fs_, degrees, **kw)
    monkeypatch.setattr(offline, "pv_harmonize_key", through_the_definition)
    assert offline.main(["harmonize", a, "--degrees", "2,4,-3", "--key", "0", "--dry", "0", "--track-csv", "--out-dir", out]) == 0
    dg, kw = seen.pop()
    assert dg == [2, 4, -3] and kw == dict(key=0, gains=None, dry=0.0, hop=256, N=1024, stream=False, hold=0, glide=1.0, device=0, with_track=True)
    fs_got, y = offline.read_wav(os.path.join(out, "a_harmonize.wav"))
    assert fs_got == fs and y.shape == (2, 6000) and np.abs(y).max() > 0.05
    for v in range(3):
        with open(os.path.join(out, f"a_harmonize_v{v}.csv")) as f:
            rows = f.read().splitlines()
        assert rows[0] == "time_s,period,semitones" and len(rows) > 10 and rows[3].split(",")[1] == str(K.P_A3)
    assert abs(float(rows[3].split(",")[2]) - 12.0 * np.log2(164.81 / (44100.0 / K.P_A3))) < 0.01          # three degrees below A3 in C major: E3
    assert offline.main(["harmonize", a, "--degrees=-3,2", "--key", "5", "--stream", "--block", "256", "--hold", "8", "--glide", "0.5", "--gains", "1,0.7",
                         "--out-dir", out]) == 0
    dg, kw = seen.pop()
    assert dg == [-3, 2] and kw == dict(key=5, gains=[1.0, 0.7], dry=1.0, hop=256, N=256, stream=True, hold=8, glide=0.5, device=0, with_track=True)
    with pytest.raises(SystemExit, match="--voices and --degrees exclude each other"):
        offline.main(["harmonize", a, "--degrees", "2,4", "--voices", "4,7", "--out-dir", out])
    with pytest.raises(SystemExit, match="--degrees: comma-separated integers expected"):
        offline.main(["harmonize", a, "--degrees", "2,x", "--out-dir", out])
    with pytest.raises(SystemExit, match="degrees: steps within"):
        offline.main(["harmonize", a, "--degrees", "13", "--out-dir", out])
    for bad, flag in ((["--locked"], "--locked"), (["--shift", "3"], "--shift"), (["--glide", "0.5"], "--glide"), (["--formant"], "--formant")):
        with pytest.raises(SystemExit) as e:
            offline.main(["harmonize", a, "--degrees", "2"] + bad + ["--out-dir", out])
        assert str(e.value).startswith(f"{flag}: harmonize --degrees does not take it"), e.value
    with pytest.raises(SystemExit, match="--degrees: harmonize takes it"):
        offline.main(["pvtune", a, "--degrees", "2", "--out-dir", out])
    seen.clear()
