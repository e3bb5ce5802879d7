"""CPU-side checks of the streaming pitch tracker (vp_pv_tracker_*): the definition tests/pv_track_stream_reference.py agrees with the
batch definition on every full window, does not depend on how blocks are grouped into calls, resets to a fresh tracker, has teeth (seeded
faults of it change its output on named cases), its case table holds what the GPU test needs (voiced decisions in numbers, a gap, a hold
that expires and one that does not, a glide), the loop closes through the NumPy streaming phase vocoder, and the library declares and
exports the new entry points and refuses bad arguments without a device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_stream_reference as PS  # noqa: E402
import pv_track_cases as TC  # noqa: E402
import pv_track_reference as R  # noqa: E402
import pv_track_stream_cases as SC  # noqa: E402
import pv_track_stream_reference as SR  # noqa: E402

SYMBOLS = ["vp_pv_tracker_create", "vp_pv_tracker_destroy", "vp_pv_tracker_debug_alloc_count", "vp_pv_tracker_reset", "vp_pv_tracker_set_follow",
           "vp_pv_tracker_process_blocks_device", "vp_pv_autotune_blocks_device"]


# ---- structure of the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.CASES, ids=SC.case_id)
def test_raw_decision_is_the_batch_trackers_on_the_last_window(c):
    """H = 0, g = 1 give the raw table: 0 / 1.0 below W, pv_track_reference.track on x[n_b - W, n_b) from there on."""
    x = SC.case_input(c)
    p, r = SR.run(x, c.fs, c.F, c.keys)
    rows, W = SC.rows(x), SC.window(c)
    for b in range(c.n_blocks):
        nb = (b + 1) * c.N
        if nb < W:
            assert b < SC.first_decision(c) and np.all(p[b] == 0) and np.all(r[b] == 1.0), (c.name, b)
            continue
        pb, rb = R.track(np.ascontiguousarray(rows[:, nb - W:nb]), c.fs, c.F, c.F, c.keys)
        assert pb.shape == (len(c.signals), 1)
        assert np.array_equal(p[b], pb[:, 0]) and np.array_equal(r[b], rb[:, 0]), (c.name, b)


@pytest.mark.parametrize("c", SC.CASES, ids=SC.case_id)
def test_grouping_blocks_into_calls_changes_nothing(c):
    p, r = SC.reference(c)
    x = SC.case_input(c)
    for name, groups in SC.groupings(c).items():
        assert sum(groups) == c.n_blocks and all(k >= 1 for k in groups), (c.name, name, groups)
        if name == "whole":
            continue
        pg, rg = SR.run(x, c.fs, c.F, c.keys, c.hold, c.glide, groups=groups)
        assert np.array_equal(p, pg) and np.array_equal(r, rg), (c.name, name)


def test_groupings_end_just_below_and_just_above_the_window():
    c = SC.BY_NAME["n64"]
    g, W = SC.groupings(c), SC.window(c)
    assert g["below-W"][0] * c.N < W <= (g["below-W"][0] + 1) * c.N and W <= g["above-W"][0] * c.N < W + c.N, (g, W)


def test_reset_equals_a_fresh_tracker():
    c = SC.BY_NAME["n256-glide"]
    x, S, cut = SC.case_input(c), len(c.signals), 17
    t = SR.StreamTracker(S, c.N, c.fs, c.F, c.hold, c.glide)
    t.process(x[:cut], c.keys)
    t.reset(2)                                                                     # one stream: the others carry on
    p1, r1 = t.process(x[cut:], c.keys)
    fresh_p, fresh_r = SR.run(x[cut:], c.fs, c.F, c.keys, c.hold, c.glide)
    whole_p, whole_r = SC.reference(c)
    for s in range(S):
        want = (fresh_p[:, s], fresh_r[:, s]) if s == 2 else (whole_p[cut:, s], whole_r[cut:, s])
        assert np.array_equal(p1[:, s], want[0]) and np.array_equal(r1[:, s], want[1]), s
    assert not np.array_equal(fresh_p[:, 2], whole_p[cut:, 2])                     # (the reset is visible: the window has to fill again)
    t.reset()                                                                      # every stream
    p2, r2 = t.process(x[cut:], c.keys)
    assert np.array_equal(p2, fresh_p) and np.array_equal(r2, fresh_r)


def test_domain_is_refused():
    SR.StreamTracker(1, 64, 44100.0, 1024)
    for kw in (dict(fs=7999.0), dict(fs=51201.0), dict(F=512), dict(N=0), dict(hold=-1), dict(hold=SR.HOLD_MAX + 1), dict(glide=0.0), dict(glide=1.5),
               dict(glide=float("nan"))):
        a = dict(S=1, N=64, fs=44100.0, F=1024, hold=0, glide=1.0)
        a.update(kw)
        with pytest.raises(AssertionError):
            SR.StreamTracker(**a)


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
def _runs(flags):
    """Lengths of the runs of True in a boolean sequence that have a False-free neighbour on both sides: (start, length)."""
    out, i, n = [], 0, len(flags)
    while i < n:
        if flags[i]:
            j = i
            while j < n and flags[j]:
                j += 1
            out.append((i, j - i))
            i = j
        else:
            i += 1
    return out


def test_case_table_holds_voiced_decisions_a_gap_both_holds_and_a_glide():
    total = voiced = 0
    for c in SC.CASES:
        p, r = SC.reference(c)
        assert p.shape == r.shape == (c.n_blocks, len(c.signals)) and p.dtype == np.int32 and r.dtype == np.float64
        assert np.all((r >= 0.5) & (r <= 2.0)), c.name
        total += p.size
        voiced += int((p > 0).sum())
    print(f"PV TRACK STREAM cases {len(SC.CASES)} decisions {total} voiced {voiced}")
    assert voiced * 3 >= total, (voiced, total)

    # a gap: voiced -> unvoiced -> voiced on the "gap" stream of the N = 256 cases
    c3, c1000, cg = SC.BY_NAME["n256-hold3"], SC.BY_NAME["n256-hold1000"], SC.BY_NAME["n256-glide"]
    s = c3.signals.index("gap")
    p, r3 = SC.reference(c3)
    fd = SC.first_decision(c3)
    gaps = [(b, n) for b, n in _runs((p[:, s] == 0).tolist()) if b > fd and b + n < c3.n_blocks]
    assert gaps and p[fd, s] > 0, (p[:, s], fd)
    b0, n = gaps[0]
    print(f"PV TRACK STREAM gap stream: unvoiced blocks {b0} .. {b0 + n - 1}, voiced before and after; periods {p[:, s].tolist()}")
    held = r3[b0 - 1, s]
    assert held != 1.0 and n > c3.hold + 1
    # the hold of 3 blocks keeps the last voiced ratio for three unvoiced blocks, then expires; the hold of 1000 does not
    assert np.all(r3[b0:b0 + c3.hold, s] == held) and np.all(r3[b0 + c3.hold:b0 + n, s] == 1.0), r3[b0 - 1:b0 + n + 1, s]
    r1000 = SC.reference(c1000)[1]
    assert np.array_equal(SC.reference(c1000)[0], p) and np.all(r1000[b0:b0 + n, s] == held)
    # the glide case moves half of the way per block: its ratios differ from the raw ones and approach them
    assert cg.glide == 0.5
    rg, raw = SC.reference(cg)[1], SR.run(SC.case_input(cg), cg.fs, cg.F, cg.keys)[1]
    tonal = cg.signals.index("sine_off")
    assert raw[fd, tonal] != 1.0 and rg[fd, tonal] == 1.0 + 0.5 * (raw[fd, tonal] - 1.0) and not np.array_equal(rg, raw)
    assert abs(rg[-1, tonal] - raw[-1, tonal]) < 1e-3 * abs(raw[-1, tonal] - 1.0)


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------
# the case on which each seeded fault must change the tables
TEETH = {"zero_prefill": "n64", "window_at_block_start": "n256-hold3", "age_ge_hold": "n256-hold3", "key_ignored": "n64"}


@pytest.mark.parametrize("mutant", sorted(TEETH))
def test_seeded_fault_changes_the_reference_on_its_named_case(mutant):
    c = SC.BY_NAME[TEETH[mutant]]
    p, r = SC.reference(c)
    pm, rm = SR.run(SC.case_input(c), c.fs, c.F, c.keys, c.hold, c.glide, mutant=mutant)
    print(f"PV TRACK STREAM mutant {mutant} on {c.name}: periods differ {int((p != pm).sum())}, ratios differ {int((r != rm).sum())}")
    if mutant in ("age_ge_hold", "key_ignored"):
        assert np.array_equal(p, pm)                                               # (neither the hold nor the key reaches the period)
    assert not np.array_equal(r, rm), f"the fault '{mutant}' changes nothing on {c.name}"


def test_glide_formula_at_one_is_a_different_function():
    """cur + 1.0 * (tgt - cur) is tgt whenever tgt - cur is exact, and Sterbenz's lemma makes it exact for cur / 2 <= tgt <= 2 cur: every
    ratio the tracker can produce (0.5 .. 2 around cur = 1).  So the fault shows on no tracked signal, and its named case feeds the follow
    stage a raw table directly: from cur = 1.0 to a raw ratio of 0.3 the difference is rounded and the sum comes back as 0.30000000000000004."""
    period, raw = np.array([1, 1, 1]), np.array([1.0, 0.3, 1.0])
    want, _ = SR.follow(period, raw, 0, 1.0)
    got, _ = SR.follow(period, raw, 0, 1.0, mutant="glide_formula_at_one")
    assert np.array_equal(want, raw) and not np.array_equal(got, want), (want, got)
    for c in SC.CASES:                                                             # ... and on the table it is the same function
        if c.glide == 1.0:
            pm, rm = SR.run(SC.case_input(c), c.fs, c.F, c.keys, c.hold, c.glide, mutant="glide_formula_at_one")
            assert np.array_equal(rm, SC.reference(c)[1]), c.name
            break


def test_follow_stage_matches_its_statement():
    period = np.array([0, 5, 0, 0, 0, 7, 0])
    raw = np.array([1.0, 1.25, 1.0, 1.0, 1.0, 0.75, 1.0])
    assert np.array_equal(SR.follow(period, raw, 0, 1.0)[0], raw)                  # H = 0, g = 1: the raw ratio
    assert SR.follow(period, raw, 2, 1.0)[0].tolist() == [1.0, 1.25, 1.25, 1.25, 1.0, 0.75, 0.75]
    assert SR.follow(period, raw, 2, 0.5)[0].tolist() == [1.0, 1.125, 1.1875, 1.21875, 1.109375, 0.9296875, 0.83984375]
    out, st = SR.follow(period[:3], raw[:3], 2, 0.5)
    out2, _ = SR.follow(period[3:], raw[3:], 2, 0.5, state=st)                      # the state carries across calls
    assert np.concatenate([out, out2]).tolist() == SR.follow(period, raw, 2, 0.5)[0].tolist()


# ---- closed loop without a GPU ------------------------------------------------------------------------------------------------------------
def test_closed_loop_through_the_numpy_streaming_phase_vocoder():
    """steady_input() -> streaming tracker (H = 0, g = 1, N = 256) -> PvStreamRef.process per block with that block's ratio -> batch tracker
    on the output: every period within one sample of fs / closestFreq ON THE STEADILY CORRECTED PART.  Its bounds: `first` is the output
    sample at which the first frame that took a tracked ratio ends -- that frame is computed in the first block b0 with n_b >= W, its last
    input sample is at most b0 N + N - 1, and it leaves `latency` samples later --; the part runs from first + F (every frame covering it
    took a tracked ratio) to F samples before the input's end.
    Figures: 227 Hz -> 189 against 189.20, in key 0 -> 201 against 200.45; 330.5 Hz -> 134 against 133.79; 205 Hz -> 212 / 213 against 212.37."""
    x, keys = TC.steady_input()
    fs, F, hop, N = TC.STEADY_FS, TC.STEADY_F, TC.STEADY_HOP, 256
    S, T = x.shape
    W = SR.window_len(fs, F)
    lat = PS.latency(N, hop, F)
    nb = -(-(T + lat) // N)
    xp = np.zeros((S, nb * N), np.float32)
    xp[:, :T] = x
    blocks = np.ascontiguousarray(xp.reshape(S, nb, N).transpose(1, 0, 2))
    n_in = T // N                                                                  # blocks that hold input only (the padding is silence)
    p, r = SR.run(blocks[:n_in], fs, F, keys)
    b0 = -(-W // N) - 1
    assert np.all(p[b0:] > 0) and np.all(r[:b0] == 1.0)
    ratios = np.ones((nb, S))
    ratios[:n_in] = r
    ratios[n_in:] = r[-1]
    for s, target in enumerate(TC.steady_targets()):
        pv = PS.PvStreamRef(N, hop, F)
        y = np.concatenate([pv.process(blocks[b, s].astype(np.float64), ratio=float(ratios[b, s])) for b in range(nb)])[lat:lat + T]
        first = (b0 + 1) * N                                                       # (aligned with the input: the latency is dropped above)
        lo, hi = first + F, T - F
        assert hi - lo >= F + R.tau_max(fs) + 4 * hop, (lo, hi)
        p2, _ = R.track(np.asarray(y[lo:hi], np.float32)[None], fs, F, hop, keys[s])
        print(f"PV TRACK STREAM closed loop {TC.STEADY[s]}: samples [{lo}, {hi}) periods {sorted(set(p2[0].tolist()))} target {target:.2f}")
        assert np.all(np.abs(p2[0] - target) <= 1.0), (s, p2[0], target)


# ---- library surface ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    return C.CDLL(build.build())


def test_new_symbols_are_declared_and_exported(lib):
    txt = open(os.path.join(ROOT, "include", "vp_amd.h")).read()
    assert "#define VP_ABI_VERSION 3" in txt and lib.vp_abi_version() == 3
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} not declared in include/vp_amd.h"
        assert hasattr(lib, s), f"{s} not exported"


def test_bad_arguments_are_errors_before_any_device_is_needed(lib):
    vp, one = C.c_void_p, C.c_void_p(8)
    lib.vp_pv_tracker_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(vp)]
    lib.vp_pv_tracker_process_blocks_device.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp]
    lib.vp_pv_autotune_blocks_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]
    lib.vp_pv_tracker_set_follow.argtypes = [vp, C.c_int, C.c_double]
    lib.vp_pv_tracker_debug_alloc_count.restype = C.c_long
    h = vp()
    assert lib.vp_pv_tracker_create(0, 4, 256, 1024, 44100.0, None) == -1
    for fs in (7999.0, 51201.0, float("nan")):
        assert lib.vp_pv_tracker_create(0, 4, 256, 1024, fs, C.byref(h)) == -1 and not h.value
    for F in (512, 1000, 4096):
        assert lib.vp_pv_tracker_create(0, 4, 256, F, 44100.0, C.byref(h)) == -4 and not h.value          # VP_ERR_GEOMETRY
    for S, N in ((0, 256), (4, 0), (-1, 256)):
        assert lib.vp_pv_tracker_create(0, S, N, 1024, 44100.0, C.byref(h)) == -1 and not h.value
    assert lib.vp_pv_tracker_process_blocks_device(None, one, None, one, one, 1, None) == -1
    assert lib.vp_pv_autotune_blocks_device(None, None, one, one, None, one, one, 1, None) == -1
    assert lib.vp_pv_tracker_reset(None, 0) == -1 and lib.vp_pv_tracker_set_follow(None, 0, 1.0) == -1 and lib.vp_pv_tracker_destroy(None) == -1
    assert lib.vp_pv_tracker_debug_alloc_count(None) == -1


def test_cpp_wrappers_compile_and_link(tmp_path):
    """include/vp_amd.hpp: vp::StreamingPitchTracker and vp::StreamingPitchShifter::autotuneBlocks are valid C++17 and resolve against the
    built library; run without a GPU they throw vp::Error, with one the null pointers are refused before the device is touched."""
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
    try {
        vp::StreamingPitchTracker t(0, 4, 256, 44100.0);
        vp::StreamingPitchShifter p(0, 4, 256);
        t.setFollow(3, 0.5);
        t.reset();
        try {
            p.autotuneBlocks(t, nullptr, nullptr, nullptr, nullptr, nullptr, 1);
        } catch (const vp::Error &e) {
            return e.code == VP_ERR_INVALID_ARG ? 0 : 1;
        }
        return 2;
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


def test_build_lists_the_shared_body_as_a_dependency():
    """The two tracker kernels include one body: it is a build dependency and part of vp_track.hip's object hash, and the translation
    unit keeps the default flags (-ffp-contract=off: the follow stage's product and add stay separate)."""
    from vocoderproject_amd import build
    assert "vp_track_body.inc" in build.DEPS
    assert os.path.join(build.CSRC, "vp_track_body.inc") in build.deps_of("vp_track.hip")
    src = open(os.path.join(ROOT, "vocoderproject_amd", "build.py")).read()
    assert re.search(r'"vp_track\.hip"\), os\.path\.join\(tmp, "track\.o"\), \[\]\)', src)
    hip = open(os.path.join(ROOT, "vocoderproject_amd", "csrc", "vp_track.hip")).read()
    assert hip.count('#include "vp_track_body.inc"') == 2 and "vp_k_yin_track_stream" in hip and "vp_k_track_follow" in hip
