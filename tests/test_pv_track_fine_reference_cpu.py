"""The fine pitch tracker on the CPU: the definition tests/pv_track_fine_reference.py (every mutant differs on a named case, the rule
never moves a period by more than half a sample, the note is looked up on the refined pitch), the quality condition that motivates it,
the branch coverage of the device cases (tests/pv_track_fine_cases.py, which gates tests/test_gpu_pv_track_fine.py), the streaming
definition, the new kernels' budgets from the built code object, the library's host layers without a device, and the offline flows with
the definitions in place of the GPU."""
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
import pv_track_fine_cases as FC  # noqa: E402
import pv_track_fine_reference as FR  # noqa: E402
import pv_track_fine_stream_reference as FSR  # noqa: E402
import pv_track_reference as R  # noqa: E402
import pv_track_stream_reference as SR  # noqa: E402

FS, F, HOP = 44100.0, 1024, 256
NEW_KERNELS = ("vp_k_yin_track_fine", "vp_k_yin_track_stream_fine", "vp_k_yin_track_voices_fine", "vp_k_yin_track_voices_stream_fine")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. the definition and its mutants ----------------------------------------------------------------------------------------------------------
def _differs(x, fs, keys, mutant, F_=F, hop=HOP):
    a, b = FR.track_fine(x, fs, F_, hop, keys), FR.track_fine(x, fs, F_, hop, keys, mutant=mutant)
    return not all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a[1:], b[1:]))


def test_every_mutant_differs_on_a_named_case():
    near = FC.batch_input(FC.BY_NAME["near-fs44100-F1024-clamp-3"])              # periods tau0 + 0.1, 0.3, 0.5: refined away from tau0
    left = FC.batch_input(FC.BY_NAME["left-fs44100-F1024-min"])                  # periods tau0 - 0.8, - 0.6: the left neighbour is lower
    tiled = FC.batch_input(FC.BY_NAME["residue-tm442-min"])                      # stream 0: a pattern of tauMax - 1 samples, d'[tauMax - 1] = 0
    assert _differs(near, FS, 12, "delta_sign")
    c8 = FC.BY_NAME["near-fs8000-F1024-clamp-0"]                                 # (a - 2 b) + c rounds differently on two of its frames
    assert _differs(FC.batch_input(c8), c8.fs, c8.keys, "association")
    assert not _differs(near, FS, 12, "left_lower") and _differs(left, FS, 12, "left_lower")
    assert not _differs(near, FS, 12, "guard_neighbour") and _differs(tiled, 44200.0, 12, "guard_neighbour")
    # the integer pitch of 227 Hz's period 194 lies on the other side of the midpoint between two notes of key 0 than the refined one
    note = _note_case()
    assert _differs(note, FS, 0, "note_on_integer")
    assert set(FR.MUTANTS) == {"delta_sign", "association", "left_lower", "guard_neighbour", "note_on_integer"}


def _note_case():
    """A tone whose integer pitch fs / tau and refined pitch have different nearest notes in the chromatic table: found by a scan over
    the table's midpoints, on the definition."""
    f, n = R.notes_table(0)
    for i in range(n - 1):
        mid = 0.5 * (float(f[i]) + float(f[i + 1]))
        for eps in (-0.15, 0.15):
            true = mid + eps
            x = FC.half_sine(FS / true, F + R.tau_max(FS))[None, :]
            p, pf, _ = FR.track_fine(x, FS, F, F, 0)
            if p[0, 0] > 0 and O.notes_closest(FS / p[0, 0], 0) != O.notes_closest(FS / pf[0, 0], 0):
                return x
    raise AssertionError("no tone whose two pitches straddle a midpoint")


def test_the_mutants_act_on_the_rule_itself():
    tm = 20
    yt = np.ones(tm + 1)
    yt[9:12] = (0.30, 0.10, 0.20)                                                # a minimum at 10, lower on the right: delta > 0
    tf, br = FR.refine(yt, 10, tm)
    assert br == "refined" and tf == 10.0 + (0.5 * (0.30 - 0.20)) / ((0.30 - 0.10) + (0.20 - 0.10))
    assert FR.refine(yt, 10, tm, "delta_sign")[0] == 10.0 - (tf - 10.0)
    top = np.ones(tm + 1)
    top[tm - 2:] = (0.1, 0.0, 0.0)                                               # tau = tauMax - 1 with an exact zero: the guard slot equals it
    assert FR.refine(top, tm - 1, tm) == (float(tm - 1), "edge") and FR.refine(top, tm - 1, tm, "guard_neighbour") == (tm - 0.5, "refined")
    assert FR.refine(yt, 1, tm) == (1.0, "edge") and FR.refine(yt, 0, tm) == (0.0, "unvoiced")
    low = np.ones(tm + 1)
    low[9:12] = (0.05, 0.10, 0.20)
    assert FR.refine(low, 10, tm) == (10.0, "left_lower") and FR.refine(low, 10, tm, "left_lower")[1] == "refined"
    for bad in ((np.nan, 0.1, 0.2), (0.3, np.nan, 0.2), (0.3, 0.1, np.nan), (0.1, 0.1, 0.1), (np.inf, 0.1, 0.2), (0.3, 0.1, 0.05)):
        y = np.ones(tm + 1)
        y[9:12] = bad
        assert FR.refine(y, 10, tm) == (10.0, "flat"), bad


def test_the_rule_never_moves_a_period_by_more_than_half_a_sample():
    rng = np.random.default_rng(3)
    tm = 64
    n = 0
    for trial in range(4000):
        yt = np.abs(rng.standard_normal(tm + 1)) * 10.0 ** rng.uniform(-300, 300 if trial % 2 else 0)
        tau = int(rng.integers(0, tm + 1))
        if trial % 3 == 0:
            yt[tau - 1:tau + 2] = yt[tau] * (1.0 + 2.0 ** -52 * rng.integers(0, 3, size=len(yt[tau - 1:tau + 2])))   # nearly flat
        tf, br = FR.refine(yt, tau, tm)
        assert abs(tf - tau) <= 0.5 and np.isfinite(tf), (trial, tau, tf)
        n += br == "refined"
    assert n > 500
    for c in FC.CASES:
        p, pf, _, _ = FC.reference(c)
        assert np.all(np.abs(pf - p) <= 0.5)


def test_the_note_is_looked_up_on_the_refined_pitch():
    for c in FC.LEFT_AND_NEAR + [FC.THREE_BY_THREE, FC.NULL_KEYS] + FC.EDGE[:12]:
        p, pf, r, _ = FC.reference(c)
        keys = [12] * 3 if c.keys is None else c.keys
        for s in range(3):
            for f in range(p.shape[1]):
                if p[s, f] > 0:
                    pitch = c.fs / pf[s, f]
                    k = R.norm_key(keys[s])
                    assert R.closest(pitch, k)[0] == O.notes_closest(pitch, k)
                    assert r[s, f] == O.notes_closest(pitch, k) / pitch
                    assert np.array_equal(_bits(FR.voice_ratios_fine(pf[s, f], c.fs, k, [0])), _bits([r[s, f]]))   # degree 0: the mono ratio
                else:
                    assert pf[s, f] == 0.0 and r[s, f] == 1.0
    # an unrefined frame has the integer tracker's bits
    c = FC.BY_NAME["left-fs44100-F1024-clamp"]
    want_p, want_r = R.track(FC.batch_input(c), c.fs, c.F, c.hop, c.keys)
    p, pf, r, _ = FC.reference(c)
    assert np.array_equal(p, want_p) and np.array_equal(_bits(r), _bits(want_r)) and np.array_equal(pf, want_p.astype(np.float64))


# ---- 2. quality: the condition the feature exists for -----------------------------------------------------------------------------------------------
QUALITY_BOUND = 0.1          # fine error / integer error, largest and rms


def quality_signals():
    """{name: [(true f0, float32 row of four frames)]}: 60 fundamentals between 105 and 780 Hz, spaced geometrically."""
    rng = np.random.default_rng(20240607)
    T = F + 3 * HOP + R.tau_max(FS)
    t = np.arange(T) / FS
    out = {"tone": [], "voice": []}
    for f0 in np.geomspace(105.0, 780.0, 60):
        ph = rng.uniform(0, 2 * np.pi)
        out["tone"].append((f0, (0.5 * np.sin(2 * np.pi * f0 * t + ph)).astype(np.float32)))
        y = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 13))
        out["voice"].append((f0, (0.5 * y / np.abs(y).max() + 0.002 * rng.standard_normal(T)).astype(np.float32)))
    return out


def quality_figures():
    """{name: (largest integer error, rms, largest fine error, rms, frames, refined frames)} in cents."""
    out = {}
    for name, rows in quality_signals().items():
        x = np.stack([r for _, r in rows])
        true = np.asarray([f for f, _ in rows])[:, None]
        br = []
        p, pf, _ = FR.track_fine(x, FS, F, HOP, 12, branches=br)
        p, pf, br = p[:, :4], pf[:, :4], [row[:4] for row in br]                  # (the fifth frame repeats the fourth's clamped window)
        voiced = int(np.count_nonzero(p > 0))
        refined = sum(b == "refined" for row in br for b in row)
        with np.errstate(divide="ignore"):
            ci, cf = np.abs(FR.cents(FS / p, true)), np.abs(FR.cents(FS / pf, true))
        out[name] = (ci.max(), np.sqrt(np.mean(ci ** 2)), cf.max(), np.sqrt(np.mean(cf ** 2)), p.size, voiced, refined)
    return out


def quality_text(fig):
    lines = ["Fine pitch tracker: error of the tracked pitch in cents, integer period against refined period (tests/pv_track_fine_reference.py on",
             "the CPU; no GPU run).  60 fundamentals 105 .. 780 Hz spaced geometrically, four frames each, F 1024, hop 256, 44.1 kHz, seed fixed:",
             "pure 0.5-amplitude tones, and 12-harmonic voices (1/h) with 0.002 noise.  Written by tests/test_pv_track_fine_reference_cpu.py",
             "(VP_WRITE_PROFILES=1), which asserts fine <= 0.1 x integer for both figures on both signals.", "",
             "signal   frames voiced refined   integer max   integer rms   fine max   fine rms   max ratio   rms ratio"]
    for name, (im, ir, fm, fr, n, v, rf) in fig.items():
        lines.append(f"{name:8s} {n:6d} {v:6d} {rf:7d}   {im:11.2f}   {ir:11.2f}   {fm:8.2f}   {fr:8.2f}   {fm / im:9.3f}   {fr / ir:9.3f}")
    return "\n".join(lines) + "\n"


def test_the_refined_pitch_is_ten_times_closer():
    fig = quality_figures()
    text = quality_text(fig)
    print(text)
    path = os.path.join(ROOT, "profiles", "pv_track_fine_quality.txt")
    if os.environ.get("VP_WRITE_PROFILES") == "1":
        with open(path, "w") as f:
            f.write(text)
    for name, (im, ir, fm, fr, n, voiced, refined) in fig.items():
        assert n == 240 and voiced == 240 and refined == 240, (name, n, voiced, refined)
        assert fm <= QUALITY_BOUND * im and fr <= QUALITY_BOUND * ir, (name, im, ir, fm, fr)
    # the recorded figures are these: counts exactly, cents and ratios to the last printed digit and one more unit of it (another
    # NumPy or libm may move a rounding)
    with open(path) as f:
        rows = {ln.split()[0]: ln.split()[1:] for ln in f.read().splitlines() if ln.split() and ln.split()[0] in fig}
    assert set(rows) == set(fig), sorted(rows)
    for name, (im, ir, fm, fr, n, voiced, refined) in fig.items():
        rec = rows[name]
        assert [int(v) for v in rec[:3]] == [n, voiced, refined], (name, rec)
        for got, want, tol in zip(rec[3:], (im, ir, fm, fr, fm / im, fr / ir), (0.02, 0.02, 0.02, 0.02, 0.002, 0.002)):
            assert abs(float(got) - want) <= tol, (name, rec, want)


# ---- 3. the device cases reach every branch ---------------------------------------------------------------------------------------------------------
def test_the_device_cases_reach_every_branch():
    counts = FC.branch_counts(FC.CASES)
    print(f"PV TRACK FINE branches {counts}")
    for b in ("refined", "edge", "left_lower", "unvoiced"):
        assert counts[b] >= FC.MIN_PER_BRANCH, counts
    edge = FC.branch_counts(FC.EDGE)
    assert edge["refined"] >= 600 and edge["edge"] >= 200 and edge["unvoiced"] >= 40 and edge["left_lower"] == 0, edge
    for c in FC.LEFT_AND_NEAR:
        want = "left_lower" if c.name.startswith("left") else "refined"
        p, pf, _, br = FC.reference(c)
        assert all(b == want for row in br for b in row) and np.all(p == R.tau_min(c.fs)), (c.name, br)
    # periods below tau0 refine downwards, above it upwards: both signs of delta
    lo, hi = FC.reference(FC.BY_NAME["near-fs44100-F1024-clamp-0"]), FC.reference(FC.BY_NAME["near-fs44100-F1024-clamp-3"])
    assert np.all(lo[1][:2] < lo[0][:2]) and np.all(hi[1] > hi[0])


def test_the_batch_shapes_are_the_ones_the_issue_names():
    assert {c.length for c in FC.CASES} == {"clamp", "min", "three"}
    c = FC.THREE_BY_THREE
    assert FC.reference(c)[0].shape == (3, 3) and 9 % 4 != 0
    assert FC.NULL_KEYS.keys is None and all(len(c.signals) == 3 for c in FC.CASES)
    assert any(c.keys is not None and -1 in c.keys and 13 in c.keys for c in FC.CASES)


# ---- 4. the streaming definition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.STREAM_CASES, ids=lambda c: c.name)
def test_streaming_fine_is_the_batch_decision_then_the_integer_follow(c):
    x = FC.stream_input(c)
    p, pf, r = FC.stream_reference(c)
    n, S, N = x.shape
    W = SR.window_len(c.fs, c.F)
    rows = np.ascontiguousarray(x.transpose(1, 0, 2).reshape(S, n * N))
    assert N < W <= (n - 5) * N                                                  # the ring fills inside the run
    raw = np.ones((n, S))
    for b in range(n):
        e = (b + 1) * N
        if e < W:
            assert np.all(p[b] == 0) and np.all(pf[b] == 0.0)
            continue
        bp, bf, br = FR.track_fine(rows[:, e - W:e], c.fs, c.F, c.F, c.keys)
        assert np.array_equal(p[b], bp[:, 0]) and np.array_equal(_bits(pf[b]), _bits(bf[:, 0]))
        raw[b] = br[:, 0]
    for s in range(S):
        want, _ = SR.follow(p[:, s], raw[:, s], c.hold, c.glide)
        assert np.array_equal(_bits(r[:, s]), _bits(want))
    for name, g in FC.stream_groupings(c).items():
        if name == "single" and n > 12:
            continue
        got = FSR.run(x, c.fs, c.F, c.keys, c.hold, c.glide, groups=g)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, (p, pf, r))), name


def test_a_mode_change_changes_only_what_follows():
    c = FC.STREAM_CASES[2]
    x = FC.stream_input(c)
    g = [4, 3, 3]
    p, pf, r = FSR.run(x, c.fs, c.F, c.keys, 0, 1.0, groups=g, fine=[False, True, False])
    ip, ir = SR.run(x, c.fs, c.F, c.keys, 0, 1.0)
    fp, ff, fr = FSR.run(x, c.fs, c.F, c.keys, 0, 1.0)
    assert np.array_equal(p, ip) and np.array_equal(p, fp)
    assert np.array_equal(_bits(r[:4]), _bits(ir[:4])) and np.array_equal(_bits(r[4:7]), _bits(fr[4:7])) and np.array_equal(_bits(r[7:]), _bits(ir[7:]))
    assert not np.array_equal(_bits(ir[4:7]), _bits(fr[4:7]))


def test_streaming_voices_at_degree_zero_are_the_mono_fine_table():
    c = FC.STREAM_CASES[1]
    x = FC.stream_input(c)
    p, pf, r = FC.stream_reference(c)
    t = FSR.FineStreamVoices(x.shape[1], c.N, c.fs, c.F, c.hold, c.glide)
    vp, vr = t.process(x, [0, 2, -3], c.keys)
    assert np.array_equal(vp, p) and np.array_equal(_bits(vr[:, :, 0]), _bits(r))
    import pv_harmkey_stream_reference as HSR
    ip, ivr = HSR.run(x, c.fs, c.F, [0, 2, -3], c.keys, hold=c.hold, glide=c.glide)
    assert np.array_equal(ip, p) and not np.array_equal(_bits(ivr), _bits(vr))
    t2 = FSR.FineStreamVoices(x.shape[1], c.N, c.fs, c.F, c.hold, c.glide)
    t2.fine = False
    p2, vr2 = t2.process(x, [0, 2, -3], c.keys)
    assert np.array_equal(_bits(vr2), _bits(ivr))                                # with the integer decision it is the integer definition


# ---- 5. the kernels' budgets, from the built code object ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resources():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    return kernel_resources.kernel_resources(build.build())


@pytest.mark.parametrize("kernel", NEW_KERNELS)
def test_the_fine_kernels_are_within_the_tracker_s_budget(resources, kernel):
    r = resources[kernel]
    print(f"PV TRACK FINE resources {kernel} {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["agpr"] == 0 and r["vgpr"] <= 128 and r["lds"] == 0, r


def test_the_recorded_rows_are_the_built_ones(resources):
    rows = {}
    with open(os.path.join(ROOT, "profiles", "pv_track_fine_resources.txt")) as f:
        for line in f:
            m = re.match(r"^(vp_k_\S+)\s+((?:\d+\s*){5})$", line)
            if m:
                rows[m.group(1)] = tuple(int(v) for v in m.group(2).split())
    siblings = ("vp_k_yin_track", "vp_k_yin_track_stream", "vp_k_yin_track_voices", "vp_k_yin_track_voices_stream")
    assert set(rows) == set(NEW_KERNELS + siblings), sorted(rows)
    for k in rows:
        r = resources[k]
        assert rows[k] == (r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"]), (k, rows[k], r)


def test_the_new_sources_are_part_of_the_build():
    from vocoderproject_amd import build
    assert "vp_track_fine.inc" in build.DEPS and "vp_track_fine_kernels.inc" in build.DEPS and len(build.SOURCES) == 6
    with open(os.path.join(ROOT, "vocoderproject_amd", "csrc", "vp_track.hip")) as f:
        text = f.read()
    assert text.count('#include "vp_track_body.inc"') == 2
    assert text.rstrip().endswith('#include "vp_track_fine_kernels.inc"') and text.index("vp_track_voices_kernels.inc") < text.index("vp_track_fine_kernels.inc")


# ---- 6. the library's host layers, without a device ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    return C.CDLL(build.build())


def test_null_handles_and_the_abi_version(lib):
    vp = C.c_void_p
    lib.vp_stft_track_pitch_fine.argtypes = [vp, vp, C.c_double, vp, vp, vp, vp, vp]
    lib.vp_pv_tracker_process_blocks_fine_device.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp]
    lib.vp_stft_set_track_mode.argtypes = lib.vp_pv_tracker_set_mode.argtypes = [vp, C.c_int]
    lib.vp_stft_get_track_mode.argtypes = lib.vp_pv_tracker_get_mode.argtypes = [vp]
    assert lib.vp_stft_track_pitch_fine(None, 8, 44100.0, None, 8, 8, 8, None) == -1
    assert lib.vp_pv_tracker_process_blocks_fine_device(None, 8, None, 8, 8, 8, 1, None) == -1
    for mode in (0, 1, 2, -1):
        assert lib.vp_stft_set_track_mode(None, mode) == -1 and lib.vp_pv_tracker_set_mode(None, mode) == -1
    assert lib.vp_stft_get_track_mode(None) == -1 and lib.vp_pv_tracker_get_mode(None) == -1
    lib.vp_abi_version.restype = C.c_int
    assert lib.vp_abi_version() == 3
    with open(os.path.join(ROOT, "include", "vp_amd.h")) as f:
        h = f.read()
    assert re.search(r"#define VP_TRACK_INTEGER 0\b", h) and re.search(r"#define VP_TRACK_FINE 1\b", h)


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
    if (vp_stft_track_pitch_fine(nullptr, nullptr, 44100.0, nullptr, nullptr, nullptr, nullptr, nullptr) != VP_ERR_INVALID_ARG) return 2;
    if (vp_stft_set_track_mode(nullptr, VP_TRACK_FINE) != VP_ERR_INVALID_ARG || vp_pv_tracker_set_mode(nullptr, VP_TRACK_INTEGER) != VP_ERR_INVALID_ARG) return 3;
    try {
        vp::StreamingPitchTracker trk(0, 4, 256, 44100.0);
        if (trk.fine()) return 4;
        trk.setFine(true);
        if (!trk.fine() || vp_pv_tracker_get_mode(trk.handle()) != VP_TRACK_FINE) return 5;
        trk.setFine(false);
        if (trk.fine()) return 6;
        try { trk.processBlocksFine(nullptr, nullptr, nullptr, nullptr, nullptr, 1); return 7; } catch (const vp::Error &e) { if (e.code != VP_ERR_INVALID_ARG) return 8; }
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


# ---- 7. the offline flows and their command line, the definitions in place of the GPU -----------------------------------------------------------
class _Definition:
    """The flows' processor: the definitions in place of the GPU.  run returns the input as the audio (the shift is the sibling files'
    subject) and the definition's tables; set_fine is the mode setter the flows must reach."""

    def __init__(self, hop=256, stream_N=None, hold=0, glide=1.0, voices=False):
        self.hop, self.N, self.hold, self.glide, self.voices, self.fine, self.set_calls = hop, stream_N, hold, glide, voices, False, []

    def set_fine(self, fine):
        self.set_calls.append(fine)
        self.fine = bool(fine)

    def run(self, x, fs, keys, *tables, **kw):
        import pv_harmkey_reference as HR
        import pv_harmkey_stream_reference as HSR
        S = x.shape[0]
        if self.N is None:
            p, pf, r = FR.track_fine(x, fs, 1024, self.hop, keys)
            if not self.fine:
                p, r = R.track(x, fs, 1024, self.hop, keys)
            if self.voices:
                unv = HR.nominal_unvoiced(tables[0], keys, S)
                r = (FR.track_harmony_fine if self.fine else HR.track_harmony)(x, fs, 1024, self.hop, tables[0], keys, unv)[1]
        else:
            blocks = np.ascontiguousarray(x.reshape(S, x.shape[1] // self.N, self.N).transpose(1, 0, 2))
            if self.voices:
                unv = HR.nominal_unvoiced(tables[0], keys, S)
                t = FSR.FineStreamVoices(S, self.N, fs, 1024, self.hold, self.glide)
                t.fine = self.fine
                p, r = t.process(blocks, tables[0], keys, unv)
                pf = t.raw_tracker.period_fine
                if not self.fine:
                    assert np.array_equal(r, HSR.run(blocks, fs, 1024, tables[0], keys, unv, self.hold, self.glide)[1])
            else:
                p, pf, r = FSR.run(blocks, fs, 1024, keys, self.hold, self.glide, fine=[self.fine])
        return (x.copy(), p, r, pf) if self.fine else (x.copy(), p, r)


def _tone(n, period):
    return FC.half_sine(period, n)


def test_the_offline_flows_reach_the_mode_setter_and_return_the_refined_periods():
    from vocoderproject_amd import offline
    voices = [_tone(6000, 200.37), _tone(5000, 150.8)]
    for stream in (False, True):
        flow = offline.pv_autotune_stream if stream else offline.pv_autotune
        skw = dict(N=256) if stream else {}
        p = _Definition(stream_N=256 if stream else None)
        outs, period, ratio = flow(voices, 44100.0, key=0, processor=p, with_track=True, **skw)
        assert p.set_calls == []                                                     # without fine the setter is not touched
        p = _Definition(stream_N=256 if stream else None)
        outs, fperiod, fratio, fine = flow(voices, 44100.0, key=0, processor=p, with_track=True, fine=True, **skw)
        assert p.set_calls == [True] and [o.shape for o in outs] == [(2, 6000), (2, 5000)]
        assert np.array_equal(period, fperiod) and fine.shape == period.shape and not np.array_equal(ratio, fratio)
        voiced = period > 0
        assert np.count_nonzero(voiced) > 10 and np.all(np.abs(fine - period) <= 0.5) and np.all(fine[~voiced] == 0.0)
        col = (slice(None), 0) if stream else (0, slice(None))
        first, n_in = (1465 // 256 + 1, (6000 - 1465) // 256 - 1465 // 256 - 1) if stream else (0, (6000 - 1465) // 256)
        inside = slice(first, first + n_in)                                         # decisions whose window lies inside the tone
        assert n_in > 5 and np.all(period[col][inside] == 200) and np.all(np.abs(fine[col][inside] - 200.37) < 0.02)   # the refined period is the tone's
        with pytest.raises(ValueError, match="returned 2 tables where 3"):
            q = _Definition(stream_N=256 if stream else None)
            q.set_fine = lambda f: None                                             # a processor that ignores the setter
            flow(voices, 44100.0, key=0, processor=q, fine=True, **skw)
        # the key-aware harmonizer
        p = _Definition(stream_N=256 if stream else None, voices=True)
        outs, hp, hr, hf = offline.pv_harmonize_key(voices, 44100.0, [0, 2], key=0, stream=stream, N=256, processor=p, with_track=True, fine=True)
        assert p.set_calls == [True] and np.array_equal(hp, period) and np.array_equal(_bits(hf), _bits(fine))
        assert np.array_equal(_bits(hr[:, :, 0] if stream else hr[:, 0]), _bits(fratio))   # degree 0: the mono fine ratio
        p = _Definition(stream_N=256 if stream else None, voices=True)
        assert len(offline.pv_harmonize_key(voices, 44100.0, [0, 2], key=0, stream=stream, N=256, processor=p, with_track=True)) == 3 and p.set_calls == []


@pytest.mark.parametrize("stream", [False, True])
def test_command_line_the_csv_has_four_columns_only_with_fine(tmp_path, monkeypatch, stream):
    from vocoderproject_amd import offline
    a = str(tmp_path / "a.wav")
    offline.write_wav(a, 44100, _tone(6000, 200.37))
    procs = []
    real = {n: getattr(offline, n) for n in ("pv_autotune", "pv_autotune_stream", "pv_harmonize_key")}

    def through(name, voices=False):
        def f(*args, **kw):
            procs.append((name, dict(kw), _Definition(stream_N=kw.get("N") if stream else None, hold=kw.get("hold", 0), glide=kw.get("glide", 1.0), voices=voices)))
            return real[name](*args, processor=procs[-1][2], **kw)
        return f
    monkeypatch.setattr(offline, "pv_autotune", through("pv_autotune"))
    monkeypatch.setattr(offline, "pv_autotune_stream", through("pv_autotune_stream"))
    monkeypatch.setattr(offline, "pv_harmonize_key", through("pv_harmonize_key", voices=True))
    extra = ["--stream", "--block", "256"] if stream else []
    texts = {}
    for flow, tail in (("pvtune", "a_pvtune.csv"), ("harmonize", "a_harmonize_v1.csv")):
        for fine in (False, True):
            out = str(tmp_path / f"{flow}{int(fine)}")
            argv = [flow, a, "--key", "0", "--track-csv", "--out-dir", out] + (["--degrees", "0,2"] if flow == "harmonize" else []) + extra + (["--fine"] if fine else [])
            assert offline.main(argv) == 0
            name, kw, p = procs[-1]
            assert ("fine" in kw) == fine and p.set_calls == ([True] if fine else [])     # --fine reaches the mode setter, and only --fine
            with open(os.path.join(out, tail)) as f:
                texts[flow, fine] = f.read().splitlines()
        plain, four = texts[flow, False], texts[flow, True]
        assert plain[0] == "time_s,period,semitones" and four[0] == "time_s,period,semitones,period_fine" and len(plain) == len(four) > 10
        assert all(len(r.split(",")) == 3 for r in plain) and all(len(r.split(",")) == 4 for r in four)
        inside = (6000 - 1465) // 256 - (1465 // 256 + 1 if stream else 0)   # decisions whose window lies inside the tone
        rows = [r.split(",") for r in four[1:]][1465 // 256 + 1 if stream else 0:][:inside]
        assert len(rows) > 5 and all(r[1] == "200" and abs(float(r[3]) - 200.37) < 0.02 for r in rows), rows
        assert [r.split(",")[:2] for r in plain] == [r.split(",")[:2] for r in four]
    for bad in (["pvshift", a, "--shift", "2", "--fine", "--out-dir", str(tmp_path / "x")], ["harmonize", a, "--voices", "4", "--fine", "--out-dir", str(tmp_path / "x")]):
        with pytest.raises(SystemExit, match="--fine"):
            offline.main(bad)
