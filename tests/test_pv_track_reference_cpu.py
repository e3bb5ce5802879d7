"""CPU-side checks of the pitch tracker (vp_stft_track_pitch, vp_stft_autotune): the definition tests/pv_track_reference.py is
conditioned (it reproduces known periods, the case table holds voiced and unvoiced frames in numbers, every ratio is a legal curve
entry), it has teeth (seeded faults of it change its output on named cases), it closes the loop through the NumPy phase vocoder, and the
library declares and exports the new entry points and refuses bad arguments without a device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_track_cases as TC  # noqa: E402
import pv_track_reference as R  # noqa: E402
import stft_reference as SR  # noqa: E402

SYMBOLS = ["vp_track_tau_max", "vp_stft_track_pitch", "vp_stft_autotune"]


# ---- conditioning -----------------------------------------------------------------------------------------------------------------------
def _one(x, key=12, fs=44100.0, F=1024, hop=256):
    p, r = R.track(np.asarray(x, np.float32)[None], fs, F, hop, key)
    return p[0], r[0]


def test_reference_reproduces_known_periods():
    fs, F, hop = 44100.0, 1024, 256
    T = F + 8 * hop + R.tau_max(fs)
    t = np.arange(T) / fs
    sine = lambda f: np.sin(2.0 * np.pi * f * t)                                  # noqa: E731
    assert np.all(_one(sine(220.0))[0] == 200)
    p, r = _one(sine(227.0))
    assert np.all(p == 194) and np.allclose(R.semitones(r), 0.433, atol=1e-3)
    p, r = _one(sine(227.0), key=0)
    assert np.all(p == 194) and np.allclose(R.semitones(r), -0.567, atol=1e-3)
    ph = 330.5 * t
    assert np.all(_one(2.0 * (ph - np.floor(ph)) - 1.0)[0] == 133)
    for x in (np.random.default_rng(1).standard_normal(T), np.zeros(T)):            # (silence: 0 * inf = NaN fails `< yinTol`)
        p, r = _one(x)
        assert np.all(p == 0) and np.all(r == 1.0)
    for f in (100.2, 90.0):                                                         # the walk's `tau + 1 >= tauMax` exit
        assert R.tau_max(fs) - 1 == 440 and np.all(_one(sine(f))[0] == 440)
    glide = np.sin(2.0 * np.pi * np.cumsum(200.0 + 60.0 * np.arange(T) / (T - 1)) / fs)
    p12, r12 = _one(glide)
    p0, r0 = _one(glide, key=0)
    assert np.array_equal(p12, p0) and len(np.unique(p12)) >= len(p12) - 1 and not np.array_equal(r12, r0)


def test_case_table_holds_voiced_and_unvoiced_frames_and_legal_ratios():
    total = voiced = 0
    for c in TC.CASES:
        p, r = TC.reference(c)
        nF = R.n_frames(TC.length(c), c.F, c.hop)
        assert p.shape == r.shape == (TC.N_STREAMS, nF) and p.dtype == np.int32 and r.dtype == np.float64
        assert np.all((r >= 0.5) & (r <= 2.0)), TC.case_id(c)
        assert np.all(r[p == 0] == 1.0) and np.all((p == 0) | ((p >= int(c.fs // 800)) & (p <= R.tau_max(c.fs)))), TC.case_id(c)
        total += p.size
        voiced += int((p > 0).sum())
    print(f"PV TRACK cases {len(TC.CASES)} frames {total} voiced {voiced} unvoiced {total - voiced}")
    assert voiced * 3 >= total and (total - voiced) * 10 >= total, (voiced, total)


def test_domain_is_refused():
    x = np.zeros((1, 1024 + 441), np.float32)
    R.track(x, 44100.0, 1024, 256)
    for fs, xx in ((7999.0, x), (51201.0, x), (44100.0, x[:, :-1])):
        with pytest.raises(AssertionError):
            R.track(xx, fs, 1024, 256)


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------
# what a seeded fault must change: the period on some case, or (the key plays no part in the period) the ratio
TEETH = {"unclamped": "period", "no_descent": "period", "key_ignored": "ratio", "guard_nonzero": "period"}


@pytest.mark.parametrize("mutant", sorted(TEETH))
def test_seeded_fault_changes_the_reference_on_a_named_case(mutant):
    hit = None
    for c in TC.CASES:
        p, r = TC.reference(c)
        pm, rm = R.track(TC.case_input(c), c.fs, c.F, c.hop, c.keys, mutant=mutant)
        if TEETH[mutant] == "period" and not np.array_equal(p, pm):
            hit = (TC.case_id(c), int((p != pm).sum()))
            break
        if TEETH[mutant] == "ratio":
            assert np.array_equal(p, pm), TC.case_id(c)                            # (the walk does not know the key)
            if not np.array_equal(r, rm):
                hit = (TC.case_id(c), int((r != rm).sum()))
                break
    print(f"PV TRACK mutant {mutant}: first case that differs {hit}")
    assert hit is not None, f"the fault '{mutant}' changes the {TEETH[mutant]} on no case of tests/pv_track_cases.py"


def test_pairwise_summation_is_a_different_function():
    """The order of the sum over i is part of the definition: numpy's pairwise sum gives other bits in d.  Recorded on the shortest rows of
    the first geometry: d differs on every voiced stream; the periods there do not (the walk's comparisons are far from ties), so only a
    difference in d is required."""
    d_hits, tau_hits = [], []
    for c in [c for c in TC.CASES if (c.fs, c.F, c.hop, c.length) == (44100.0, 1024, 256, "min")]:
        x = TC.case_input(c)
        p, _, fn = R.track(x, c.fs, c.F, c.hop, c.keys, with_function=True)
        pm, _, fm = R.track(x, c.fs, c.F, c.hop, c.keys, mutant="pairwise", with_function=True)
        assert np.array_equal(p, TC.reference(c)[0])
        if not np.array_equal(fn, fm, equal_nan=True):
            d_hits.append(TC.case_id(c))
        if not np.array_equal(p, pm):
            tau_hits.append(TC.case_id(c))
    print(f"PV TRACK mutant pairwise: d differs on {len(d_hits)} cases, the period on {len(tau_hits)}")
    assert d_hits, "pairwise summation gives the left-to-right sums' bits on every case tried"


# ---- closed loop without a GPU ------------------------------------------------------------------------------------------------------------
def test_closed_loop_through_the_numpy_phase_vocoder():
    """tracker -> stft_roundtrip with the tracker's ratio -> tracker: every frame of the corrected signal has a period within one sample
    of fs / closestFreq.  Figures: 227 Hz -> 189 against 189.20, in key 0 -> 201 against 200.45; 330.5 Hz -> 134 against 133.79;
    205 Hz -> 212 / 213 against 212.37."""
    x, keys = TC.steady_input()
    fs, F, hop = TC.STEADY_FS, TC.STEADY_F, TC.STEADY_HOP
    p, r = R.track(x, fs, F, hop, keys)
    for s, target in enumerate(TC.steady_targets()):
        assert len(np.unique(r[s])) == 1 and p[s, 0] > 0, (s, p[s])                 # steady: one ratio for the whole row
        y = SR.stft_roundtrip(x[s].astype(np.float64), F, hop, ratio=float(r[s, 0]))
        p2, _ = R.track(np.asarray(TC.covered_part(y, F, hop), np.float32)[None], fs, F, hop, keys[s])
        print(f"PV TRACK closed loop {TC.STEADY[s]}: period {p[s, 0]} -> {sorted(set(p2[0].tolist()))} target {target:.2f}")
        assert p2.shape[1] >= 8 and np.all(np.abs(p2[0] - target) <= 1.0), (s, p2[0], target)


# ---- library surface ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    return C.CDLL(build.build())


def test_new_symbols_are_declared_and_exported(lib):
    txt = open(os.path.join(ROOT, "include", "vp_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} not declared in include/vp_amd.h"
        assert hasattr(lib, s), f"{s} not exported"
    assert "#define VP_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "vp_amd.h")).read() and lib.vp_abi_version() == 3


def test_tau_max_and_its_domain(lib):
    lib.vp_track_tau_max.argtypes = [C.c_double]
    assert [lib.vp_track_tau_max(fs) for fs in (44100.0, 48000.0, 8000.0, 51200.0)] == [441, 480, 80, 512]
    assert [lib.vp_track_tau_max(fs) for fs in (44100.0, 48000.0, 8000.0, 51200.0)] == [R.tau_max(fs) for fs in (44100.0, 48000.0, 8000.0, 51200.0)]
    assert lib.vp_track_tau_max(7999.0) < 0 and lib.vp_track_tau_max(51201.0) < 0 and lib.vp_track_tau_max(float("nan")) < 0


def test_null_handle_is_an_error_not_a_crash(lib):
    lib.vp_stft_track_pitch.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_stft_autotune.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    one = C.c_void_p(8)
    assert lib.vp_stft_track_pitch(None, one, 44100.0, None, one, one, None) == -1
    assert lib.vp_stft_autotune(None, one, one, 44100.0, None, one, one, None) == -1
    lib.vp_stft_last_error.restype = C.c_char_p
    lib.vp_stft_last_error.argtypes = [C.c_void_p]
    assert lib.vp_stft_last_error(None) == b""


def test_build_compiles_the_tracker_with_the_default_flags():
    """-ffp-contract=off is what makes the kernel's sums the oracle's: vp_track.hip is its own translation unit with no extra flags (the
    STFT unit's -ffp-contract=fast does not reach it), it is a build dependency, and the units bench.py hashes do not include it."""
    from vocoderproject_amd import build
    assert "vp_track.hip" in build.SOURCES and {"vp_track.hip", "vp_track.h"} <= set(build.DEPS)
    src = open(os.path.join(ROOT, "vocoderproject_amd", "build.py")).read()
    assert re.search(r'"vp_track\.hip"\), os\.path\.join\(tmp, "track\.o"\), \[\]\)', src)
    for f in ("vp_kernels.hip", "vp_voc2.hip", "vp_stft.hip"):
        assert "vp_track" not in open(os.path.join(ROOT, "vocoderproject_amd", "csrc", f)).read(), f
