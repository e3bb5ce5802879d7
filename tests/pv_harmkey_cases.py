"""The case table of the key-aware voices (vp_stft_track_harmony, vp_stft_harmonize_key, vp_pv_tracker_process_blocks_voices_device,
vp_hz_autoharm_blocks_device): what tests/test_pv_harmkey_reference_cpu.py (conditioning, teeth) and tests/test_gpu_pv_harmkey.py (bit
equality with the definitions) BOTH iterate.  Test infrastructure only.  The signal builders are tests/pv_track_cases.py's and
tests/pv_track_edge_cases.py's; no sample is a float32 denormal (batch_input and stream_input assert it).  The reference of a case is
computed once and shared; callers do not write to it.

Batch: S = 3 streams x T = 4096 samples at 44.1 kHz, F = 1024, hop 256: 13 frames a stream, 39 in all -- no multiple of the kernel's four
frames per workgroup, so its tail guard runs.  One case has F = 2048 / hop 512, one runs at 8 kHz (tauMax 80) with T = 2048.

`expect` names what a case is there for, per stream, as a predicate on the definition's tables (tests/test_pv_harmkey_reference_cpu.py
fails when a case does not reach it); `kills` names the mutants of the definition that must differ on the case."""
from collections import namedtuple

import numpy as np

import pv_harmkey_reference as HR
import pv_harmkey_stream_reference as HSR
import pv_track_cases as TC
import pv_track_edge_cases as EC
import pv_track_reference as R

S = 3
NAN = float("nan")
Case = namedtuple("Case", "name fs F hop T signals keys degrees unvoiced expect kills")
_G = (44100.0, 1024, 256, 4096)
# the period of a sharp A3 at 44.1 kHz (221.6 Hz), and of a note just above the table's lowest (104.0 Hz): the lower clamp's case
P_A3, P_LOW = 199, 424

CASES = [
    # steady voices of integer period; keys in and out of range; degrees of both signs and 0
    Case("steady-v3", *_G, (("sine_p", P_A3), ("sine_p", 150), ("sine_p", 300)), (0, 11, 12), ((0, 2, 4), (-3, 0, 5), (7, -12, 0)), None,
         ("voiced",) * 3, ("parallel", "index_from_lower_bound")),
    Case("steady-v1", *_G, (("sine_p", P_A3), ("sine_p", 150), ("sine_p", 300)), (99, 0, 11), ((4,), (-2,), (0,)), None, ("voiced",) * 3, ()),
    Case("steady-v4", *_G, (("sine_p", P_A3), ("sine_p", 150), ("sine_p", 300)), (12, 99, 0), ((0, 4, 7, -12), (12, -5, 0, 3), (-7, 0, 2, 4)), None,
         ("voiced",) * 3, ()),
    Case("glide-v4", *_G, (("tc", "glide"), ("tc", "vibrato"), ("tc", "saw")), (0, 11, 12), ((2, -2, 0, 4), (0, 1, -1, 7), (3, 0, -4, 12)),
         ((1.25, 0.8, 1.0, 1.5),) * 3, ("voiced",) * 3, ("parallel",)),
    # silence and noise: unvoiced frames take u; no table gives 1.0; a NaN or an infinity gives 1.0
    Case("unvoiced-u", *_G, (("tc", "silence"), ("tc", "noise"), ("tc", "gap")), (0, 11, 12), ((0, 2, 4), (-3, 0, 5), (7, -12, 0)),
         ((1.125, 0.75, 1.5), (0.9, 1.0, 1.3), (2.5, 0.25, 1.0)), ("unvoiced", "unvoiced", "some_unvoiced"), ("unvoiced_one",)),
    Case("unvoiced-null", *_G, (("tc", "silence"), ("tc", "noise"), ("tc", "gap")), (0, 11, 12), ((0, 2, 4), (-3, 0, 5), (7, -12, 0)), None,
         ("unvoiced", "unvoiced", "some_unvoiced"), ()),
    Case("unvoiced-nan", *_G, (("tc", "silence"), ("tc", "noise"), ("tc", "gap")), (0, 11, 12), ((0, 2, 4), (-3, 0, 5), (7, -12, 0)),
         ((NAN, 0.75, float("inf")), (0.9, NAN, float("-inf")), (NAN, NAN, 1.2)), ("unvoiced", "unvoiced", "some_unvoiced"), ()),
    # the popped slot (c = n) in scale keys, seven degrees up and down from it
    Case("popped", *_G, (("sine_p", 55.5), ("sine_p", 56.0), ("sine_p", 55.0)), (0, 7, 0), ((7, -7, 0),) * 3, None,
         ("popped",) * 3, ("popped_as_top",)),
    # the lower clamp: j = off + c + d < 0
    Case("low-clamp", *_G, (("sine_p", P_LOW), ("sine_p", P_LOW), ("sine_p", P_LOW)), (11, 12, 0), ((-7, 0, -12), (-12, -11, 0), (-12, 0, 12)), None,
         ("clamped", "clamped", "voiced"), ("no_lower_clamp",)),
    Case("f2048", 44100.0, 2048, 512, 4096, (("sine_p", P_A3), ("tc", "glide"), ("tc", "noise")), (0, 11, 12), ((0, 2, 4), (-3, 0, 5), (7, -12, 0)),
         ((1.1, 1.2, 1.3),) * 3, ("voiced", "voiced", "unvoiced"), ()),
    Case("fs8000", 8000.0, 1024, 256, 2048, (("sine_p", 36), ("sine_p", 61.5), ("tc", "noise")), (0, 11, 12), ((0, 2, 4), (-3, 0, 5), (7, -12, 0)),
         ((1.1, 1.2, 1.3),) * 3, ("voiced", "voiced", "unvoiced"), ()),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) and {len(c.degrees[0]) for c in CASES} == {1, 3, 4}
assert all(len(c.signals) == len(c.keys) == len(c.degrees) == len(c.expect) == S for c in CASES)


def case_id(c):
    return c.name


def batch_input(c):
    """float32 [3][T]"""
    x = EC.make_rows(c.signals, c.T, c.fs, int(c.fs) + c.hop)
    assert TC.no_denormals(x)
    return x


def degrees_of(c):
    return np.asarray(c.degrees, np.int32)


def unvoiced_of(c):
    return None if c.unvoiced is None else np.asarray(c.unvoiced, np.float64)


_REF = {}


def reference(c):
    """(period int32 [3][nF], ratio float64 [3][V][nF]) of the case, computed once."""
    if c.name not in _REF:
        p, r = HR.track_harmony(batch_input(c), c.fs, c.F, c.hop, degrees_of(c), c.keys, unvoiced_of(c))
        p.setflags(write=False)
        r.setflags(write=False)
        _REF[c.name] = (p, r)
    return _REF[c.name]


def _c_and_j(c, s):
    """Per voiced frame of stream s: (c == n, min over voices of off + c + d)."""
    p = reference(c)[0][s]
    key = R.norm_key(c.keys[s])
    n, off = R.notes_table(key)[1], HR.harmony_table(key)[2]
    out = []
    for tau in p[p > 0]:
        ci = HR.chosen_index(c.fs / int(tau), key)[0]
        out.append((ci == n, min(off + ci + max(-12, min(12, d)) for d in c.degrees[s])))
    return out


def holds(c, s):
    """Does stream s of the case reach what it is there for?"""
    p = reference(c)[0][s]
    e = c.expect[s]
    if e == "voiced":
        return bool(np.all(p > 0))
    if e == "unvoiced":
        return bool(np.all(p == 0))
    if e == "some_unvoiced":
        return bool(np.any(p == 0) and np.any(p > 0))
    if e == "popped":
        return bool(np.all(p > 0)) and all(pop for pop, _ in _c_and_j(c, s))
    if e == "clamped":
        return bool(np.all(p > 0)) and all(j < 0 for _, j in _c_and_j(c, s))
    raise KeyError(e)


# ---- streaming: S = 3, N = 256, 24 blocks, V = 3 ------------------------------------------------------------------------------------------
STREAM_FS, STREAM_F, STREAM_N, STREAM_BLOCKS = 44100.0, 1024, 256, 24
STREAM_SIGNALS = (("sine_p", P_A3), ("tone_zeros", 3000), ("tc", "glide"))        # stream 1 falls silent: the hold and the unvoiced target run
STREAM_KEYS = (0, 11, 12)
STREAM_DEGREES = ((0, 2, 4), (-3, 0, 5), (7, -12, 0))
STREAM_UNVOICED = ((1.125, 0.75, 1.5), (0.9, 1.1, 1.3), (2.5, 0.25, 1.0))
STREAM_FOLLOW = ((0, 1.0), (3, 0.5))
STREAM_GROUPINGS = {"whole": [24], "singles": [1] * 24, "1+7+16": [1, 7, 16]}
FIRST_DECISION = -(-(STREAM_F + R.tau_max(STREAM_FS)) // STREAM_N) - 1              # the first block with n_b >= W (block 5: 1536 >= 1465)


def stream_input():
    """float32 [24][3][256]: the slab the device calls take."""
    x = EC.make_rows(STREAM_SIGNALS, STREAM_BLOCKS * STREAM_N, STREAM_FS, 44100 + STREAM_N)
    assert TC.no_denormals(x)
    return np.ascontiguousarray(x.reshape(S, STREAM_BLOCKS, STREAM_N).transpose(1, 0, 2))


_SREF = {}


def stream_reference(hold, glide, degrees=STREAM_DEGREES, unvoiced=STREAM_UNVOICED):
    """(period [24][3], ratio [24][3][V]) of the slab in one call, computed once per argument set."""
    k = (hold, glide, degrees, unvoiced)
    if k not in _SREF:
        p, r = HSR.run(stream_input(), STREAM_FS, STREAM_F, np.asarray(degrees, np.int32), STREAM_KEYS,
                       None if unvoiced is None else np.asarray(unvoiced, np.float64), hold, glide)
        p.setflags(write=False)
        r.setflags(write=False)
        _SREF[k] = (p, r)
    return _SREF[k]


def all_partitions(n):
    """Every composition of n blocks into calls would be 2^(n - 1); the CPU test takes these: one call, singles, every split in two,
    and a seeded sample of mixed ones."""
    out = [[n], [1] * n] + [[k, n - k] for k in range(1, n)]
    rng = np.random.default_rng(24)
    for _ in range(12):
        cuts = sorted(set(rng.integers(1, n, size=int(rng.integers(2, 8))).tolist()))
        out.append([b - a for a, b in zip([0] + cuts, cuts + [n])])
    return out


# ---- the musical check: a sharp A3 in C major gets a third and a fifth above it ---------------------------------------------------------
CHORD_FS, CHORD_T, CHORD_KEY, CHORD_DEGREES = 44100.0, 16384, 0, (2, 4)
CHORD_SEG = (4096, 12288)                                                        # the output's middle 8192 samples
CHORD_BIN_HZ = CHORD_FS / (CHORD_SEG[1] - CHORD_SEG[0])                          # one bin of the check's own transform: 5.38 Hz
# the largest distance the NumPy harmonizer (tests/pv_harm_reference.py) leaves between its two maxima and the table's notes, along the
# definition's table: measured on the CPU, recorded in profiles/pv_harmkey_quality.txt (tests/test_pv_harmkey_reference_cpu.py recomputes it)
CHORD_REF_DISTANCE_HZ = 0.0807


def chord_input():
    """float32 [1][16384]: the period-199 voice."""
    return EC.make_rows((("sine_p", P_A3),), CHORD_T, CHORD_FS, 1)


def chord_notes():
    """The table's notes two and four degrees above the note chosen for the voice: 277.18 and 329.63 Hz."""
    return tuple(float(v) for v in HR.voice_ratios(P_A3, CHORD_FS, CHORD_KEY, CHORD_DEGREES) * (CHORD_FS / P_A3))


def chord_peaks(y):
    """The frequencies (Hz, ascending) of the two largest spectral maxima of the middle 8192 samples of y [16384], Hann window, parabolic
    interpolation of the log magnitude."""
    seg = np.asarray(y, np.float64)[CHORD_SEG[0]:CHORD_SEG[1]]
    spec = np.abs(np.fft.rfft(seg * np.hanning(len(seg))))
    loc = [k for k in range(2, len(spec) - 2) if spec[k] > spec[k - 1] and spec[k] >= spec[k + 1]]
    out = []
    for k in sorted(loc, key=lambda k: -spec[k])[:2]:
        a, b, c = np.log(spec[k - 1:k + 2])
        out.append((k + 0.5 * (a - c) / (a - 2 * b + c)) * CHORD_BIN_HZ)
    return tuple(sorted(out))


def chord_tolerance():
    """Twice the distance the definitions leave, or one bin of the check's transform, whichever is larger."""
    return max(2.0 * CHORD_REF_DISTANCE_HZ, CHORD_BIN_HZ)


def chord_reference_distance():
    """The NumPy harmonizer along the definition's table on the CPU -> (its two maxima, the largest distance to the table's notes)."""
    import pv_harm_reference as PH
    x = chord_input()
    _, ratio = HR.track_harmony(x, CHORD_FS, 1024, 256, np.asarray(CHORD_DEGREES, np.int32), [CHORD_KEY])
    y = PH.harmonize(x[0], np.clip(ratio[0], 0.5, 2.0), None, 0.0, 1024, 256)
    got = chord_peaks(y)
    return got, max(abs(g - w) for g, w in zip(got, chord_notes()))
