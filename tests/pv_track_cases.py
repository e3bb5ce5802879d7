"""The pitch tracker's case table (vp_stft_track_pitch, vp_stft_autotune): what tests/test_pv_track_reference_cpu.py (conditioning,
teeth, closed loop) and tests/test_gpu_pv_track.py (bit equality with tests/pv_track_reference.py) BOTH iterate.  Test infrastructure
only.  Three streams per case, rows of a few thousand samples, seeded; the reference of a case is computed once and shared.

A case is a geometry (fs, F, hop), a row length, a group of three signals and a key per stream; every geometry meets every row length and
every signal group, the key sets rotate through them.

No sample of any signal is a float32 denormal (the tracker's definition leaves those out): case_input asserts it."""
from collections import namedtuple

import numpy as np

import pv_track_reference as R

N_STREAMS = 3
# (fs, F, hop); the last one has tauMax = 512: every lag slot of the kernel is in use
GEOMETRIES = ((44100.0, 1024, 256), (44100.0, 1024, 64), (44100.0, 1024, 512), (48000.0, 2048, 512), (8000.0, 1024, 128), (51200.0, 1024, 256))
# "min": T = F + tauMax exactly (every window at b = 0); "clamp": T off the hop grid, the last frames clamped; "long": 23 frames
LENGTHS = ("min", "clamp", "long")
LONG_FRAMES = 23
SIGNAL_GROUPS = (("sine_on", "sine_off", "saw"), ("glide", "vibrato", "noise"), ("silence", "gap", "sine_100_2"),
                 ("sine_90", "sine_900", "sine_tiny"), ("square", "sine_edge", "noise"))
# per stream; -1 and 13 are out of range and count as 12
KEY_SETS = ((12, 12, 12), (0, 0, 0), (7, 7, 7), (0, 7, 12), (-1, 13, 12))

TrackCase = namedtuple("TrackCase", "fs F hop length group keys")
CASES = [TrackCase(fs, F, hop, ln, grp, KEY_SETS[(gi + li + si) % len(KEY_SETS)])
         for gi, (fs, F, hop) in enumerate(GEOMETRIES) for li, ln in enumerate(LENGTHS) for si, grp in enumerate(SIGNAL_GROUPS)]
assert len(CASES) == 90 and len({(c.group, c.keys) for c in CASES}) == 25       # every signal group meets every key set


def case_id(c):
    return f"fs{int(c.fs)}-F{c.F}-hop{c.hop}-{c.length}-{c.group[0]}+{c.group[1]}+{c.group[2]}-keys{'_'.join(str(k) for k in c.keys)}"


def length(c):
    tm = R.tau_max(c.fs)
    if c.length == "min":
        return c.F + tm
    if c.length == "clamp":
        return c.F + tm + 3 * c.hop + 17
    T = c.F + (LONG_FRAMES - 1) * c.hop + 5
    assert T >= c.F + tm
    return T


def signal(name, n, fs, seed):
    """float64 [n]; frequencies in Hz whatever fs is (at 8 kHz some of them lie outside the tracker's lag range: that is a case too)."""
    t = np.arange(n) / fs
    rng = np.random.default_rng([seed, sum(name.encode())])
    two_pi = 2.0 * np.pi
    if name == "sine_on":
        return 0.8 * np.sin(two_pi * 220.0 * t + 0.3)
    if name == "sine_off":
        return 0.3 * np.sin(two_pi * 227.0 * t + 0.7)
    if name == "saw":
        ph = 330.5 * t + 0.21
        return 0.5 * (2.0 * (ph - np.floor(ph)) - 1.0) + 0.4 * np.sin(two_pi * ph)
    if name == "glide":
        f = 200.0 + 60.0 * np.arange(n) / max(n - 1, 1)
        return 0.7 * np.sin(two_pi * np.cumsum(f) / fs + 0.1)
    if name == "vibrato":
        # +-60 cents around the boundary between 220 Hz and the semitone above it
        f = 220.0 * 2.0 ** (0.5 / 12.0) * 2.0 ** (0.6 / 12.0 * np.sin(two_pi * 20.0 * t))
        return 0.6 * np.sin(two_pi * np.cumsum(f) / fs + 0.4)
    if name == "noise":
        return 0.5 * rng.standard_normal(n)
    if name == "silence":
        return np.zeros(n)
    if name == "gap":
        y = 0.7 * np.sin(two_pi * 196.0 * t + 0.2)
        y[n // 3:2 * n // 3] = 0.0
        return y
    if name == "sine_100_2":
        return 0.8 * np.sin(two_pi * 100.2 * t + 0.5)
    if name == "sine_90":
        return 0.8 * np.sin(two_pi * 90.0 * t + 0.9)
    if name == "sine_900":
        return 0.8 * np.sin(two_pi * 900.0 * t + 0.6)
    if name == "sine_tiny":
        return 1e-30 * np.sin(two_pi * 262.0 * t + 0.37)
    if name == "square":
        return np.where(np.sin(two_pi * 147.0 * t + 0.45) >= 0.0, 1.0, -1.0)
    if name == "sine_edge":
        # a period just above tauMax - 1 samples: the first lag under the tolerance is among the last the walk may start from
        return 0.8 * np.sin(two_pi * (fs / (R.tau_max(fs) + EDGE_EXCESS)) * t + 1.1)
    raise KeyError(name)


EDGE_EXCESS = 12.0       # samples by which sine_edge's period exceeds tauMax


def no_denormals(x):
    a = np.abs(np.asarray(x, np.float32))
    return bool(np.all((a == 0) | (a >= np.finfo(np.float32).tiny)))


def make_input(names, n, fs, seed):
    x = np.stack([signal(nm, n, fs, seed) for nm in names]).astype(np.float32)
    assert no_denormals(x), names
    return x


def case_input(c):
    """float32 [3][T]"""
    return make_input(c.group, length(c), c.fs, int(c.fs) + c.hop + len(c.length))


_REF = {}


def reference(c):
    """(period int32 [3][nF], ratio float64 [3][nF]) of the case, computed once (callers do not write to it)."""
    if c not in _REF:
        p, r = R.track(case_input(c), c.fs, c.F, c.hop, c.keys)
        p.setflags(write=False)
        r.setflags(write=False)
        _REF[c] = (p, r)
    return _REF[c]


# ---- the steady cases of the closed loop: tracker -> phase-vocoder shift along its ratios -> tracker -------------------------------------
# (name, frequency, key): the corrected signal's period must lie within one sample of fs / closestFreq on every frame
STEADY_FS, STEADY_F, STEADY_HOP, STEADY_FRAMES = 44100.0, 1024, 256, 21
STEADY = (("sine", 227.0, 12), ("sine", 227.0, 0), ("saw", 330.5, 12), ("sine", 205.0, 12))
STEADY_T = STEADY_F + (STEADY_FRAMES - 1) * STEADY_HOP + R.tau_max(STEADY_FS)


def steady_input():
    """float32 [4][STEADY_T] and the keys [4]"""
    t = np.arange(STEADY_T) / STEADY_FS
    rows = []
    for kind, f, _ in STEADY:
        if kind == "sine":
            rows.append(0.6 * np.sin(2.0 * np.pi * f * t + 0.3))
        else:
            ph = f * t + 0.21
            rows.append(0.5 * (2.0 * (ph - np.floor(ph)) - 1.0) + 0.4 * np.sin(2.0 * np.pi * ph))
    x = np.stack(rows).astype(np.float32)
    assert no_denormals(x)
    return x, [k for _, _, k in STEADY]


def covered_part(y, F, hop):
    """The samples of a phase-vocoder output that lie under the full overlap of F / hop frames.  The first and last F - hop samples of
    what the frames cover are sums of fewer windows than the 1 / sum w^2 scale assumes (an amplitude ramp and, over the first frames, a
    phase still settling): they are not the corrected signal, and the closed loop does not track them.  (With them, stream 1 below gives
    199 on its first and last two frames against 200.45.)"""
    end = (R.n_frames(len(y), F, hop) - 1) * hop + F
    return y[F - hop:end - (F - hop)]


def steady_targets():
    """fs / closestFreq per steady stream (samples)."""
    from oracle import oracle_py as O
    return [STEADY_FS / O.notes_closest(f, k) for _, f, k in STEADY]
