"""The fine pitch trackers' device cases: what tests/test_pv_track_fine_reference_cpu.py (branch coverage, on the definition) and
tests/test_gpu_pv_track_fine.py (bit equality with tests/pv_track_fine_reference.py and tests/pv_track_fine_stream_reference.py) BOTH
iterate.  Test infrastructure only.  Three streams per batch case, three keys per case, no float32 denormal and no non-finite sample.

Every branch of the rule must be reached at least MIN_PER_BRANCH times (the CPU file asserts it):
  refined      pv_track_edge_cases.CASES by import (the tiled rows refine around an exact zero of d'), and 0.5-amplitude sines whose
               period lies tau0 - 0.4 .. tau0 + 0.5 samples: the walk stays at tau0 and the parabola moves the period to either side;
  edge         the edge cases' rows whose period is tauMax - 1: the guard slot would be the right neighbour;
  left_lower   0.5-amplitude sines of period tau0 - 0.8 and tau0 - 0.6: the pitch lies above fMax, the walk starts at tau0 on the far
               side of the minimum, so d'[tau0 - 1] < d'[tau0] -- at 44.1 kHz / 1024 / 256, 48 kHz / 2048 / 512 and 8 kHz / 1024 / 256;
  unvoiced     the edge cases' silent, DC, impulse and over-long-period rows.
Lengths: "clamp" is F + tauMax + 3 hop + 17 samples, "min" exactly F + tauMax (one frame), "three" F + 2 hop + 5 (three frames: 3 streams
x 3 frames is no multiple of the four frames a workgroup holds, so the last workgroup's other wavefronts leave early)."""
from collections import namedtuple

import numpy as np

import pv_track_cases as TC
import pv_track_edge_cases as EC
import pv_track_fine_reference as FR
import pv_track_fine_stream_reference as FSR
import pv_track_reference as R

N_STREAMS = 3
MIN_PER_BRANCH = 4
FineCase = namedtuple("FineCase", "name fs F hop length signals keys")
SINE_GEOMETRIES = ((44100.0, 1024, 256), (48000.0, 2048, 512), (8000.0, 1024, 256))
LEFT_OFFSETS = (-0.8, -0.6)
REFINE_OFFSETS = (-0.4, -0.2, 0.0, 0.1, 0.3, 0.5)


def half_sine(period, n):
    """0.5 sin with a period of `period` samples."""
    return (0.5 * np.sin(2.0 * np.pi * np.arange(n) / period + 0.3)).astype(np.float32)


def _sine_cases():
    out = []
    for gi, (fs, F, hop) in enumerate(SINE_GEOMETRIES):
        t0 = R.tau_min(fs)
        for ln in ("clamp", "min"):
            out.append(FineCase(f"left-fs{int(fs)}-F{F}-{ln}", fs, F, hop, ln, (("half_sine", t0 + LEFT_OFFSETS[0]), ("half_sine", t0 + LEFT_OFFSETS[1]),
                                                                                ("half_sine", t0 + LEFT_OFFSETS[0])), TC.KEY_SETS[(gi + 3) % 5]))
            for i in (0, 3):
                trio = tuple(("half_sine", t0 + o) for o in REFINE_OFFSETS[i:i + 3])
                out.append(FineCase(f"near-fs{int(fs)}-F{F}-{ln}-{i}", fs, F, hop, ln, trio, TC.KEY_SETS[(gi + i) % 5]))
    return out


LEFT_AND_NEAR = _sine_cases()
THREE_BY_THREE = FineCase("three-by-three", 44100.0, 1024, 256, "three", (("half_sine", 54.2), ("tc", "saw"), ("half_sine", 200.37)), (-1, 13, 12))
NULL_KEYS = FineCase("null-keys", 44100.0, 1024, 256, "clamp", (("tc", "sine_off"), ("tc", "vibrato"), ("half_sine", 75.3)), None)
EDGE = [FineCase(c.name, c.fs, c.F, c.hop, c.length, c.signals, c.keys) for c in EC.CASES]
CASES = EDGE + LEFT_AND_NEAR + [THREE_BY_THREE, NULL_KEYS]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert any(k is not None and (min(k) < 0 or max(k) > 12) for k in (c.keys for c in CASES))     # keys outside 0 .. 12 are covered


def case_id(c):
    return c.name


def length(c):
    tm = R.tau_max(c.fs)
    return {"min": c.F + tm, "clamp": c.F + tm + 3 * c.hop + 17, "three": c.F + 2 * c.hop + 5}[c.length]


def batch_input(c):
    """float32 [3][T]"""
    n, seed = length(c), int(c.fs) + c.hop
    x = np.stack([half_sine(sp[1], n) if sp[0] == "half_sine" else EC.edge_signal(sp, n, c.fs, seed) for sp in c.signals])
    assert x.dtype == np.float32 and TC.no_denormals(x) and np.all(np.isfinite(x)), c.name
    return x


_REF = {}


def reference(c):
    """(period, period_fine, ratio, branches [3][nF]) of the case, computed once (callers do not write to it)."""
    if c.name not in _REF:
        br = []
        p, pf, r = FR.track_fine(batch_input(c), c.fs, c.F, c.hop, c.keys, branches=br)
        for a in (p, pf, r):
            a.setflags(write=False)
        _REF[c.name] = (p, pf, r, br)
    return _REF[c.name]


def branch_counts(cases):
    out = dict.fromkeys(FR.BRANCHES, 0)
    for c in cases:
        for row in reference(c)[3]:
            for b in row:
                out[b] += 1
    return out


# ---- streaming: N = 64, 256 and 1000 at 44.1 kHz / 1024, the ring fills inside the run ------------------------------------------------------
StreamCase = namedtuple("StreamCase", "name fs F N n_blocks signals keys hold glide")
_T0 = R.tau_min(44100.0)
_FIVE = (("half_sine", _T0 - 0.8), ("half_sine", _T0 + 0.3), ("tc", "saw"), ("tone_zeros", 5200), ("tiled", R.tau_max(44100.0) - 1))
STREAM_CASES = [
    StreamCase("n64", 44100.0, 1024, 64, 30, _FIVE, (12, 0, 7, 12, -1), 0, 1.0),
    StreamCase("n256-hold8-glide", 44100.0, 1024, 256, 30, _FIVE, (0, 12, 12, 7, 13), 8, 0.5),
    StreamCase("n1000-glide", 44100.0, 1024, 1000, 10, _FIVE, (12, 12, 0, 12, 7), 0, 0.5),
]


def stream_input(c):
    """float32 [n_blocks][S][N]: the slab the device calls take."""
    n, seed = c.n_blocks * c.N, int(c.fs) + c.N
    x = np.stack([half_sine(sp[1], n) if sp[0] == "half_sine" else EC.edge_signal(sp, n, c.fs, seed) for sp in c.signals])
    assert x.dtype == np.float32 and TC.no_denormals(x) and np.all(np.isfinite(x)), c.name
    return np.ascontiguousarray(x.reshape(len(c.signals), c.n_blocks, c.N).transpose(1, 0, 2))


def stream_groupings(c):
    """Three ways to cut the case's blocks into calls."""
    n = c.n_blocks
    mixed, pat, i = [], (3, 1, 4, 2), 0
    while sum(mixed) < n:
        mixed.append(min(pat[i % len(pat)], n - sum(mixed)))
        i += 1
    return {"single": [1] * n, "whole": [n], "mixed": mixed}


_SREF = {}


def stream_reference(c):
    """(period [n][S], period_fine [n][S], followed ratio [n][S]) of the case in one call, computed once."""
    if c.name not in _SREF:
        out = FSR.run(stream_input(c), c.fs, c.F, c.keys, c.hold, c.glide)
        for a in out:
            a.setflags(write=False)
        _SREF[c.name] = out
    return _SREF[c.name]
