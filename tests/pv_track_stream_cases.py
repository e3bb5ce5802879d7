"""The streaming pitch tracker's case table (vp_pv_tracker_*): what tests/test_pv_track_stream_reference_cpu.py (conditioning, teeth,
closed loop) and tests/test_gpu_pv_track_stream.py (bit equality with tests/pv_track_stream_reference.py) BOTH iterate.  Test
infrastructure only.  The signals are pv_track_cases.signal's; the reference of a case is computed once and shared.

A case is a geometry (fs, F, N), a number of blocks that passes W = F + tauMax by at least six decisions, three to six signals with a key
each, and the follow parameters (hold, glide).  Every block size meets the way it relates to W:
  N = 64     a window spans 23 blocks: ring and slab are mixed in one window over many calls;
  N = 256    the everyday size; carries the hold and glide cases on a stream with a gap;
  N = 1000   no alignment, no power of two;
  N = 1024   N < W < 2 N;
  N = 4096   N > W: the ring is never read, and its rewrite takes the tail of the call's last block."""
from collections import namedtuple

import numpy as np

import pv_track_cases as TC
import pv_track_stream_reference as SR

StreamCase = namedtuple("StreamCase", "name fs F N n_blocks signals keys hold glide")

_SIX = ("sine_on", "sine_off", "saw", "vibrato", "gap", "noise")
CASES = [
    StreamCase("n64", 44100.0, 1024, 64, 40, _SIX, (12, 0, 7, 12, 12, 12), 0, 1.0),
    StreamCase("n256-hold3", 44100.0, 1024, 256, 40, _SIX, (12, 12, 0, 7, 12, 0), 3, 1.0),          # the gap outlasts the hold: it expires
    StreamCase("n256-hold1000", 44100.0, 1024, 256, 40, _SIX, (12, 12, 0, 7, 12, 0), 1000, 1.0),    # ... and here it does not
    StreamCase("n256-glide", 44100.0, 1024, 256, 40, _SIX, (12, 12, 0, 7, 12, 0), 2, 0.5),
    StreamCase("n1000", 51200.0, 1024, 1000, 10, ("sine_off", "square", "sine_edge"), (-1, 13, 0), 0, 1.0),
    StreamCase("n1024", 8000.0, 1024, 1024, 8, ("sine_on", "glide", "noise", "sine_100_2"), (12, 7, 12, 0), 1, 0.25),
    StreamCase("n1024-44k", 44100.0, 1024, 1024, 9, ("saw", "vibrato", "sine_tiny", "silence", "glide"), (0, 12, 12, 12, 7), 0, 1.0),
    StreamCase("n4096", 48000.0, 2048, 4096, 7, ("sine_off", "saw", "gap"), (12, 0, 12), 1, 0.5),
]
BY_NAME = {c.name: c for c in CASES}
assert {c.N for c in CASES} == {64, 256, 1000, 1024, 4096}
assert {(c.fs, c.F) for c in CASES} == {(44100.0, 1024), (51200.0, 1024), (8000.0, 1024), (48000.0, 2048)}
assert all(3 <= len(c.signals) <= 6 and len(c.keys) == len(c.signals) for c in CASES)


def case_id(c):
    return c.name


def window(c):
    return SR.window_len(c.fs, c.F)


def first_decision(c):
    """The first block whose end reaches W samples."""
    return -(-window(c) // c.N) - 1


assert all(c.n_blocks - first_decision(c) >= 6 for c in CASES), [(c.name, c.n_blocks - first_decision(c)) for c in CASES]


def case_input(c):
    """float32 [n_blocks][S][N]: the slab the device calls take."""
    T = c.n_blocks * c.N
    x = TC.make_input(c.signals, T, c.fs, int(c.fs) + c.N)
    return np.ascontiguousarray(x.reshape(len(c.signals), c.n_blocks, c.N).transpose(1, 0, 2))


def rows(blocks):
    """[n][S][N] -> the streams' signals [S][n N]."""
    n, S, N = blocks.shape
    return np.ascontiguousarray(blocks.transpose(1, 0, 2).reshape(S, n * N))


_REF = {}


def reference(c):
    """(period int32 [n_blocks][S], followed ratio float64 [n_blocks][S]) of the case in one call, computed once (callers do not write to it)."""
    if c not in _REF:
        p, r = SR.run(case_input(c), c.fs, c.F, c.keys, c.hold, c.glide)
        p.setflags(write=False)
        r.setflags(write=False)
        _REF[c] = (p, r)
    return _REF[c]


def groupings(c):
    """Ways to cut the case's blocks into calls: one block per call, all in one, a mixed pattern -- and, where a window spans many blocks,
    first calls that end just below and just above W samples."""
    n = c.n_blocks
    out = {"single": [1] * n, "whole": [n]}
    mixed, pat, i = [], (3, 1, 4, 2), 0
    while sum(mixed) < n:
        mixed.append(min(pat[i % len(pat)], n - sum(mixed)))
        i += 1
    out["mixed"] = mixed
    fd = first_decision(c)
    if fd >= 2:
        out["below-W"] = [fd, 1, n - fd - 1]               # the first call's fd N samples stay below W: the next block's window is ring + slab
        out["above-W"] = [fd + 1, n - fd - 1]              # the first call passes W by itself
    return out
