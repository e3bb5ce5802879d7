"""The ratio-curve test matrix (vp_stft_pitch_shift_curve, vp_pv_process_blocks_curve_device): the cases that
tests/test_pv_curve_reference_cpu.py (conditioning gate, teeth) and tests/test_gpu_pv_curve.py (kernels against NumPy) BOTH iterate, and
the reference of a time-varying ratio.  Test infrastructure only.

The reference is the definition tests/pv_stream_reference.py already gives ("the ratio schedule is per frame"): a loop over
PvStreamRef._frame(x[f hop : f hop + F], f, ratio[f]) with overlap-add and the 1 / sum w^2 scale -- stft_reference.stft_roundtrip with
`ratio` replaced by ratio[f] in frame f (on a constant curve the loop equals stft_roundtrip bit for bit: tested on the CPU).  Its second
form is the same loop over pv_cases.PvStreamTurns._frame (phases in turns).

Bound of the pointwise comparisons: pv_cases.bound's derivation (double transforms and stage, float32 output frames and a float32
overlap-add of O = F / hop terms), in which nothing depends on the ratio:
    |y - ref| <= 4 O 2^-24 max(1, max |ref|)       at every sample.
"""
from collections import namedtuple

import numpy as np

import pv_cases
import pv2k_cases
import pv_stream_reference as P

N_STREAMS = 5
HOPS = {1024: pv_cases.HOPS, 2048: pv2k_cases.HOPS}
N_FRAMES = (19, 4)                          # last round of 3 frames, odd T, a tail of 3 | exactly one round, aligned, no tail
CURVES = ("glide", "vibrato", "steps", "octaves")
GATE_TOL = 1e-9                             # the two forms of the reference, relative to max(1, max |ref|)
TEETH = 100.0                               # the reference with the curve rolled by a frame differs by more than TEETH x bound

CurveCase = namedtuple("CurveCase", "F hop nF curve")
CASES = [CurveCase(F, hop, nF, c) for F in (1024, 2048) for hop in HOPS[F] for nF in N_FRAMES for c in CURVES]
assert len(CASES) == 64


def case_id(c):
    return f"F{c.F}-hop{c.hop}-nF{c.nF}-{c.curve}"


def length(c):
    return c.F + (c.nF - 1) * c.hop + (3 if c.nF == 19 else 0)


def bound(c, ref):
    return 4.0 * (c.F // c.hop) * 2.0 ** -24 * max(1.0, float(np.abs(ref).max()))


def case_input(c):
    return pv_cases.mixed_streams(length(c), seed=c.hop + 5)


def semitones_of(c):
    """[N_STREAMS][nF] float64, every value in [-12, 12]."""
    nF, f = c.nF, np.arange(c.nF, dtype=np.float64)
    st = np.zeros((N_STREAMS, nF))
    for s in range(N_STREAMS):
        if c.curve == "glide":
            st[s] = (-12.0 + 24.0 * f / (nF - 1)) * (-1.0 if s & 1 else 1.0)
        elif c.curve == "vibrato":
            st[s] = np.clip((7.0 - 3.0 * s) + 0.5 * np.sin(2.0 * np.pi * f / 9.0 + s), -12.0, 12.0)
        elif c.curve == "steps":
            st[s] = np.random.default_rng([c.hop, s, 9]).uniform(-12.0, 12.0, nF)
        elif c.curve == "octaves":
            st[s] = np.where((np.arange(nF) // 3) & 1, 12.0, -12.0)
        else:
            raise KeyError(c.curve)
    return st


def ratios_of(c):
    return pv_cases.ratio_of(semitones_of(c))


def frame_loop(x, F, hop, ratio, form="radians"):
    """One stream: x float [T], ratio [nFrames] -> float64 [T]."""
    cls = P.PvStreamRef if form == "radians" else pv_cases.PvStreamTurns
    r = cls(F, hop, F)                      # (the block size plays no part in _frame)
    x = np.asarray(x, np.float64)
    nF = (len(x) - F) // hop + 1
    assert len(ratio) == nF
    y = np.zeros(len(x))
    for f in range(nF):
        y[f * hop:f * hop + F] += r._frame(x[f * hop:f * hop + F], f, float(ratio[f]))
    return y * r.scale


_REF = {}


def reference(c, form="radians", roll=0):
    """[N_STREAMS][T] float64, computed once per case, form and roll (callers do not write to it).  roll = 1: every stream's curve rolled
    by one frame (np.roll(ratio, 1)) -- what a kernel that reads its neighbour frame's ratio would compute."""
    key = (c, form, roll)
    if key not in _REF:
        x, ratio = case_input(c), ratios_of(c)
        ref = np.stack([frame_loop(x[s], c.F, c.hop, np.roll(ratio[s], roll), form) for s in range(N_STREAMS)])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]
