"""The time-stretch test matrix (vp_stft_time_stretch): the cases that tests/test_pv_stretch_reference_cpu.py (conditioning gate, teeth)
and tests/test_gpu_pv_stretch.py (kernels against NumPy) BOTH iterate.  Test infrastructure only.  The reference is
tests/pv_stretch_reference.py.

96 cases of five streams: both frame lengths at every hop; six shapes (nF, extra) of the OUTPUT row T = F + (nF - 1) hop + extra -- last
rounds of 3, 4, 1, 2, 1 and 2 frames, odd T, the longest tail --; a pure stretch (0 semitones) and one of pv_cases.SEMITONES, cycled over
the cases.  Stream s analyses its frames at its own positions: streams 0-3 at floor(f hop / a) for a = 0.5, 0.8, 1.37 and 4, stream 4 with
increments that glide from 2 hop to hop / 4 (odd and even advances).  The input rows are n_in = F + max(pos) + 1 samples, odd for
nF = 19 and 5.

Bound of the pointwise comparisons: pv_cases.bound's derivation (double transforms and stage, float32 output frames and a float32
overlap-add of O = F / hop terms), in which nothing depends on the positions:
    |y - ref| <= 4 O 2^-24 max(1, max |ref|)       at every sample.
"""
from collections import namedtuple

import numpy as np

import pv_cases
import pv_curve_cases
import pv_stretch_reference as SR

N_STREAMS = 5
HOPS = pv_curve_cases.HOPS
SHAPES = ((19, 3), (4, 0), (1, "hop-1"), (2, 0), (5, "hop-1"), (6, 2))       # (nF, extra)
FACTORS = (0.5, 0.8, 1.37, 4.0)                                            # streams 0-3: pos[f] = floor(f hop / a)
GATE_TOL = pv_cases.GATE_TOL                # the two forms of the reference, relative to max(1, max |ref|)
TEETH = pv_curve_cases.TEETH                # a reference that is off by a frame / an advance differs by more than TEETH x bound

StretchCase = namedtuple("StretchCase", "F hop nF extra semitones")


def _cases():
    out, i = [], 0
    for F in (1024, 2048):
        for hop in HOPS[F]:
            for nF, extra in SHAPES:
                ex = hop - 1 if extra == "hop-1" else extra
                out += [StretchCase(F, hop, nF, ex, 0.0), StretchCase(F, hop, nF, ex, pv_cases.SEMITONES[i % len(pv_cases.SEMITONES)])]
                i += 1
    return out


CASES = _cases()
assert len(CASES) == 96


def case_id(c):
    return f"F{c.F}-hop{c.hop}-nF{c.nF}+{c.extra}-{c.semitones:+g}st"


def out_length(c):
    return c.F + (c.nF - 1) * c.hop + c.extra


def bound(c, ref):
    return 4.0 * (c.F // c.hop) * 2.0 ** -24 * max(1.0, float(np.abs(ref).max()))


def positions(c):
    """int32 [N_STREAMS][nF]."""
    f = np.arange(c.nF, dtype=np.int64)
    rows = [np.floor(f * c.hop / a).astype(np.int64) for a in FACTORS]
    steps = np.rint(np.linspace(2.0 * c.hop, c.hop / 4.0, max(c.nF - 1, 0))).astype(np.int64)
    rows.append(np.concatenate([[0], np.cumsum(steps)]))
    return np.stack(rows).astype(np.int32)


def in_length(c):
    n = c.F + int(positions(c).max()) + 1
    return n + 1 if c.nF in (19, 5) and n % 2 == 0 else n


def case_input(c):
    return pv_cases.mixed_streams(in_length(c), seed=c.hop + 5)


def rolled(pos):
    return np.roll(pos, 1, axis=-1)


_REF = {}


def reference(c, form="radians", variant=None):
    """[N_STREAMS][T] float64, computed once per case, form and variant (callers do not write to it).  variant "roll": every stream's table
    rolled by one frame (what a kernel that reads its neighbour frame's position would compute); "hop": a stage that unwraps with hop
    instead of the frame's advance."""
    key = (c, form, variant)
    if key not in _REF:
        x, pos = case_input(c), positions(c)
        if variant == "roll":
            pos = rolled(pos)
        ref = np.stack([SR.stretch_roundtrip(x[s], pos[s], out_length(c), c.F, c.hop, pv_cases.ratio_of(c.semitones), form,
                                             "hop" if variant == "hop" else "delta") for s in range(N_STREAMS)])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


# ---- more workgroups than compute units: 300 streams, every stream its own constant stretch from [0.25, 4], a pure stretch -------------
BIG_S = 300
BIG_CHECKED = (0, 1, 255, 256, 299)
BIG_F, BIG_HOP, BIG_NF = 1024, 256, 19
BIG_T = BIG_F + (BIG_NF - 1) * BIG_HOP + 3
BIG_N_IN = BIG_F + (BIG_NF - 1) * BIG_HOP * 4 + 1                          # room for the slowest stream (stretch 0.25), odd


def big_stretch():
    return np.random.default_rng([BIG_HOP, 11]).uniform(0.25, 4.0, BIG_S)


def big_positions():
    return np.stack([SR.stretch_positions(BIG_NF, BIG_HOP, a, BIG_N_IN, BIG_F) for a in big_stretch()])


def big_input():
    return pv_cases.harmonic_streams(BIG_S, BIG_N_IN, seed=BIG_HOP + 3)


def big_reference(form="radians", variant=None):
    """{stream: [T] float64} for BIG_CHECKED."""
    key = ("big", form, variant)
    if key not in _REF:
        x, pos = big_input(), big_positions()
        if variant == "roll":
            pos = rolled(pos)
        _REF[key] = {s: SR.stretch_roundtrip(x[s], pos[s], BIG_T, BIG_F, BIG_HOP, 1.0, form, "hop" if variant == "hop" else "delta")
                     for s in BIG_CHECKED}
    return _REF[key]
