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

The matrix above advances by hop / 4 .. 2 hop: neither clamp of the advance is ever taken.  EDGE_CASES (tests/test_gpu_pv_stretch_edges.py)
are 48 cases of SIX streams whose tables reach both clamps of the advance, both clamps of the position and every alignment of a frame's
address: edge_positions() says which row reaches what.  The bound is the same.
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


# ---- the advance clamps and the table edges: 48 cases of six streams ---------------------------------------------------------------------
EDGE_STREAMS = 6
EDGE_ROWS = ("freeze", "reverse", "crawl", "leap", "ends", "skew")
EDGE_SHAPES = ((19, 3), (6, 2), (2, 0))                                    # (nF, extra)
EDGE_SEMITONES = (0.0, 7.0)
EDGE_CASES = [StretchCase(F, hop, nF, extra, v) for F in (1024, 2048) for hop in HOPS[F] for nF, extra in EDGE_SHAPES for v in EDGE_SEMITONES]
assert len(EDGE_CASES) == 48
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _cycled(first, incs, nF):
    return np.concatenate([[first], first + np.cumsum([incs[i % len(incs)] for i in range(nF - 1)], dtype=np.int64)]).astype(np.int64)


def _leap(c):
    return _cycled(0, (c.F, c.F + 1, c.F - 1, 2 * c.F + 3), c.nF)


def edge_in_length(c):
    """F + max(leap) + 1, raised to the next value = 3 (mod 4): the six row starts s n_in sit at residues 0, 3, 2, 1, 0, 3."""
    n = c.F + int(_leap(c).max()) + 1
    return n + (3 - n) % 4


def edge_positions(c, n_in=None):
    """int64 [EDGE_STREAMS][nF] (the wrapper makes them int32), with qm = n_in - F:
      0 freeze   3 hop + 1 at every frame                            raw step 0 -> D = 1; the phase difference is exactly 0
      1 reverse  (nF - 1 - f) hop + 2                                negative steps -> D = 1
      2 crawl    0, then increments cycling 1, 2, 3                  D = 1, 2, 3 unclamped; F / D up to F
      3 leap     0, then increments cycling F, F + 1, F - 1, 2 F + 3 D = F exactly, clamped from F + 1 and from 2 F + 3, and F - 1
      4 ends     cycling -1, qm + 1, qm, -2^31, 2^31 - 1, 0, qm - 1, 1   both clamps of q, steps of +-qm and 0 between them
      5 skew     1 + f (hop + 1)                                     frame addresses walk every residue mod 4"""
    n_in = edge_in_length(c) if n_in is None else n_in
    qm = n_in - c.F
    f = np.arange(c.nF, dtype=np.int64)
    ends = np.array([-1, qm + 1, qm, INT_MIN, INT_MAX, 0, qm - 1, 1], np.int64)
    return np.stack([np.full(c.nF, 3 * c.hop + 1, np.int64), (c.nF - 1 - f) * c.hop + 2, _cycled(0, (1, 2, 3), c.nF), _leap(c), ends[f % 8],
                     1 + f * (c.hop + 1)])


def edge_rows(x5):
    """Stream s of an edge case takes row s % 5 of a five-stream signal."""
    return np.ascontiguousarray(x5[[s % 5 for s in range(EDGE_STREAMS)]])


def edge_input(c, n_in=None):
    return edge_rows(pv_cases.mixed_streams(edge_in_length(c) if n_in is None else n_in, seed=c.hop + 7))


def edge_reference(c, form="radians", advance="delta", n_in=None, rows=range(EDGE_STREAMS)):
    """{stream: [T] float64} of the streams in rows, each computed once per case, form, advance (a mutant of pv_stretch_reference.ADVANCES)
    and input length (None: the case's; the smallest-input tests give their own, and the tables are then built against it).  Callers do
    not write to them."""
    x = pos = None
    out = {}
    for s in rows:
        key = ("edge", c, form, advance, n_in, s)
        if key not in _REF:
            if x is None:
                x, pos = edge_input(c, n_in), edge_positions(c, n_in)
            r = SR.stretch_roundtrip(x[s], pos[s], out_length(c), c.F, c.hop, pv_cases.ratio_of(c.semitones), form, advance)
            r.setflags(write=False)
            _REF[key] = r
        out[s] = _REF[key]
    return out


# ---- the smallest inputs: n_in = F (qm = 0: every table is freeze at 0) and n_in = F + 1 (positions 0 and 1 only), the case's own tables --
SMALL_CASES = [(StretchCase(F, 256, 6, 2, v), F + more) for F in (1024, 2048) for more in (0, 1) for v in EDGE_SEMITONES]


def small_id(cn):
    return f"{case_id(cn[0])}-n_in{cn[1]}"
