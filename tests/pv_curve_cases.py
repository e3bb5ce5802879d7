"""The ratio-curve test matrix (vp_stft_pitch_shift_curve, vp_pv_process_blocks_curve_device): the cases that
tests/test_pv_curve_reference_cpu.py (conditioning gate, teeth) and tests/test_gpu_pv_curve.py / tests/test_gpu_pv_curve_edges.py (kernels
against NumPy) BOTH iterate, and the reference of a time-varying ratio.  Test infrastructure only.  CASES is the first matrix; the lists
behind it (EDGE_CASES, STREAM_CURVE_CASES, CURVE_SCENARIOS, BIG_LEGS) are the edges the fixed-interval kernels are tested at.

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


# ---- the edges of the one-shot curve kernels ----------------------------------------------------------------------------------------------
# Last rounds of one and two frames, the one- and two-frame signals and the longest tail (hop - 1 samples no frame covers), which CASES
# (last rounds of three and four frames) leaves out.  "glide" divides by nF - 1 and "octaves" is constant over so few frames: "glide" and
# "steps" from two frames on, "steps" alone on one frame.
EdgeCase = namedtuple("EdgeCase", "F hop nF extra curve")
EDGE_FRAMES = ((1, "hop-1"), (2, 0), (5, "hop-1"), (6, 2))       # (nF, extra): the last round holds 1, 2, 1 and 2 frames
EDGE_CASES = [EdgeCase(F, hop, nF, hop - 1 if extra == "hop-1" else extra, c) for F in (1024, 2048) for hop in HOPS[F]
              for nF, extra in EDGE_FRAMES for c in (("glide", "steps") if nF >= 2 else ("steps",))]
assert len(EDGE_CASES) == 56


def edge_id(c):
    return f"F{c.F}-hop{c.hop}-nF{c.nF}+{c.extra}-{c.curve}"


def edge_length(c):
    return c.F + (c.nF - 1) * c.hop + c.extra


def edge_input(c):
    return pv_cases.mixed_streams(edge_length(c), seed=c.hop + 5)


def edge_reference(c, form="radians", off=False):
    """[N_STREAMS][T] float64, computed once per case, form and off (callers do not write to it).  off: the curve one step off -- rolled
    by a frame (np.roll(ratio, 1)) from two frames on; on one frame, where a roll changes nothing, stream s with stream s + 1's ratio
    (what a kernel that reads its neighbour row would compute)."""
    key = (c, form, off)
    if key not in _REF:
        x, ratio = edge_input(c), ratios_of(c)
        if off:
            ratio = np.roll(ratio, 1, axis=1) if c.nF >= 2 else np.roll(ratio, -1, axis=0)
        ref = np.stack([frame_loop(x[s], c.F, c.hop, ratio[s], form) for s in range(N_STREAMS)])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


# ---- the streaming curve kernel against NumPy -----------------------------------------------------------------------------------------------
# pv_cases.STREAM_CASES' block sizes (N = 17 and 64: calls without a frame; N = 4096: many rounds in a call) at every hop, every block
# and stream its own interval.  The reference is the restatement driven ONE BLOCK AT A TIME with that block's ratio: a frame is computed
# in the block in which its last sample arrives.
StreamCurveCase = namedtuple("StreamCurveCase", "hop N n_blocks")
STREAM_CURVE_HOPS = (64, 128, 256, 512)
STREAM_CURVE_CALLS = (1, 3, 16, 4)
STREAM_CURVE_CASES = [StreamCurveCase(hop, N, max(-(-10 * 1024 // N), 5)) for hop in STREAM_CURVE_HOPS for N in pv_cases.STREAM_BLOCKS]
assert len(STREAM_CURVE_CASES) == 24


def stream_curve_id(c):
    return f"hop{c.hop}-N{c.N}"


def stream_curve_input(c):
    return pv_cases.mixed_streams(c.N * c.n_blocks, seed=c.hop + c.N)


def stream_curve_semitones(c):
    """[n_blocks][N_STREAMS] float64."""
    return np.random.default_rng([c.N, c.hop, 4]).uniform(-12.0, 12.0, (c.n_blocks, N_STREAMS))


def by_block(cls, x, N, hop, ratio):
    """One stream through a fresh cls(N, hop), block b with ratio[b]."""
    r = cls(N, hop)
    return np.concatenate([r.process(x[b * N:(b + 1) * N], float(ratio[b])) for b in range(len(ratio))])


def stream_curve_reference(c, form="radians", shift=0):
    """[N_STREAMS][N n_blocks] float64, once per case, form and shift.  shift = +1 / -1: block b takes the ratio of block b + 1 / b - 1,
    clamped to the table."""
    key = (c, form, shift)
    if key not in _REF:
        cls = P.PvStreamRef if form == "radians" else pv_cases.PvStreamTurns
        x, ratio = stream_curve_input(c), pv_cases.ratio_of(stream_curve_semitones(c))
        rows = np.clip(np.arange(c.n_blocks) + shift, 0, c.n_blocks - 1)
        ref = np.stack([by_block(cls, x[s], c.N, c.hop, ratio[rows, s]) for s in range(N_STREAMS)])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


# ---- one scenario per hop: curve calls, plain calls, interval changes and resets ------------------------------------------------------------
# pv_cases.SCENARIOS' geometry and schedule (blocks of 100 samples, calls of 1, 3, 16 and 2 blocks, the same changes and resets, keyed by
# the call they precede).  Call i is a curve call unless i % 5 == 1; all three resets precede curve calls.  The rules:
#   a change sets the HELD interval at its call, whether that is a curve call or a plain one;
#   a reset applies before its call;
#   a curve call runs block by block with its own ratios and leaves the held interval as it was;
#   a plain call uses the held interval.
CURVE_SCENARIOS = list(pv_cases.SCENARIOS)


def scenario_is_plain(i):
    return i % 5 == 1


def scenario_semitones(c):
    """[n_blocks][S] float64: the table the curve calls cut their rows from."""
    return np.random.default_rng([c.hop, 6]).uniform(-12.0, 12.0, (c.n_blocks, len(c.semitones)))


def scenario_reference(c, form="radians", shift=0, all_plain=False):
    """The output [S][T] (once per case and variant), per stream [(call, frames since the last reset mod 4, samples of the call)] of its
    resets, and the held interval [S] after the last call.  shift = 1: the curve calls take block b + 1's row (clamped to the table);
    all_plain: every call a plain one."""
    key = ("scenario", c.hop, form, shift, all_plain)
    if key not in _REF:
        cls = P.PvStreamRef if form == "radians" else pv_cases.PvStreamTurns
        x, ratio = pv_cases.scenario_input(c), pv_cases.ratio_of(scenario_semitones(c))
        spans = pv_cases.call_spans(c.n_blocks, c.calls)
        y, landed, held = np.zeros(x.shape), [], []
        for s in range(x.shape[0]):
            r = cls(c.N, c.hop, ratio=pv_cases.ratio_of(c.semitones[s]))
            semi, b0, out, hits = c.semitones[s], 0, [], []
            for i, k in enumerate(spans):
                for st, v in c.changes.get(i, []):
                    if st == s:
                        semi = v
                if s in c.resets.get(i, []):
                    hits.append((i, r.nf % pv_cases.ROUND, k * c.N))
                    r.reset()
                if all_plain or scenario_is_plain(i):
                    out.append(r.process(x[s, b0 * c.N:(b0 + k) * c.N], pv_cases.ratio_of(semi)))
                else:
                    for b in range(b0, b0 + k):
                        out.append(r.process(x[s, b * c.N:(b + 1) * c.N], float(ratio[min(b + shift, c.n_blocks - 1), s])))
                b0 += k
            y[s] = np.concatenate(out)
            landed.append(hits)
            held.append(semi)
        y.setflags(write=False)
        _REF[key] = (y, landed, held)
    return _REF[key]


# ---- more workgroups than compute units: 300 streams, every stream its own "steps" curve --------------------------------------------------
# Three legs: the 1024-point one-shot kernel (odd T), the 2048-point one (aligned T), the streaming kernel (24 blocks of 256 samples).
# Streams 0, 1, 255, 256 and 299 are compared with NumPy (and gated on the CPU like every pointwise case).
BigLeg = namedtuple("BigLeg", "kind F hop T N")
BIG_S = 300
BIG_CHECKED = (0, 1, 255, 256, 299)
BIG_LEGS = [BigLeg("one-shot", 1024, 256, 1024 + 18 * 256 + 3, 0), BigLeg("one-shot", 2048, 512, 2048 + 18 * 512, 0),
            BigLeg("stream", 1024, 256, 24 * 256, 256)]


def big_id(g):
    return f"{g.kind}-F{g.F}-hop{g.hop}"


def steps(hop, s, n):
    """semitones_of's "steps" curve for any stream number."""
    return np.random.default_rng([hop, s, 9]).uniform(-12.0, 12.0, n)


def big_input(g):
    return pv_cases.harmonic_streams(BIG_S, g.T, seed=g.hop + 3)


def big_semitones(g):
    """[BIG_S][n]: n frames (one-shot) or n blocks (stream; the call's table is its transpose)."""
    n = g.T // g.N if g.kind == "stream" else (g.T - g.F) // g.hop + 1
    return np.stack([steps(g.hop, s, n) for s in range(BIG_S)])


def big_reference(g, form="radians", off=False):
    """{stream: [T] float64} for BIG_CHECKED; off: the curve rolled by one frame / block."""
    key = (g, form, off)
    if key not in _REF:
        x, ratio = big_input(g), pv_cases.ratio_of(big_semitones(g))
        if off:
            ratio = np.roll(ratio, 1, axis=1)
        cls = P.PvStreamRef if form == "radians" else pv_cases.PvStreamTurns
        if g.kind == "stream":
            _REF[key] = {s: by_block(cls, x[s], g.N, g.hop, ratio[s]) for s in BIG_CHECKED}
        else:
            _REF[key] = {s: frame_loop(x[s], g.F, g.hop, ratio[s], form) for s in BIG_CHECKED}
    return _REF[key]
