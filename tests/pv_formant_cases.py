"""The formant test matrix (vp_stft_pitch_shift_formant, vp_pv_process_blocks_formant_device): the cases that
tests/test_pv_formant_reference_cpu.py (gate, teeth, clamp share) and tests/test_gpu_pv_formant.py (kernels against NumPy) BOTH iterate.
Test infrastructure only.  The definition is tests/pv_formant_reference.py; signals, curves, lengths and the bound are
tests/pv_curve_cases.py's at 1024-point frames (the formant build's only frame length):

    |y - ref| <= 4 O 2^-24 max(1, max |ref|)       at every sample

-- pv_cases.bound, whose derivation holds unchanged: the envelope stage is double like the rest of the stage, and only the output frames
and their overlap-add are float32.
"""
from collections import namedtuple

import numpy as np

import pv_cases
import pv_curve_cases as CC
import pv_formant_reference as FR

F = 1024
N_STREAMS = CC.N_STREAMS
HOPS = pv_cases.HOPS
N_FRAMES = CC.N_FRAMES
CURVES = ("glide", "steps", "octaves")
LIFTERS = (4, 32, 64)
FORMANT_RATIOS = np.array([1.0, 1.0, 2.0 ** (-5.0 / 12.0), 2.0, 0.5])      # per stream: preserved twice, down a fourth, the two ends of the clamp
GATE_TOL = CC.GATE_TOL
TEETH = CC.TEETH
CLAMP_SHARE_CAP = 0.10

FormantCase = namedtuple("FormantCase", "hop nF extra curve nc")
CASES = [FormantCase(hop, nF, 3 if nF == 19 else 0, c, nc) for hop in HOPS for nF in N_FRAMES for c in CURVES for nc in LIFTERS]
assert len(CASES) == 72
# the edge frame counts of pv_curve_cases.EDGE_FRAMES (last rounds of 1, 2, 1 and 2 frames, the longest tail), the lifters in turn
EDGE_CASES = [FormantCase(e.hop, e.nF, e.extra, e.curve, LIFTERS[i % 3]) for i, e in enumerate(c for c in CC.EDGE_CASES if c.F == F)]
assert len(EDGE_CASES) == 28 and sorted({c.nF for c in EDGE_CASES}) == [1, 2, 5, 6]
ALL_CASES = CASES + EDGE_CASES


def case_id(c):
    return f"hop{c.hop}-nF{c.nF}+{c.extra}-{c.curve}-nc{c.nc}"


def length(c):
    return F + (c.nF - 1) * c.hop + c.extra


def bound(c, ref):
    return pv_cases.bound(c.hop, ref)


# pv_curve_cases' seed (hop + 5) everywhere but here: on that seed's one frame at hop 256 the pure tone of stream 3 under lifter 64 puts
# 11 % of the (frame, bin) pairs at the +-ln 16 clamp in the REFERENCE alone (276 of its 513 bins), above CLAMP_SHARE_CAP; seed hop + 6 has 4 %
SEED_OF = {FormantCase(256, 1, 255, "steps", 64): 256 + 6}


def case_input(c):
    return pv_cases.mixed_streams(length(c), seed=SEED_OF.get(c, c.hop + 5))


def ratios_of(c):
    """[N_STREAMS][nF] pitch ratios: pv_curve_cases' curves."""
    return pv_cases.ratio_of(CC.semitones_of(CC.CurveCase(F, c.hop, c.nF, c.curve)))


_REF = {}
STATS = {}                                  # case -> clamp counts of the plain radians reference


def reference(c, form="radians", variant=None):
    """[N_STREAMS][T] float64, computed once per case, form and variant (callers do not write to it).  Variants, each what a plausible
    wrong kernel would compute: "nc+1" / "nc-1" the lifter one sample off, "nohalf" no half weight at nc, "phi-next" stream s with
    stream s + 1's formant ratio, "roll" the pitch curve rolled by one frame."""
    key = (c, form, variant)
    if key not in _REF:
        x, ratio, phi, nc, half = case_input(c), ratios_of(c), FORMANT_RATIOS, c.nc, True
        if variant == "nc+1":
            nc += 1
        elif variant == "nc-1":
            nc -= 1
        elif variant == "nohalf":
            half = False
        elif variant == "phi-next":
            phi = np.roll(phi, -1)
        elif variant == "roll":
            ratio = np.roll(ratio, 1, axis=1)
        else:
            assert variant is None, variant
        stats = {}
        ref = np.stack([FR.frame_loop(x[s], F, c.hop, ratio[s], phi[s], nc, form, half, stats) for s in range(N_STREAMS)])
        ref.setflags(write=False)
        _REF[key] = ref
        if variant is None and form == "radians":
            STATS[c] = stats
    return _REF[key]


# ---- streaming: (N, hop, blocks), the calls' sizes cycled -----------------------------------------------------------------------------------
StreamFormantCase = namedtuple("StreamFormantCase", "N hop n_blocks nc")
STREAM_CASES = [StreamFormantCase(1024, 256, 8, 32), StreamFormantCase(100, 128, 60, 4), StreamFormantCase(256, 512, 24, 64)]
STREAM_CALLS = (1, 3, 16, 4)


def stream_id(c):
    return f"N{c.N}-hop{c.hop}-nc{c.nc}"


def stream_input(c):
    return pv_cases.mixed_streams(c.N * c.n_blocks, seed=c.hop + c.N)


def stream_semitones(c):
    """[n_blocks][N_STREAMS] float64."""
    return np.random.default_rng([c.N, c.hop, 11]).uniform(-12.0, 12.0, (c.n_blocks, N_STREAMS))


def per_frame(table, N, hop, T):
    """The per-block table [n_blocks][S] expanded to the one-shot's [S][nFrames]: a frame takes the block in which its last sample arrives."""
    nF = (T - F) // hop + 1
    blk = (np.arange(nF) * hop + F - 1) // N
    return np.ascontiguousarray(np.asarray(table)[blk].T)


# ---- more workgroups than compute units -----------------------------------------------------------------------------------------------------
BIG_S = CC.BIG_S
BIG_CHECKED = CC.BIG_CHECKED
BIG_HOP, BIG_NF, BIG_NC = 256, 19, 32
BIG_T = F + (BIG_NF - 1) * BIG_HOP + 3


def big_input():
    return pv_cases.harmonic_streams(BIG_S, BIG_T, seed=BIG_HOP + 3)


def big_ratios():
    return pv_cases.ratio_of(np.stack([CC.steps(BIG_HOP, s, BIG_NF) for s in range(BIG_S)]))


def big_formants():
    return FORMANT_RATIOS[np.arange(BIG_S) % N_STREAMS]


def big_reference(form="radians"):
    key = ("big", form)
    if key not in _REF:
        x, ratio, phi = big_input(), big_ratios(), big_formants()
        stats = {}
        _REF[key] = {s: FR.frame_loop(x[s], F, BIG_HOP, ratio[s], phi[s], BIG_NC, form, stats=stats) for s in BIG_CHECKED}
        if form == "radians":
            STATS["big"] = stats
    return _REF[key]


# =============================================================================================================================================
# The edges (tests/test_pv_formant_edges_cpu.py gates them, tests/test_gpu_pv_formant_edges.py runs the kernels on them): where the additions
# marked "formant:" can be wrong and the matrix above, by its own design, does not look.  Six frames (+3 samples) unless stated otherwise.
# =============================================================================================================================================
EDGE_NF, EDGE_EXTRA = 6, 3
EDGE_HOPS = (64, 512)                       # the longest and the shortest overlap-add
_STATS = {}                                 # key of an edge reference -> per stream clamp counts of its plain radians form


def _band_noise(T, seed, tag, edge_bin, db, below, amp):
    """White noise with the part of its spectrum at or above (below: under) frame bin edge_bin's frequency, k >= edge_bin T / F, taken
    down by db; float32 [T]."""
    X = np.fft.rfft(np.random.default_rng([seed, tag]).standard_normal(T))
    k = np.arange(len(X))
    X[(k < edge_bin * T / F) if below else (k >= edge_bin * T / F)] *= 10.0 ** (db / 20.0)
    return (amp * np.fft.irfft(X, T)).astype(np.float32)


def step_noise(T, seed):
    """Noise with a 60 dB step down at frame bin 128.  With phi = 2 the weak upper band takes the strong band's envelope (the + clamp, on
    content that after x 16 is still far above the bound); with phi < 1 the strong band's upper part takes the weak band's (the - clamp)."""
    return _band_noise(T, seed, 21, 128, -60.0, False, 0.25)


def bright_noise(T, seed):
    """Noise whose energy sits in frame bins 496 .. 512 (everything below at -40 dB): the envelope is steep at its last bin, where a
    cosine series is otherwise flat."""
    return _band_noise(T, seed, 22, 496, -40.0, True, 1.0)


def _edge_streams(signal, T, hop):
    return np.stack([signal(T, hop + 1000 * s) for s in range(N_STREAMS)])


def _edge_reference(key, x, ratio, phi, nc, hop, form, wrong):
    """[S][T] float64 of one-shot streams x with tables ratio [S][nF] and phi [S], once per key."""
    key = key + (form, wrong)
    if key not in _REF:
        per_stream = [{} for _ in range(len(x))]
        ref = np.stack([FR.frame_loop(x[s], F, hop, ratio[s], phi[s], nc, form, stats=per_stream[s], wrong=wrong) for s in range(len(x))])
        ref.setflags(write=False)
        _REF[key] = ref
        if form == "radians" and wrong is None:
            _STATS[key[:-2]] = per_stream
    return _REF[key]


# ---- 1. the clamp, both signs, on bins that carry energy --------------------------------------------------------------------------------------
# CLAMP_SHARE_CAP does not apply: these cases are there FOR the clamp.  Streams 0 and 3 (phi = 2) reach the + clamp, streams 1 and 4 (1/2)
# and stream 2 (down a fourth) the - clamp.
CLAMP_PHIS = np.array([2.0, 0.5, 2.0 ** (-5.0 / 12.0), 2.0, 0.5])
CLAMP_HIGH, CLAMP_LOW = (0, 3), (1, 4)                                              # the streams with phi = 2 and phi = 1/2
CLAMP_CASES = [FormantCase(hop, EDGE_NF, EDGE_EXTRA, c, nc) for hop in EDGE_HOPS for c in ("glide", "steps") for nc in (32, 64)]
CLAMP_MIN_SHARE = 0.05


def clamp_input(c):
    return _edge_streams(step_noise, length(c), c.hop)


def clamp_reference(c, form="radians", wrong=None):
    return _edge_reference(("clamp", c), clamp_input(c), ratios_of(c), CLAMP_PHIS, c.nc, c.hop, form, wrong)


def clamp_stats(c):
    clamp_reference(c)
    return _STATS[("clamp", c)]


# ---- 2. the top of the interpolation ------------------------------------------------------------------------------------------------------------
# phi = 1/2 on every stream: every kk >= 256 reads the envelope at the clip, src = 512, i0 = 511, t = 1, le[512].  One pitch ratio for all
# frames and streams.  The clamp share is near one half (the envelope steps by 40 dB): no cap here either.
# The clip on the PITCH-ratio side cannot be observed: for r < 1 no content lands above bin 512 r, so at(r) is read at the clip only for
# bins whose magnitude is zero ("top511" with r = 1/2 and phi = 1 moves the reference by 0 bounds), and for r >= 1 the source kk / r never
# reaches the clip.  No test is written for it.
TopCase = namedtuple("TopCase", "hop nF extra semitones nc")
TOP_CASES = [TopCase(hop, EDGE_NF, EDGE_EXTRA, st, nc) for hop in EDGE_HOPS for st in (0.0, -7.0) for nc in (32, 64)]
TOP_PHIS = np.full(N_STREAMS, 0.5)


def top_id(c):
    return f"hop{c.hop}-{c.semitones:+g}st-nc{c.nc}"


def top_input(c):
    return _edge_streams(bright_noise, length(c), c.hop)


def top_ratios(c):
    return np.full((N_STREAMS, c.nF), pv_cases.ratio_of(c.semitones))


def top_reference(c, form="radians", wrong=None):
    return _edge_reference(("top", c), top_input(c), top_ratios(c), TOP_PHIS, c.nc, c.hop, form, wrong)


def top_stats(c):
    top_reference(c)
    return _STATS[("top", c)]


# ---- 3. levels: the floor m^2 + 1e-12 -----------------------------------------------------------------------------------------------------------
# The envelope stage is the one stage of the family that is NOT homogeneous: below about 2^-16 the floor flattens the envelope of the quiet
# bins.  mixed_streams x 2^e (exact in float32), lifter 32, the "steps" curve, FORMANT_RATIOS.
LevelCase = namedtuple("LevelCase", "hop nF extra e")
LEVELS = (-16, -20, -24, 15)
LEVEL_CASES = [LevelCase(hop, EDGE_NF, EDGE_EXTRA, e) for hop in HOPS for e in LEVELS]
LEVEL_NC = 32
LEVEL_GATE_TOL = 1e-9                       # the two forms, relative to max |ref| (no max(1, .))
NON_HOMOGENEITY = 0.01                      # at e = -20 the reference is further than this from 2^-20 x the full-level one, of its peak


def level_id(c):
    return f"hop{c.hop}-2^{c.e}"


def level_bound(hop, ref):
    """4 O 2^-24 max |ref|: pv_cases.bound without its max(1, .).  That derivation counts roundings RELATIVE to the partial sums of the
    overlap-add, so it is scale-free; the max(1, .) only keeps a bound for signals that cancel to nothing.  At 2^-24 the float32 terms are
    around 6e-8 (the quietest part, the noise floor at -40 dB, 6e-10), far above the denormal range (1.2e-38), so every rounding is
    still relative."""
    return 4.0 * (F // hop) * 2.0 ** -24 * float(np.abs(ref).max())


def _level_case(c):
    return FormantCase(c.hop, c.nF, c.extra, "steps", LEVEL_NC)


def level_input(c):
    x = case_input(_level_case(c))
    y = x * np.float32(2.0 ** c.e)
    assert np.array_equal(y.astype(np.float64), x.astype(np.float64) * 2.0 ** c.e)  # exact: no sample leaves the normal range
    return y


def level_reference(c, form="radians", wrong=None):
    return _edge_reference(("level", c), level_input(c), ratios_of(_level_case(c)), FORMANT_RATIOS, LEVEL_NC, c.hop, form, wrong)


# a level step INSIDE frames: the first F + 300 and the last 700 samples 2^-22 times the rest (frames 0 and 1 and the last one wholly quiet,
# frames 2 and 7, 8 across the steps).  Exact digital silence in front of an onset does NOT pass the gate (the wrap ties of the all-zero
# frame: the two forms differ by 0.01 .. 0.18 of the peak) and gets property checks only (silence_onset_input).
STEP_CASE = FormantCase(256, 10, 3, "steps", 32)
STEP_HEAD, STEP_TAIL, STEP_LEVEL = F + 300, 700, 2.0 ** -22
STEP_QUIET = 2 * 256                        # output samples [0, 512) are covered by frames 0 and 1 alone


def step_input():
    x = pv_cases.mixed_streams(length(STEP_CASE), seed=77).copy()
    x[:, :STEP_HEAD] *= np.float32(STEP_LEVEL)
    x[:, -STEP_TAIL:] *= np.float32(STEP_LEVEL)
    return x


def step_reference(form="radians", wrong=None):
    return _edge_reference(("step",), step_input(), ratios_of(STEP_CASE), FORMANT_RATIOS, STEP_CASE.nc, STEP_CASE.hop, form, wrong)


def silence_onset_input():
    x = pv_cases.mixed_streams(length(STEP_CASE), seed=77).copy()
    x[:, :STEP_HEAD] = 0.0
    x[:, -STEP_TAIL:] = 0.0
    return x


# ---- 4. every lifter ----------------------------------------------------------------------------------------------------------------------------
ALL_LIFTERS = tuple(range(4, 65))
LIFTER_CASE = FormantCase(256, EDGE_NF, EDGE_EXTRA, "steps", 0)                      # (nc: the call's)


def lifter_reference(nc, form="radians"):
    c = LIFTER_CASE
    return _edge_reference(("lifter", nc), case_input(c), ratios_of(c), FORMANT_RATIOS, nc, c.hop, form, None)


def lifter_stats(nc):
    lifter_reference(nc)
    return _STATS[("lifter", nc)]


# ---- 5. the streaming kernel --------------------------------------------------------------------------------------------------------------------
# (a) bit identity with the one-shot on pv_curve_cases.STREAM_CURVE_CASES: nothing to gate, GPU only.
STREAM_BIT_LIFTERS = (4, 32, 64)
# (b) against NumPy driven block by block: hop 64 (never launched), N = 17 (calls without a frame) and N = 4096 (many rounds in a call)
STREAM_EDGE_CASES = [StreamFormantCase(N, hop, max(-(-6 * F // N), 3), LIFTERS[i % 3])
                     for i, (hop, N) in enumerate(((64, 17), (64, 4096), (512, 17), (512, 4096), (256, 1000), (128, 64)))]


def stream_edge_reference(c, form="radians", shift=0):
    """[N_STREAMS][N n_blocks] float64; shift = 1: block b takes block b + 1's ratios (clamped to the table)."""
    key = ("stream-edge", c, form, shift)
    if key not in _REF:
        x, ratio = stream_input(c), pv_cases.ratio_of(stream_semitones(c))
        rows = np.clip(np.arange(c.n_blocks) + shift, 0, c.n_blocks - 1)
        ref = np.stack([FR.by_block(x[s], c.N, c.hop, ratio[rows, s], FORMANT_RATIOS[s], c.nc, form) for s in range(N_STREAMS)])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


# (c) one scenario per hop: pv_cases.SCENARIOS' geometry and schedule (blocks of 100 samples in calls of 1, 3, 16 and 2, four streams, the
# interval changes and the resets keyed by the call they precede; the resets at calls 4 and 8 land in the middle of a round at every hop).
# The calls cycle through curve (i % 3 == 0), plain (1) and formant (2): the reset at call 8 and the changes at calls 2, 5, 14 and 17 are
# pending at FORMANT calls, the resets at calls 4 and 13 at plain ones, the change at call 9 at a curve call.  pv_curve_cases' rules hold,
# with: a formant call is a curve call with the streams' formant ratios and the lifter; curve and plain calls are phi = "pitch".
FORMANT_SCENARIOS = list(pv_cases.SCENARIOS)
SCENARIO_KINDS = ("curve", "plain", "formant")
SCENARIO_PHIS = FORMANT_RATIOS[1:]          # four streams: preserved, down a fourth, the two ends of the clamp
SCENARIO_NC = 32


def scenario_kind(i):
    return SCENARIO_KINDS[i % 3]


def scenario_semitones(c):
    """[n_blocks][S] float64: the table the formant and curve calls cut their rows from."""
    return np.random.default_rng([c.hop, 14]).uniform(-12.0, 12.0, (c.n_blocks, len(c.semitones)))


def scenario_reference(c, form="radians", shift=0):
    """The output [S][T] (once per case and variant), per stream [(call, frames since the last reset mod 4, samples of the call)] of its
    resets, and the held interval [S] after the last call.  shift = +1 / -1: every change and reset one call late / early."""
    key = ("formant-scenario", c.hop, form, shift)
    if key not in _REF:
        cls = FR.FormantRef if form == "radians" else FR.FormantTurns
        x, ratio = pv_cases.scenario_input(c), pv_cases.ratio_of(scenario_semitones(c))
        spans = pv_cases.call_spans(c.n_blocks, c.calls)
        y, landed, held = np.zeros(x.shape), [], []
        for s in range(x.shape[0]):
            r = cls(c.N, c.hop, ratio=pv_cases.ratio_of(c.semitones[s]), phi="pitch", nc=SCENARIO_NC)
            semi, b0, out, hits = c.semitones[s], 0, [], []
            for i, k in enumerate(spans):
                j = i - shift                                    # the call whose changes and resets apply before call i
                for st, v in c.changes.get(j, []):
                    if st == s:
                        semi = v
                if s in c.resets.get(j, []):
                    hits.append((i, r.nf % pv_cases.ROUND, k * c.N))
                    r.reset()
                kind = scenario_kind(i)
                r.set_formant(SCENARIO_PHIS[s] if kind == "formant" else "pitch")
                if kind == "plain":
                    out.append(r.process(x[s, b0 * c.N:(b0 + k) * c.N], pv_cases.ratio_of(semi)))
                else:
                    for b in range(b0, b0 + k):
                        out.append(r.process(x[s, b * c.N:(b + 1) * c.N], float(ratio[b, s])))
                b0 += k
            y[s] = np.concatenate(out)
            landed.append(hits)
            held.append(semi)
        y.setflags(write=False)
        _REF[key] = (y, landed, held)
    return _REF[key]


# (d) 300 streams through the streaming kernel: 24 blocks of 256 samples at hop 256, every stream its own "steps" table
BIG_STREAM = StreamFormantCase(256, 256, 24, 32)


def big_stream_input():
    return pv_cases.harmonic_streams(BIG_S, BIG_STREAM.N * BIG_STREAM.n_blocks, seed=BIG_STREAM.hop + 4)


def big_stream_ratios():
    """[n_blocks][BIG_S]."""
    return pv_cases.ratio_of(np.stack([CC.steps(BIG_STREAM.hop, s, BIG_STREAM.n_blocks) for s in range(BIG_S)]).T)


def big_stream_reference(form="radians"):
    key = ("big-stream", form)
    if key not in _REF:
        c, x, ratio, phi = BIG_STREAM, big_stream_input(), big_stream_ratios(), big_formants()
        _REF[key] = {s: FR.by_block(x[s], c.N, c.hop, ratio[:, s], phi[s], c.nc, form) for s in BIG_CHECKED}
    return _REF[key]


# ---- 6. degenerate inputs: pv_cases.DEGENERATE, blocks of 100 samples ---------------------------------------------------------------------------
DEG_N, DEG_BLOCKS = 100, 42


def deg_semitones(hop):
    """[DEG_BLOCKS][N_STREAMS]."""
    return np.stack([CC.steps(hop, s, DEG_BLOCKS) for s in range(N_STREAMS)]).T
