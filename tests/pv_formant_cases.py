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
