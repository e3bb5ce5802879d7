"""The test matrix of the peak-locked pitch shift with sub-bin region offsets (vp_stft_pitch_shift_locked_subbin,
vp_pv_process_blocks_locked_subbin_device): what tests/test_pv_lockf_reference_cpu.py (gate, identity, teeth, conditioning, quality) and
tests/test_gpu_pv_lockf.py (kernels against NumPy) iterate.  Signals, curves, hops, lengths, the bound, the gate tolerance and the teeth
are tests/pv_lock_cases.py's; the references are tests/pv_lockf_reference.py's.  Test infrastructure only.

Conditioning.  The parabola of step 5b is ill-conditioned on a near-flat peak (its denominator is then of rounding size), and the kernel's
magnitudes differ from NumPy's in the last place.  Every (hop, nF, curve, stream) item the GPU compares against NumPy is therefore probed
on the CPU with the lock family's probe -- the spectrum of every frame moved by CONDITION_EPS of its largest magnitude, three seeds -- and
admitted only if the output moves by less than CONDITION_SHARE of the GPU bound.  DROPPED lists the items that miss; the CPU test asserts
that it is exactly those, and that it is at most one in eight of the candidates."""
from collections import namedtuple

import numpy as np

import pv_lock_cases as LC
import pv_lockf_reference as FR

F = LC.F
GATE_TOL, TEETH, bound = LC.GATE_TOL, LC.TEETH, LC.bound
GateCase = LC.GateCase
CONDITION_EPS, CONDITION_SEEDS, CONDITION_SHARE = 1e-13, (0, 1, 2), 0.01      # the lock family's probe
MAX_DROPPED_SHARE = 1.0 / 8.0

_REF = {}


def gate_reference(c, form="a", mutant=None):
    """float64 [T] of gate case c (pv_lock_cases.GATE_CASES), once per case, form and mutant (callers do not write to it)."""
    key = ("gate", c, form, mutant)
    if key not in _REF:
        x, r = LC.gate_input(c), LC.curve(c.curve, c.nF, c.hop)
        y = FR.lockf_roundtrip_b(x, r, F, c.hop) if form == "b" else FR.lockf_roundtrip(x, r, F, c.hop, mutant)
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


# ---- teeth: mutant of the new steps -> the gated case chosen to see it ---------------------------------------------------------------------
TEETH_CASES = {
    "nosign": GateCase("tone", "+7", 256, LC.GATE_NF),           # one lobe, an offset that is no integer: taps of alternating sign cancel
    "nopar": GateCase("voice", "+7", 256, LC.GATE_NF),           # partials off their bins' centres
    "notaper": GateCase("tone", "vibrato", 256, LC.GATE_NF),     # f sweeps (0, 1): the truncated sinc's edge taps
    "leak": GateCase("voice", "steps", 256, LC.GATE_NF),         # partials 3.5 bins apart: taps reach into the neighbour's region
    "round": GateCase("tone", "vibrato", 256, LC.GATE_NF),
    "four": GateCase("square", "+7", 256, LC.GATE_NF),           # wide regions (32 bins): the outer taps -2 and 3 are owned and count
    "mirror": GateCase("tone", "steps", 256, LC.GATE_NF),        # at r < 1 the lowest region's taps reach below bin 0
}
assert set(TEETH_CASES) == set(FR.MUTANTS)

# ---- GPU one-shot items ---------------------------------------------------------------------------------------------------------------------
Item = namedtuple("Item", "hop nF curve stream")
CANDIDATES = [Item(hop, nF, name, s) for hop in LC.GPU_HOPS for nF in LC.GPU_NF for name in LC.GPU_CURVES for s in range(len(LC.GPU_STREAMS))]
DROPPED = frozenset()                      # items that miss the probe (none: the worst moves by 0.008 of the bound)


def admitted(hop, nF, name):
    """The streams of one-shot case (hop, nF, curve) that are compared against NumPy."""
    return [s for s in range(len(LC.GPU_STREAMS)) if Item(hop, nF, name, s) not in DROPPED]


def gpu_reference(hop, nF, name):
    key = ("gpu", hop, nF, name)
    if key not in _REF:
        x, r = LC.gpu_input(hop, nF), LC.gpu_ratios(name, hop, nF)
        y = np.stack([FR.lockf_roundtrip(x[s], r[s], F, hop) for s in range(len(x))])
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


def probe(x, r, hop, y):
    """How far the probe moves the definition's output y of (x, r), in GPU bounds."""
    moved = max(np.abs(FR.lockf_roundtrip(x, r, F, hop, perturb=(CONDITION_EPS, s)) - y).max() for s in CONDITION_SEEDS)
    return moved / bound(hop, y)


# ---- streaming: the issue's block sizes and groupings ----------------------------------------------------------------------------------------
STREAM_BLOCKS = (17, 64, 256, 1000, 1024)
STREAM_CALLS = (1, 3, 16)

# ---- what it is for: the 227.3 Hz tone at -12 and +7 ----------------------------------------------------------------------------------------------
PURPOSE_TONE = 227.3
PURPOSE_SEMITONES = (-12.0, 7.0)
LEVEL_TOL = 0.005


def purpose_levels(st):
    """(integer definition's level, sub-bin definition's level) of the purpose tone at st semitones, once."""
    key = ("purpose", st)
    if key not in _REF:
        import pv_lock_reference as LR
        x, r = LC.quality_tone(PURPOSE_TONE), LC.ratio_of(st)
        _REF[key] = (LC.ripple(LR.locked_roundtrip(x, r, F, 256))[1], LC.ripple(FR.lockf_roundtrip(x, r, F, 256))[1])
    return _REF[key]


# ---- degenerate frames: every peak leaves past N ----------------------------------------------------------------------------------------------
def shifted_out(hop, nF):
    """One damped burst around bin 403 (pv_lock_edge_cases.burst_signal: a single wide lobe, one peak): at r = 2 the peak of every frame
    that sees it shifts past N and nothing is synthesised; the other frames are digital silence."""
    import pv_lock_edge_cases as E
    return E.burst_signal(LC.length(nF, hop, 3), [(F, 403.0, 0.5)], hop)
