"""The peak-locked test matrix (vp_stft_pitch_shift_locked, vp_pv_process_blocks_locked_device): signals, curves and cases that
tests/test_pv_lock_reference_cpu.py (gate, identity, teeth, quality) and tests/test_gpu_pv_lock.py (kernels against NumPy) iterate.
tests/pv_lock_edge_cases.py (the edge cases, with tests/test_pv_lock_edges_cpu.py and tests/test_gpu_pv_lock_edges.py) takes the bound,
the gate tolerance, the teeth, the lengths and the streaming call pattern from here, and the CPU file pins what this matrix reaches.
Test infrastructure only.  The definition is tests/pv_lock_reference.py; the bound of every pointwise GPU comparison is pv_cases.bound's,

    |y - ref| <= 4 O 2^-24 max(1, max |ref|)       at every sample,

whose derivation holds unchanged: the locked stage is double like the plain one, only the output frames and their overlap-add are float32.
"""
from collections import namedtuple

import numpy as np

import pv_cases
import pv_lock_reference as LR

F = 1024
FS = 44100.0
GATE_TOL = 1e-9                             # the two forms of the reference, relative to max(1, max |ref|): the plain family's gate
TEETH = 10.0                                # a mutant is at least this many GPU bounds away on a case chosen to see it
bound = pv_cases.bound
ratio_of = pv_cases.ratio_of


# ---- signals (float32, seeded) --------------------------------------------------------------------------------------------------------------
def _t(T):
    return np.arange(T) / FS


def noise(T, seed=0):
    return (0.25 * np.random.default_rng([seed, 31]).standard_normal(T)).astype(np.float32)


def voice(T, seed=0, f0=151.0, harmonics=12):
    """A 12-harmonic voice, 1 / h amplitudes, seeded phases."""
    rng = np.random.default_rng([seed, 32])
    x = np.zeros(T)
    for h in range(1, harmonics + 1):
        x += 0.3 / h * np.sin(2 * np.pi * f0 * h * _t(T) + rng.uniform(0, 2 * np.pi))
    return x.astype(np.float32)


def glide(T, seed=0):
    """Three harmonics gliding up an octave over the signal: peaks cross bins."""
    ph = 2 * np.pi * np.cumsum(220.0 * 2.0 ** (np.arange(T) / max(T - 1, 1))) / FS
    rng = np.random.default_rng([seed, 33])
    return sum(0.3 / h * np.sin(h * ph + rng.uniform(0, 2 * np.pi)) for h in (1, 2, 3)).astype(np.float32)


def tone(T, seed=0, freq=227.3, amp=0.5):
    ph = np.random.default_rng([seed, 34]).uniform(0, 2 * np.pi)
    return (amp * np.sin(2 * np.pi * freq * _t(T) + ph)).astype(np.float32)


def voice_noise(T, seed=0):
    return (voice(T, seed, 196.0, 8).astype(np.float64) + 0.05 * np.random.default_rng([seed, 35]).standard_normal(T)).astype(np.float32)


def tone_tone(T, seed=0):
    """A tone, then (from the middle) another one: a peak disappears and one appears."""
    x = tone(T, seed, 440.0, 0.4).copy()
    x[T // 2:] = tone(T, seed + 1, 1000.7, 0.4)[T // 2:]
    return x


def square_exact(T, seed=0):
    """Period 64 samples: harmonics on exact bins (16, 48, 80, ...)."""
    return np.where((np.arange(T) // 32) & 1, -0.5, 0.5).astype(np.float32)


def silence_noise(T, seed=0):
    """Digital silence (frames without a peak), then noise."""
    x = noise(T, seed + 2).copy()
    x[:T // 2] = 0.0
    return x


def centre_clicks(T, seed=0):
    """Clicks that a hop-512 frame sees exactly at its centre (the frame before and the one after see them at sample 0, where the window
    is 0): X[k] = +-w[512] x, a magnitude spectrum that is flat to the last bit -- one plateau over all bins, whose leftmost bin (0) is
    the frame's only peak.  Frames in between are digital silence."""
    x = np.zeros(T, np.float32)
    x[1024] = 0.5
    x[2048] = -0.25
    return x


SIGNALS = {"noise": noise, "voice": voice, "glide": glide, "tone": tone, "voice+noise": voice_noise, "tone-tone": tone_tone,
           "square": square_exact, "silence-noise": silence_noise}
GPU_STREAMS = ("noise", "voice", "glide", "tone", "voice+noise", "tone-tone")        # the mixed content of a pointwise GPU case


# ---- curves: semitones or ratios per frame ------------------------------------------------------------------------------------------------
def curve(name, nF, hop=256, stream=0):
    """float64 [nF] RATIOS (unclamped: "outside" leaves [0.5, 2] on purpose)."""
    f = np.arange(nF)
    if name == "+7":
        return np.full(nF, ratio_of(7.0))
    if name == "-12":
        return np.full(nF, 0.5)
    if name == "vibrato":
        return ratio_of(3.0 + 2.5 * np.sin(2 * np.pi * (f + stream) / 5.3))
    if name == "steps":
        return ratio_of(np.array([-12.0, -5.0, 0.37, 7.0, 12.0, 0.0, -11.99])[(f // 2 + stream) % 7])
    if name == "octaves":
        return np.where((f + stream) % 2 == 0, 0.5, 2.0)
    if name == "outside":
        return np.array([0.25, 3.0, 1.0, np.inf, 0.0, -1.0, 2.5, 0.5])[(f + stream) % 8]
    raise KeyError(name)


GATE_CURVES = ("+7", "-12", "vibrato", "steps")
GPU_CURVES = ("+7", "-12", "vibrato", "steps", "octaves", "outside")

# ---- the gate matrix: 8 signals x 4 curves x 3 hops --------------------------------------------------------------------------------------
GateCase = namedtuple("GateCase", "signal curve hop nF")
GATE_HOPS = (64, 256, 512)
GATE_NF = 14
GATE_CASES = [GateCase(s, c, hop, GATE_NF) for s in SIGNALS for c in GATE_CURVES for hop in GATE_HOPS]
assert len(GATE_CASES) == 96


def gate_id(c):
    return f"{c.signal}-{c.curve}-hop{c.hop}"


def length(nF, hop, extra=0):
    return F + (nF - 1) * hop + extra


def gate_input(c):
    return SIGNALS[c.signal](length(c.nF, c.hop, 3), seed=c.hop)


_REF = {}


def gate_reference(c, form="a", mutant=None):
    """float64 [T], once per case, form and mutant (callers do not write to it)."""
    key = ("gate", c, form, mutant)
    if key not in _REF:
        x, r = gate_input(c), curve(c.curve, c.nF, c.hop)
        y = LR.locked_roundtrip_b(x, r, F, c.hop) if form == "b" else LR.locked_roundtrip(x, r, F, c.hop, mutant)
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


# degenerate inputs: listed apart, held to properties (finite, bounded); whether they pass the gate is recorded, not asserted
DEGENERATE = ("silence", "dc", "nyquist", "impulses")

# ---- teeth: mutant -> the gated case chosen to see it -------------------------------------------------------------------------------------
TEETH_CASES = {
    "noprop": GateCase("glide", "vibrato", 256, GATE_NF),        # peaks move across bins: the region's angle must travel with them
    "tieup": GateCase("square", "+7", 256, GATE_NF),             # peaks 32 bins apart: the bin in the middle is a tie
    "ratio": GateCase("tone", "+7", 256, GATE_NF),
    "floor": GateCase("voice", "+7", 256, GATE_NF),
    "noown": GateCase("voice", "steps", 256, GATE_NF),           # partials 3.5 bins apart, r from 0.5 to 2: at r > 1 the gaps between regions must stay empty
    "late": GateCase("voice", "steps", 256, GATE_NF),
    "strict": None,                                              # the plateau case below
}
PLATEAU_NF, PLATEAU_HOP = 8, 512


def plateau_input():
    return centre_clicks(length(PLATEAU_NF, PLATEAU_HOP), 0)


# ---- GPU one-shot cases -----------------------------------------------------------------------------------------------------------------------
GPU_HOPS = pv_cases.HOPS
GPU_NF = (1, 2, 5, 6, 7, 8)                 # every residue mod 4 of the last round, with a tail of hop - 1 samples


def gpu_input(hop, nF):
    T = length(nF, hop, hop - 1)
    return np.stack([SIGNALS[s](T, seed=hop + nF) for s in GPU_STREAMS])


def gpu_ratios(name, hop, nF):
    """[S][nF] float64 ratios, every stream its own phase of the curve."""
    return np.stack([curve(name, nF, hop, s) for s in range(len(GPU_STREAMS))])


def gpu_reference(hop, nF, name):
    key = ("gpu", hop, nF, name)
    if key not in _REF:
        x, r = gpu_input(hop, nF), gpu_ratios(name, hop, nF)
        y = np.stack([LR.locked_roundtrip(x[s], r[s], F, hop) for s in range(len(x))])
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


# ---- streaming --------------------------------------------------------------------------------------------------------------------------------
STREAM_BLOCKS = (17, 64, 256, 1000, 1024, 4096)
STREAM_CALLS = (1, 3, 16)


def stream_blocks(N):
    """Blocks of a streaming case: at least six frame lengths, at least 20 blocks."""
    return max(-(-6 * F // N), 20)


def stream_input(hop, N):
    T = N * stream_blocks(N)
    return np.stack([SIGNALS[s](T, seed=hop + N) for s in GPU_STREAMS])


def stream_ratios(hop, N):
    """[n_blocks][S] ratios, some outside the clamp."""
    nb = stream_blocks(N)
    r = ratio_of(np.random.default_rng([hop, N, 36]).uniform(-13.0, 13.0, (nb, len(GPU_STREAMS))))
    return r


def per_frame(table, N, hop, T):
    """[n_blocks][S] -> the one-shot's [S][nFrames]: a frame takes the block in which its last sample arrives."""
    nF = (T - F) // hop + 1
    blk = (np.arange(nF) * hop + F - 1) // N
    return np.ascontiguousarray(np.asarray(table)[blk].T)


# ---- quality: envelope ripple of stationary tones ---------------------------------------------------------------------------------------------
QUALITY_TONES = (227.3, 1000.7)
QUALITY_SEMITONES = (7.0, -5.0, 12.0, -12.0, 0.37)
QUALITY_T = 44100 // 2 + 6 * F
QUALITY_TRIM = 2048


def analytic_magnitude(y):
    Y = np.fft.fft(y)
    n = len(y)
    h = np.zeros(n)
    h[0] = 1.0
    h[1:(n + 1) // 2] = 2.0
    if n % 2 == 0:
        h[n // 2] = 1.0
    return np.abs(np.fft.ifft(Y * h))


def ripple(y):
    """(std / mean, mean) of the analytic-signal magnitude with QUALITY_TRIM samples trimmed at each end."""
    a = analytic_magnitude(np.asarray(y, np.float64))[QUALITY_TRIM:-QUALITY_TRIM]
    return float(a.std() / a.mean()), float(a.mean())


def quality_tone(freq):
    return (0.5 * np.sin(2 * np.pi * freq * np.arange(QUALITY_T) / FS)).astype(np.float32)


def quality_voice():
    return voice(QUALITY_T, 0, 151.0, 12)
