"""The cross-synthesis test matrix (vp_stft_cross_synth, vp_xs_process_blocks_device): the cases that
tests/test_pv_cross_reference_cpu.py (identities, teeth, clamp share) and tests/test_gpu_pv_cross.py (kernels against NumPy) BOTH iterate.
Test infrastructure only.  The definition is tests/pv_cross_reference.py.

Three streams, one signal family each (44.1 kHz):
  0 "saw"   a 151 Hz voice of 12 harmonics under three formant resonances, over a 110 Hz sawtooth;
  1 "late"  the same voice over a sawtooth that starts half way through the row, on a noise floor of 1e-5: in front of the start the gain
            runs into the +48 dB clamp on a carrier that is NOT exactly zero (an exactly silent bin hides the clamp: 0 gain = 0);
  2 "band"  the voice with 0.02 of white noise over noise band-limited to 1.5 kHz on a floor of 1e-6: above the band nearly every bin is at
            the clamp.
The depth table is [1, 0.5, 0] -- full, half (what tells "depth-after-clamp" apart), and the identity -- or NULL (1 everywhere).

The gate is the plain round trip's (tests/test_gpu_round4.py): |y - ref| <= 3e-7 max(1, max |ref|) per stream.  The stage adds no decision
and no accumulation, min and exp are continuous: the float32 rounding of the output frames and of their overlap-add still dominates.
"""
from collections import namedtuple

import numpy as np

import pv_cross_reference as XR

F = 1024
FS = 44100.0
N_STREAMS = 3
HOPS = (64, 128, 256, 512)
LIFTERS = (4, 32, 64)
DEPTHS = np.array([1.0, 0.5, 0.0])
GATE = 3e-7
TEETH = 10.0                                 # every WRONG variant is this many gates away on some case
LENGTHS = ("one", "tail", "uncovered", "odd")

CrossCase = namedtuple("CrossCase", "hop length nc table")
CASES = [CrossCase(hop, ln, nc, tab) for hop in HOPS for ln in LENGTHS for nc in LIFTERS for tab in (True, False)]
assert len(CASES) == 96


def case_id(c):
    return f"hop{c.hop}-{c.length}-nc{c.nc}-{'table' if c.table else 'null'}"


def length(c):
    """one frame; a tail round with dead wavefronts; tail samples no frame covers; an odd row length (the unaligned load path)."""
    return {"one": F, "tail": F + 5 * c.hop, "uncovered": F + 11 * c.hop + 37, "odd": F + 3 * c.hop + 1}[c.length]


def gate(ref):
    """per stream: ref [T] -> the bound on |y - ref|."""
    return GATE * max(1.0, float(np.abs(ref).max()))


# ---- signals ---------------------------------------------------------------------------------------------------------------------------------
def voice(T, noise=0.0, seed=0, f0=151.0):
    """12 harmonics of f0 under three resonances (700, 1200, 2600 Hz), peak about 0.5."""
    t = np.arange(T) / FS
    x = np.zeros(T)
    for h in range(1, 13):
        f = h * f0
        a = sum(g / (1.0 + ((f - fc) / bw) ** 2) for fc, bw, g in ((700.0, 130.0, 1.0), (1200.0, 160.0, 0.6), (2600.0, 250.0, 0.35)))
        x += a * np.sin(2.0 * np.pi * f * t + 0.7 * h)
    x *= 0.5 / np.abs(x).max()
    if noise:
        x = x + noise * np.random.default_rng([seed, 1]).standard_normal(T)
    return x


def saw(T, f=110.0, amp=0.5):
    ph = np.arange(T) * (f / FS)
    return amp * (2.0 * (ph - np.floor(ph)) - 1.0)


def late_saw(T, seed=0):
    """A sawtooth from sample T / 2 on, over a noise floor of 1e-5."""
    c = 1e-5 * np.random.default_rng([seed, 2]).standard_normal(T)
    c[T // 2:] += saw(T - T // 2)
    return c


def band_noise(T, seed=0, cutoff=1500.0):
    """White noise band-limited to `cutoff` (a brick wall on the row's spectrum), rms 0.1, on a white floor of 1e-6."""
    rng = np.random.default_rng([seed, 3])
    X = np.fft.rfft(rng.standard_normal(T))
    X[np.fft.rfftfreq(T, 1.0 / FS) > cutoff] = 0.0
    c = np.fft.irfft(X, T)
    c *= 0.1 / np.sqrt(np.mean(c * c))
    return c + 1e-6 * rng.standard_normal(T)


def signals(T, seed=0):
    """(voice, carrier) float32 [N_STREAMS][T] each: the three families."""
    v = np.stack([voice(T), voice(T, f0=163.0), voice(T, noise=0.02, seed=seed)])
    c = np.stack([saw(T), late_saw(T, seed), band_noise(T, seed)])
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(c, np.float32)


def case_input(c):
    return signals(length(c), seed=c.hop + c.nc)


def depths(c):
    """[N_STREAMS] float64, or None for the library's NULL table."""
    return DEPTHS if c.table else None


_REF = {}
STATS = {}                                   # case -> clamp counts of the definition


def reference(c, wrong=None):
    """[N_STREAMS][T] float64, computed once per case and variant (callers do not write to it)."""
    key = (c, wrong)
    if key not in _REF:
        v, x = case_input(c)
        d = depths(c)
        stats = {}
        ref = np.stack([XR.cross_synth(v[s], x[s], F, c.hop, None if d is None else d[s], c.nc, wrong, stats) for s in range(N_STREAMS)])
        ref.setflags(write=False)
        _REF[key] = ref
        if wrong is None:
            STATS[c] = stats
    return _REF[key]


# ---- streaming: (N, hop), the blocks grouped 1, 3 and 16 per call ---------------------------------------------------------------------------
StreamCase = namedtuple("StreamCase", "N hop n_blocks nc")
STREAM_CASES = [StreamCase(64, 256, 64, 32), StreamCase(100, 256, 48, 4), StreamCase(256, 256, 20, 64), StreamCase(1024, 256, 20, 32),
                StreamCase(1536, 256, 20, 32), StreamCase(256, 64, 20, 32), StreamCase(256, 512, 20, 32)]
STREAM_GROUPS = (1, 3, 16)


def stream_id(c):
    return f"N{c.N}-hop{c.hop}"


def stream_input(c):
    return signals(c.N * c.n_blocks, seed=c.N + c.hop)


# ---- more workgroups than compute units -----------------------------------------------------------------------------------------------------
BIG_S = 300
BIG_N, BIG_HOP, BIG_BLOCKS = 1024, 256, 3


def big_input():
    """(voice, carrier) float32 [BIG_S][BIG_N BIG_BLOCKS]: the three families in turn, each stream with a gain of its own."""
    v, c = signals(BIG_N * BIG_BLOCKS, seed=7)
    g = (0.5 + 0.5 * (np.arange(BIG_S) % 7) / 6.0).astype(np.float32)[:, None]
    idx = np.arange(BIG_S) % N_STREAMS
    return np.ascontiguousarray(v[idx] * g), np.ascontiguousarray(c[idx] * g[::-1])
