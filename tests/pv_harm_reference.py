"""Build-authored NumPy definition of the phase-vocoder HARMONIZER (vp_stft_harmonize, vp_hz_process_blocks_device;
csrc/vp_stft_harm.inc).  No reference counterpart -- PARITY UNPINNED by nature.  Test infrastructure only.

The inverse transform and the overlap-add are linear, every voice has its own angle state, and the locked stage's analysis (previous
phases, peaks, owners) does not depend on the ratio.  So, in float64 and before any cast,

    harmonize(x, ratio[V][nF], gain[V], dry) = dry stft_roundtrip(x) + sum_v gain[v] locked_roundtrip(x, ratio[v])

with stft_reference.stft_roundtrip and pv_lock_reference.locked_roundtrip: the definition is the composition the kernel replaces.  A gain
or dry value that is NaN or infinite counts as 0; a finite one is clamped to [-4, 4] (clean_gain).  The streaming form replaces the
per-voice term with pv_lock_reference.by_block and delays the dry term by the stream's latency F - gcd(N, hop).

`mutant` names a deliberately wrong variant (the tests' teeth):
  shared_theta      all voices turn ONE angle array (a per-frame voice loop over lock_stage with one LockState)
  swapped           the ratio table of a batch read as [V][S] instead of [S][V] (harmonize_batch only)
  nodry             the dry term missing
  gain_first_voice  every voice takes voice 0's gain
"""
import math

import numpy as np

import pv_lock_reference as LR
from stft_reference import stft_roundtrip, window

MUTANTS = ("shared_theta", "swapped", "nodry", "gain_first_voice")
MAX_VOICES = 4


def clean_gain(g):
    """The gains as the kernels take them: NaN and infinities are 0, the rest is clamped to [-4, 4]."""
    g = np.asarray(g, np.float64)
    return np.where(np.isfinite(g), np.clip(np.where(np.isfinite(g), g, 0.0), -4.0, 4.0), 0.0)


def _shared_theta_voices(x, ratio, F, hop):
    """The mutant's voices: one LockState for all of them; every voice sees the frame's true previous phases, but theta is turned V
    times per frame."""
    x = np.asarray(x, np.float64)
    T = len(x)
    w = window(F)
    scale = 1.0 / np.sum(w[::hop] ** 2)
    nF = (T - F) // hop + 1
    O = F // hop
    r = np.stack([LR.frame_ratios(rv, nF) for rv in ratio])
    st = LR.LockState(F // 2 + 1)
    y = np.zeros((len(r), T))
    for f in range(nF):
        X = np.fft.rfft(x[f * hop:f * hop + F] * w)
        pprev = st.pprev
        for v in range(len(r)):
            st.pprev = pprev
            y[v, f * hop:f * hop + F] += np.fft.irfft(LR.lock_stage(X, r[v, f], st, O), F) * w
    return y * scale


def harmonize(x, ratio, gain=None, dry=0.0, F=1024, hop=256, mutant=None):
    """x: float [T]; ratio: [V][nFrames] (or [V] scalars); gain: [V] or None (1 each); dry: a scalar -> float64 [T]."""
    assert mutant in (None,) + MUTANTS and mutant != "swapped", mutant
    x = np.asarray(x, np.float64)
    V = len(ratio)
    assert 1 <= V <= MAX_VOICES, V
    g = clean_gain(np.ones(V) if gain is None else gain)
    assert g.shape == (V,), g.shape
    if mutant == "gain_first_voice":
        g = np.full(V, g[0])
    d = float(clean_gain(dry))
    y = np.zeros(len(x)) if (mutant == "nodry" or d == 0.0) else d * stft_roundtrip(x, F, hop)
    if mutant == "shared_theta":
        voices = _shared_theta_voices(x, ratio, F, hop)
    else:
        voices = [LR.locked_roundtrip(x, ratio[v], F, hop) for v in range(V)]
    for v in range(V):
        y = y + g[v] * voices[v]
    return y


def harmonize_batch(x, ratio, gain=None, dry=None, F=1024, hop=256, mutant=None):
    """x [S][T]; ratio [S][V][nFrames]; gain [S][V] or None; dry [S] or None (0) -> float64 [S][T]."""
    x = np.asarray(x)
    ratio = np.asarray(ratio, np.float64)
    S, V = ratio.shape[:2]
    if mutant == "swapped":
        ratio = ratio.reshape(V, S, -1).transpose(1, 0, 2)       # entry [s][v] is read where a [V][S] table keeps it
        mutant = None
    return np.stack([harmonize(x[s], ratio[s], None if gain is None else np.asarray(gain)[s], 0.0 if dry is None else np.asarray(dry)[s],
                               F, hop, mutant) for s in range(S)])


def from_parts(rt, refs, gain, dry):
    """The definition from its parts, for callers that hold them already: rt = stft_roundtrip(x) [T] (or None with dry 0), refs = the
    voices' locked_roundtrip [V][T]."""
    g = clean_gain(np.ones(len(refs)) if gain is None else gain)
    d = float(clean_gain(0.0 if dry is None else dry))
    y = np.zeros(np.shape(refs[0])) if d == 0.0 else d * np.asarray(rt, np.float64)
    for v in range(len(refs)):
        y = y + g[v] * np.asarray(refs[v], np.float64)
    return y


def by_block(x, N, hop, block_ratio, gain=None, dry=0.0, F=1024):
    """The streaming form: x [T] (T a multiple of N) block by block, block b with block_ratio[b][v] -> the stream's output [T] (float64):
    every voice is pv_lock_reference.by_block's, the dry term the round trip delayed by the latency."""
    x = np.asarray(x, np.float64)
    block_ratio = np.asarray(block_ratio, np.float64)
    V = block_ratio.shape[1]
    L = F - math.gcd(N, hop)
    g = clean_gain(np.ones(V) if gain is None else gain)
    d = float(clean_gain(dry))
    y = np.zeros(len(x))
    if d != 0.0 and len(x) >= F:
        rt = stft_roundtrip(x, F, hop)
        y[L:] = d * rt[:len(x) - L]
    for v in range(V):
        y = y + g[v] * LR.by_block(x, N, hop, block_ratio[:, v])
    return y


def gpu_bound(hop, dry, rt, gain, refs, F=1024):
    """pv_lock_reference.gpu_bound's derivation (a double stage, float32 frames, a float32 overlap-add of O terms) with the output peak
    replaced by the sum the frame values are bounded by: 4 O 2^-24 max(1, |dry| max|rt| + sum_v |g_v| max|ref_v|)."""
    g = clean_gain(np.ones(len(refs)) if gain is None else gain)
    d = abs(float(clean_gain(0.0 if dry is None else dry)))
    peak = (d * float(np.max(np.abs(rt))) if d else 0.0) + sum(abs(g[v]) * float(np.max(np.abs(refs[v]))) for v in range(len(refs)))
    return 4.0 * (F // hop) * 2.0 ** -24 * max(1.0, peak)
