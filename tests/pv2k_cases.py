"""The phase-vocoder test matrix for 2048-point frames (vp_stft_pitch_shift on a handle with frame_len = 2048; kernel vp_k_stft_pv2k of
csrc/vp_stft.hip): the list of cases that tests/test_pv2k_reference_cpu.py (conditioning gate) and tests/test_gpu_pv2k.py (kernel against
NumPy) BOTH iterate.  Test infrastructure only.

The signals, the second statement of the reference (roundtrip_turns, written for any F) and the intervals come from tests/pv_cases.py;
what that file computes from its module-level F = 1024 (bound, magnitude_ceiling, n_frames, the lengths) has a local version for
F = 2048 here.  The bound of every pointwise comparison is pv_cases.py's derivation, in which nothing depends on F: double transforms and
stage (1e-13 from NumPy's), float32 output frames and a float32 overlap-add of O = F / hop terms,
    |y - ref| <= 4 O 2^-24 max(1, max |ref|)       at every sample.
"""
from collections import namedtuple

import numpy as np

from pv_cases import (DEGENERATE, GATE_TOL, ROUND, SEMITONES, degenerate, harmonic, harmonic_streams,  # noqa: F401  (re-exported)
                      mixed_streams, ratio_of, roundtrip_turns, tone, white)

F = 2048
FS = 48000.0
HOPS = (128, 256, 512, 1024)                # everything vp_stft_supported(2048, hop) admits with a power-of-two overlap of 2 .. 16


def bound(hop, ref):
    return 4.0 * (F // hop) * 2.0 ** -24 * max(1.0, float(np.abs(ref).max()))


def n_frames(T, hop):
    return (T - F) // hop + 1


def magnitude_ceiling(x, hop):
    """2 Mf of the amplitude bound (pv_cases.magnitude_ceiling, for F = 2048): Mf = 2 max over frames of sum_k |X_f[k]| / F."""
    x = np.asarray(x, np.float64)
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(F) / F))
    m = 0.0
    for f in range(n_frames(len(x), hop)):
        m = max(m, float(np.abs(np.fft.rfft(x[f * hop:f * hop + F] * w)).sum()))
    return 2.0 * (2.0 * m / F)


OneShotCase = namedtuple("OneShotCase", "hop semitones T what")


def _lengths(hop):
    """(T, what): the two one-frame lengths, then frame counts of every residue mod 4 (the last round holds 4, 1, 2 and 3 frames) with
    odd T (scalar loads), T = 2 mod 4 (even, but off the float4 path) and the aligned float4 path."""
    base = 8 * F // hop                                          # about eight frame lengths (a multiple of 4)

    def t_of(nf, extra):
        return F + (nf - 1) * hop + extra
    out = [(F, "one frame, T = F"), (F + hop - 1, "one frame, T = F + hop - 1 (odd, tail)"),
           (t_of(base, 0), "frames mod 4 = 0, aligned"), (t_of(base + 1, hop - 1), "frames mod 4 = 1, odd T, longest tail"),
           (t_of(base + 2, 2), "frames mod 4 = 2, T = 2 mod 4, tail of 2"), (t_of(base + 3, 3), "frames mod 4 = 3, odd T, tail of 3")]
    assert sorted(n_frames(T, hop) % 4 for T, _ in out[2:]) == [0, 1, 2, 3]
    assert out[2][0] % 4 == 0 and out[3][0] % 2 == 1 and out[4][0] % 4 == 2 and out[5][0] % 2 == 1
    return out


# three intervals per hop, always the two octaves (ratio 2 and 1/2: every second synthesis bin empty / two bins per synthesis bin)
_SEMIS_OF_HOP = {128: (12.0, -12.0, 7.0), 256: (12.0, -12.0, 0.37), 512: (12.0, -12.0, -11.99), 1024: (12.0, -12.0, 7.0)}

ONE_SHOT_CASES = [OneShotCase(hop, v, T, what) for hop in HOPS for v in _SEMIS_OF_HOP[hop] for T, what in _lengths(hop)]
assert len(ONE_SHOT_CASES) == 72


def one_shot_id(c):
    return f"hop{c.hop}-{c.semitones:+g}st-T{c.T}"


def one_shot_input(c):
    return mixed_streams(c.T, seed=c.hop + c.T)


_REF = {}


def one_shot_reference(c, x, form="radians"):
    """[S][T] float64: the restatement of tests/stft_reference.py ("radians") or pv_cases.roundtrip_turns ("turns") at F = 2048.
    Computed once per case and form (callers do not write to it)."""
    import stft_reference as R
    key = (c, form)
    if key not in _REF:
        r = ratio_of(c.semitones)
        if form == "radians":
            ref = np.stack([R.stft_roundtrip(xs, F, c.hop, ratio=r) for xs in x])
        else:
            ref = np.stack([roundtrip_turns(xs, F, c.hop, r) for xs in x])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]
