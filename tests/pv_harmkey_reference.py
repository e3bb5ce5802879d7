"""The definition of the key-aware voices of the pitch tracker (include/vp_amd.h vp_stft_track_harmony, kernel vp_k_yin_track_voices):
one pitch decision per frame, V ratios at scale degrees of the note the tracker chose.  Everything up to the period is
tests/pv_track_reference.py's definition, imported and not restated.  Test infrastructure only.

  harmony table  per key k (0 .. 12, anything else counts as 12): H_k, hN_k = notes_build(k, 25.0, 3200.0), the recurrence of the
                 tracker's table notes_build(k, 100.0, 800.0) through a wider filter.  The tracker's table (its n entries and the popped
                 slot) is the slice H_k[off_k : off_k + n_k + 1], bit for bit; off_k + n_k + 12 <= hN_k - 1 in every key;
  voiced frame   tau > 0, pitch = fs / tau.  c: the index, in the tracker's table, of the entry getClosestFreq returns (0 .. n; n is the
                 popped slot).  Voice v has an integer degree d[s][v], clamped to -12 .. 12, in steps of the key's table (scale degrees
                 in the 12 scale keys, semitones in the chromatic key).  j = max(off + c + d, 0); ratio[s][v][f] = H_k[j] / pitch, that
                 one division.  Degree 0 gives the tracker's ratio bit for bit;
  unvoiced frame tau = 0: ratio[s][v][f] = u[s][v], a caller-given double per stream and voice; no table means 1.0, a NaN or an
                 infinity counts as 1.0.  No hold and no smoothing, like the batch tracker.

Output: period int32 [S][nF], ratio float64 [S][V][nF] (the layout vp_stft_harmonize takes).  The ratios are not clamped here.

MUTANTS are seeded faults of this definition (tests/test_pv_harmkey_reference_cpu.py requires each to differ from it on a case named in
tests/pv_harmkey_cases.py):
  parallel                the ratio is closest 2^(d' / 12) / pitch with d' the mean step (d in the chromatic key, 12 d / 7 in a scale key);
  index_from_lower_bound  the lookup's lower bound idx stands where the definition uses c;
  no_lower_clamp          a negative j wraps to the table's end;
  popped_as_top           c = n is treated as n - 1;
  unvoiced_one            u is ignored."""
import math

import numpy as np

from oracle import oracle_py as O
import pv_track_reference as R

MUTANTS = ("parallel", "index_from_lower_bound", "no_lower_clamp", "popped_as_top", "unvoiced_one")
MAX_VOICES = 4
MAX_DEGREE = 12
HARM_FMIN, HARM_FMAX = 25.0, 3200.0
STRIDE = 89

_HARM = {}


def harmony_table(key):
    """(H float64 [89], hN, off) of a key: hN entries and the popped one behind them; off: the tracker table's entry 0 in H."""
    key = R.norm_key(key)
    if key not in _HARM:
        H, hN = O.notes_build(key, HARM_FMIN, HARM_FMAX)
        f, n = R.notes_table(key)
        off = int(np.flatnonzero(H[:hN + 1] == f[0])[0])
        H.setflags(write=False)
        _HARM[key] = (H, hN, off)
    return _HARM[key]


def chosen_index(pitch, key):
    """c: the index in the tracker's table of the entry Notes::getClosestFreq returns for `pitch`, and the lookup's lower bound idx."""
    f, n = R.notes_table(key)
    cf, idx = R.closest(pitch, key)
    c = idx
    if idx > 0 and not (abs(float(f[idx]) - pitch) <= abs(float(f[idx - 1]) - pitch)):
        c = idx - 1
    assert float(f[c]) == cf, (pitch, key, c, idx)
    return c, idx


def sane_unvoiced(u):
    u = float(u)
    return u if math.isfinite(u) else 1.0


def voice_ratios(tau, fs, key, degrees, unvoiced=None, mutant=None):
    """The voice stage of one frame: its period, the stream's key, degrees [V] and unvoiced [V] or None -> ratio float64 [V]."""
    key = R.norm_key(key)
    V = len(degrees)
    out = np.ones(V, np.float64)
    if tau <= 0:
        if unvoiced is not None and mutant != "unvoiced_one":
            out[:] = [sane_unvoiced(u) for u in unvoiced]
        return out
    pitch = fs / tau
    H, hN, off = harmony_table(key)
    n = R.notes_table(key)[1]
    c, idx = chosen_index(pitch, key)
    if mutant == "index_from_lower_bound":
        c = idx
    if mutant == "popped_as_top" and c == n:
        c = n - 1
    for v in range(V):
        d = max(-MAX_DEGREE, min(MAX_DEGREE, int(degrees[v])))
        if mutant == "parallel":
            mean = float(d) if key == 12 else 12.0 * d / 7.0
            out[v] = float(H[off + c]) * 2.0 ** (mean / 12.0) / pitch
            continue
        j = off + c + d
        if j < 0:
            j = j % STRIDE if mutant == "no_lower_clamp" else 0
        assert j <= hN or mutant == "no_lower_clamp"                            # (the upper bound cannot bind)
        out[v] = float(H[j]) / pitch
    return out


def _tables(x_S, degrees, keys, unvoiced):
    S = x_S
    if keys is None:
        keys = [12] * S
    elif np.ndim(keys) == 0:
        keys = [int(keys)] * S
    degrees = np.asarray(degrees)
    assert degrees.dtype.kind in "iu"
    if degrees.ndim == 1:
        degrees = np.broadcast_to(degrees, (S, len(degrees)))
    assert degrees.ndim == 2 and degrees.shape[0] == S and 1 <= degrees.shape[1] <= MAX_VOICES and len(keys) == S, (degrees.shape, S)
    if unvoiced is not None:
        unvoiced = np.asarray(unvoiced, np.float64)
        assert unvoiced.shape == degrees.shape, unvoiced.shape
    return keys, degrees, unvoiced


def track_harmony(x, fs, F, hop, degrees, keys=None, unvoiced=None, mutant=None):
    """x float32 [S][T], degrees int [V] or [S][V], unvoiced float64 [S][V] or None -> (period int32 [S][nF], ratio float64 [S][V][nF])."""
    assert mutant is None or mutant in MUTANTS, mutant
    x = np.asarray(x)
    S = x.shape[0]
    keys, degrees, unvoiced = _tables(S, degrees, keys, unvoiced)
    period, _ = R.track(x, fs, F, hop, keys)
    V, nF = degrees.shape[1], period.shape[1]
    ratio = np.ones((S, V, nF), np.float64)
    for s in range(S):
        for f in range(nF):
            ratio[s, :, f] = voice_ratios(int(period[s, f]), fs, keys[s], degrees[s], None if unvoiced is None else unvoiced[s], mutant)
    return period, ratio


def nominal_unvoiced(degrees, keys, S):
    """The nominal interval of every voice, what the Python front ends pass for unvoiced=None: 2^(d / 12) in the chromatic key,
    2^(round(12 d / 7) / 12) in a scale key -> float64 [S][V]."""
    keys, degrees, _ = _tables(S, degrees, keys, None)
    out = np.ones(degrees.shape, np.float64)
    for s in range(S):
        for v in range(degrees.shape[1]):
            d = max(-MAX_DEGREE, min(MAX_DEGREE, int(degrees[s, v])))
            semis = float(d) if R.norm_key(keys[s]) == 12 else float(np.floor(12.0 * d / 7.0 + 0.5))
            out[s, v] = 2.0 ** (semis / 12.0)
    return out
