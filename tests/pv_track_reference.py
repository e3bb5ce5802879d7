"""The definition of the phase-vocoder path's pitch tracker (include/vp_amd.h vp_stft_track_pitch, kernel vp_k_yin_track), written with
the CPU oracle's exported pieces (oracle_py.yin_temp_linear, yin_pick, notes_closest).  Test infrastructure only.

A handle of S streams x T samples, frame length F, hop, nF = (T - F) // hop + 1, sample rate fs, a key per stream (0..12, 12 = chromatic;
any other value counts as 12):

  lag range   tauMax = ceil(fs / 100) (PitchProcess.cpp:100), the walk starts at floor(fs / 800) (:429);
  domain      8000 <= fs <= 51200 (tauMax <= 512) and T >= F + tauMax;
  window      frame f reads the F + tauMax samples from b_f = min(f hop, T - (F + tauMax)) on: the last frames of a row share a clamped
              window, a frame never reads outside its row;
  difference  computeYinTemp (:350-403) as vpo_yin_temp_linear states it: the float32 input widened to double,
              d[k] = sum_{i < F} (x[b + i] - x[b + i + k])^2 for k < tauMax, each its own left-to-right sum, product and add separate;
              d[0] = 1, then tmp += d[k]; d[k] *= k / tmp in increasing k; the guard slot d[tauMax] = 0;
  pick        yin_pick's threshold walk (:429-447): the period tau, or 0 for unvoiced;
  ratio       tau > 0: pitch = fs / tau, ratio = closest(pitch, key) / pitch, those two divisions (:595-596); tau = 0: ratio = 1.0.

No gate and no hold of the last voiced ratio: frames are independent.  Output: period int32 [S][nF], ratio float64 [S][nF].

Input samples that are float32 denormals are outside the tested domain: the library's default kernel build flushes them to zero when it
widens them, the oracle does not.  pv_track_cases.py asserts that its signals hold none.

MUTANTS are seeded faults of this definition (tests/test_pv_track_reference_cpu.py requires each to differ from it on a named case).
EDGE_MUTANTS are faults of the walk, the note lookup and the normalisation's last lags; they act on walk() and closest(), the two steps
written out here in Python (tests/test_pv_track_edges_cpu.py requires both to equal yin_pick and notes_closest on every case, and each
fault to differ on a named case of tests/pv_track_edge_cases.py)."""
import math

import numpy as np

from oracle import oracle_py as O

FS_MIN, FS_MAX = 8000.0, 51200.0
EDGE_MUTANTS = ("popped_zero", "popped_clamped", "tau0_exclusive", "last_lag_always_next", "word_edge", "owners_floor")
MUTANTS = ("unclamped", "no_descent", "key_ignored", "guard_nonzero", "pairwise") + EDGE_MUTANTS
YIN_TOL = 0.25


def tau_max(fs):
    return int(math.ceil(fs / 100.0))


def n_frames(T, F, hop):
    return (T - F) // hop + 1


def in_domain(fs, T, F):
    return FS_MIN <= fs <= FS_MAX and T >= F + tau_max(fs)


def norm_key(key):
    key = int(key)
    return key if 0 <= key <= 12 else 12


def _pick_no_descent(yt, tm, fs):
    for tau in range(int(math.floor(fs / 800.0)), tm):
        if yt[tau] < 0.25:
            return tau
    return 0


def _yin_pairwise(w, F, tm):
    """d by numpy's pairwise summation instead of the left-to-right sum; the normalisation as the definition's."""
    yt = np.zeros(tm + 1)
    for k in range(tm):
        d = w[:F] - w[k:k + F]
        yt[k] = np.sum(d * d)
    yt[0] = 1.0
    tmp = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(1, tm):
            tmp += yt[k]
            yt[k] *= np.float64(k) / np.float64(tmp)
    return yt


def tau_min(fs):
    return int(math.floor(fs / 800.0))


def walk(yt, tm, fs, mutant=None):
    """yin_pick's threshold walk (:429-447) in the kernel's terms -> (first, ks, tau): first is the first lag in [tau0, tauMax) under
    the tolerance (-1: none, unvoiced), ks the first lag >= first whose successor is not smaller (the guard slot yt[tauMax] = 0 is the
    last successor looked at), tau the period: the walk leaves at tauMax - 1 without looking further; started there, it looks once."""
    yt = np.asarray(yt, np.float64)[:tm + 1]
    t0 = tau_min(fs) + (1 if mutant == "tau0_exclusive" else 0)
    under = np.flatnonzero(yt[t0:tm] < YIN_TOL)
    if under.size == 0:
        return -1, -1, 0
    first = t0 + int(under[0])
    stop = ~(yt[first + 1:tm + 1] < yt[first:tm])                              # stop[j]: lag first + j, for lags first .. tauMax - 1
    if mutant == "word_edge":                                                  # the last lag of first's ballot word is not looked at
        edge = 64 * (first // 64) + 63
        if edge < tm:
            stop[edge - first] = False
    at = np.flatnonzero(stop)
    ks = first + int(at[0]) if at.size else tm                                 # (behind the guard slot nothing is smaller)
    if first + 1 >= tm:
        tau = first + 1 if (ks > first or mutant == "last_lag_always_next") else first
    else:
        tau = min(ks, tm - 1)
    return first, ks, tau


_NOTES = {}


def notes_table(key):
    """(freq float64 [89], n) of a key: n entries and the popped one behind them (Notes.cpp:27-60)."""
    if key not in _NOTES:
        f, n = O.notes_build(key)
        f.setflags(write=False)
        _NOTES[key] = (f, n)
    return _NOTES[key]


def closest(pitch, key, mutant=None):
    """Notes::getClosestFreq (Notes.cpp:79-110) -> (closest frequency, idx): idx = lower_bound = entries below the pitch; idx == n
    compares the popped slot freq[n] with the top entry (:99)."""
    f, n = notes_table(key)
    idx = int(np.count_nonzero(f[:n] < pitch))
    at = min(idx, n - 1) if mutant == "popped_clamped" else idx
    fi = 0.0 if (mutant == "popped_zero" and at == n) else float(f[at])
    if at > 0 and not (abs(fi - pitch) <= abs(float(f[at - 1]) - pitch)):
        return float(f[at - 1]), idx
    return fi, idx


def decide(yt, tm, fs, key, mutant=None):
    """One frame's decision from its normalised function, by walk() and closest() -> (first, ks, tau, idx, ratio)."""
    first, ks, tau = walk(yt, tm, fs, mutant)
    if tau <= 0:
        return first, ks, tau, -1, 1.0
    pitch = fs / tau
    c, idx = closest(pitch, key, mutant)
    return first, ks, tau, idx, c / pitch


def _owners_floor(yt, w, F, tm):
    """The fault 'owners_floor': the lags from 8 floor(tauMax / 8) on are divided by a running sum of 1 (their owner lane never ran)."""
    yt = yt.copy()
    for k in range(8 * (tm // 8), tm):
        d = w[:F] - w[k:k + F]
        yt[k] = float(np.cumsum(d * d)[-1]) * (np.float64(k) / 1.0)           # (cumsum adds left to right: the definition's d[k])
    return yt


def frame_function(x, f, fs, F, hop, mutant=None):
    """The normalised difference function of frame f of one row x (float32 [T]): float64 [tauMax + 1], guard slot included."""
    tm, T = tau_max(fs), len(x)
    n = F + tm
    if mutant == "unclamped":
        w = np.zeros(n)
        seg = np.asarray(x[f * hop:f * hop + n], np.float64)
        w[:len(seg)] = seg
    else:
        b = min(f * hop, T - n)
        w = np.asarray(x[b:b + n], np.float64)
    yt = _yin_pairwise(w, F, tm) if mutant == "pairwise" else O.yin_temp_linear(w, F, tm)
    if mutant == "owners_floor":
        yt = _owners_floor(yt, w, F, tm)
    yt[tm] = 1.0 if mutant == "guard_nonzero" else 0.0
    return yt


def track(x, fs, F, hop, keys=None, mutant=None, with_function=False, detail=None):
    """x float32 [S][T] -> (period int32 [S][nF], ratio float64 [S][nF]) [, function float64 [S][nF][tauMax + 1]].
    detail: a dict that receives int32 [S][nF] tables "first", "ks", "idx" and "notesN" (-1 where a frame has none); the period and the
    ratio then come from walk() and closest() instead of the oracle's yin_pick and notes_closest, as they do under an EDGE_MUTANT."""
    assert mutant is None or mutant in MUTANTS, mutant
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2, (x.dtype, x.shape)
    S, T = x.shape
    assert in_domain(fs, T, F), (fs, T, F)
    if keys is None:
        keys = [12] * S
    elif np.ndim(keys) == 0:
        keys = [int(keys)] * S
    assert len(keys) == S
    tm, nF = tau_max(fs), n_frames(T, F, hop)
    period, ratio = np.zeros((S, nF), np.int32), np.ones((S, nF), np.float64)
    fn = np.zeros((S, nF, tm + 1)) if with_function else None
    python = (detail is not None or mutant in EDGE_MUTANTS) and mutant != "no_descent"
    if detail is not None:
        for name in ("first", "ks", "idx", "notesN"):
            detail[name] = np.full((S, nF), -1, np.int32)
    for s in range(S):
        key = 12 if mutant == "key_ignored" else norm_key(keys[s])
        for f in range(nF):
            yt = frame_function(x[s], f, fs, F, hop, mutant)
            first = ks = idx = -1
            if python:
                first, ks, tau, idx, ratio[s, f] = decide(yt, tm, fs, key, mutant)
            else:
                tau = _pick_no_descent(yt, tm, fs) if mutant == "no_descent" else O.yin_pick(yt, tm, fs)
                if tau > 0:
                    pitch = fs / tau
                    ratio[s, f] = O.notes_closest(pitch, key) / pitch
            if with_function:
                fn[s, f] = yt
            period[s, f] = tau
            if detail is not None:
                detail["first"][s, f], detail["ks"][s, f], detail["idx"][s, f], detail["notesN"][s, f] = first, ks, idx, notes_table(key)[1]
    return (period, ratio, fn) if with_function else (period, ratio)


def semitones(ratio):
    return 12.0 * np.log2(np.asarray(ratio, np.float64))
