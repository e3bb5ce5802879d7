"""The definition of the FINE pitch tracker (include/vp_amd.h vp_stft_track_pitch_fine and VP_TRACK_FINE, kernels vp_k_yin_track_fine and
vp_k_yin_track_voices_fine of csrc/vp_track_fine_kernels.inc): tests/pv_track_reference.py's decision, imported and not restated, then the
period refined below one sample by a parabola through the normalised function around its minimum (step 5 of the YIN paper), and the note
looked up again on the refined pitch.  Test infrastructure only.

With yt the frame's normalised function d' (float64 [tauMax + 1], guard slot yt[tauMax] = 0) and tau > 0 the integer period of the walk:

  a = yt[tau - 1]; b = yt[tau]; c = yt[tau + 1]
  refine  iff  tau - 1 >= 1 and tau + 1 <= tauMax - 1      neither lag 0 (d'[0] = 1 by decree) nor the guard slot is a neighbour
          and  a >= b and c >= b                            tau is a local minimum of the sampled function
          and  den = (a - b) + (c - b) is > 0 and <= DBL_MAX
  delta     = (0.5 * (a - c)) / den                         each operation rounded on its own; |delta| <= 0.5
  tau_fine  = float(tau) + delta  if refined, else float(tau)
  pitch     = fs / tau_fine
  ratio     = closest(pitch, key) / pitch                   Notes::getClosestFreq again, on the refined pitch

A NaN fails a comparison, so the frame keeps the integer period.  An unvoiced frame keeps period 0, tau_fine 0.0 and ratio 1.0.  Near the
midpoint between two notes the fine tracker may choose another note than the integer one: that is intended.

Why on d' and not on the raw difference function: the walk chose tau as a minimum of d', and d'[k] = d[k] k / cumsum, whose slowly
varying factor moves the minimum; a parabola through the raw d would interpolate another function than the one that was minimised.
Why the skipped cases: d'[0] = 1 and the guard slot d'[tauMax] = 0 are not samples of the function; a left neighbour below b means the
walk started its descent on the far side of the true minimum (a pitch above fMax's lag tau0), where the parabola would extrapolate.

The voices (vp_stft_track_harmony under VP_TRACK_FINE): tests/pv_harmkey_reference.py's voice_ratios with tau_fine in place of tau -- its
statements divide by the period and look the note up on fs / period, so the chosen note index comes from the refined pitch.

MUTANTS are seeded faults of this definition (tests/test_pv_track_fine_reference_cpu.py requires each to differ from it on a named case):
  delta_sign        tau_fine = tau - delta;
  association       the denominator as (a - 2 b) + c;
  guard_neighbour   refinement not skipped when tau + 1 is the guard slot;
  left_lower        refinement not skipped when the left neighbour is lower;
  note_on_integer   the note looked up on fs / tau, the division by the refined pitch."""
import numpy as np

from oracle import oracle_py as O
import pv_harmkey_reference as HR
import pv_track_reference as R

MUTANTS = ("delta_sign", "association", "guard_neighbour", "left_lower", "note_on_integer")
BRANCHES = ("refined", "edge", "left_lower", "flat", "unvoiced")
DBL_MAX = float(np.finfo(np.float64).max)


def refine(yt, tau, tm, mutant=None):
    """The rule -> (tau_fine, branch): "refined"; "edge" (lag 0 or the guard slot would be a neighbour); "left_lower" (a < b); "flat"
    (c < b, a denominator that is not positive and finite, or a NaN); "unvoiced" (tau <= 0: tau_fine 0.0)."""
    assert mutant is None or mutant in MUTANTS, mutant
    tau = int(tau)
    if tau <= 0:
        return 0.0, "unvoiced"
    top = tm if mutant == "guard_neighbour" else tm - 1
    if not (tau - 1 >= 1 and tau + 1 <= top):
        return float(tau), "edge"
    a, b, c = np.float64(yt[tau - 1]), np.float64(yt[tau]), np.float64(yt[tau + 1])
    with np.errstate(all="ignore"):
        if not (a >= b) and mutant != "left_lower":
            return float(tau), "flat" if np.isnan(a) or np.isnan(b) else "left_lower"
        if not (c >= b):
            return float(tau), "flat"
        den = (a - np.float64(2.0) * b) + c if mutant == "association" else (a - b) + (c - b)
        if not (den > 0.0 and den <= DBL_MAX):
            return float(tau), "flat"
        delta = (np.float64(0.5) * (a - c)) / den
    return float(np.float64(tau) - delta if mutant == "delta_sign" else np.float64(tau) + delta), "refined"


def ratio_of(tau, tau_fine, fs, key, mutant=None):
    """The ratio of a voiced frame from its refined period (and, under the fault, its integer one)."""
    pitch = fs / tau_fine
    return O.notes_closest(fs / tau if mutant == "note_on_integer" else pitch, key) / pitch


def decide(yt, tm, fs, key, mutant=None):
    """One frame's decision from its normalised function -> (tau, tau_fine, ratio, branch)."""
    tau = O.yin_pick(yt, tm, fs)
    tf, br = refine(yt, tau, tm, mutant)
    return tau, tf, (ratio_of(tau, tf, fs, key, mutant) if tau > 0 else 1.0), br


def _keys(keys, S):
    if keys is None:
        return [12] * S
    if np.ndim(keys) == 0:
        return [int(keys)] * S
    assert len(keys) == S
    return list(keys)


def track_fine(x, fs, F, hop, keys=None, mutant=None, branches=None):
    """x float32 [S][T] -> (period int32 [S][nF], period_fine float64 [S][nF], ratio float64 [S][nF]).  branches: a list that receives
    [S][nF] branch names."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2, (x.dtype, x.shape)
    S, T = x.shape
    assert R.in_domain(fs, T, F), (fs, T, F)
    keys = _keys(keys, S)
    tm, nF = R.tau_max(fs), R.n_frames(T, F, hop)
    period, fine, ratio = np.zeros((S, nF), np.int32), np.zeros((S, nF), np.float64), np.ones((S, nF), np.float64)
    for s in range(S):
        row = []
        for f in range(nF):
            period[s, f], fine[s, f], ratio[s, f], br = decide(R.frame_function(x[s], f, fs, F, hop), tm, fs, R.norm_key(keys[s]), mutant)
            row.append(br)
        if branches is not None:
            branches.append(row)
    return period, fine, ratio


def voice_ratios_fine(tau_fine, fs, key, degrees, unvoiced=None):
    """pv_harmkey_reference's table entry over the refined pitch; the chosen note index comes from the lookup on the refined pitch."""
    return HR.voice_ratios(float(tau_fine), fs, key, degrees, unvoiced)


def track_harmony_fine(x, fs, F, hop, degrees, keys=None, unvoiced=None):
    """x float32 [S][T], degrees int [V] or [S][V], unvoiced float64 [S][V] or None -> (period int32 [S][nF], ratio float64 [S][V][nF])."""
    x = np.asarray(x)
    S = x.shape[0]
    keys, degrees, unvoiced = HR._tables(S, degrees, keys, unvoiced)
    period, fine, _ = track_fine(x, fs, F, hop, keys)
    V, nF = degrees.shape[1], period.shape[1]
    ratio = np.ones((S, V, nF), np.float64)
    for s in range(S):
        for f in range(nF):
            ratio[s, :, f] = voice_ratios_fine(fine[s, f], fs, keys[s], degrees[s], None if unvoiced is None else unvoiced[s])
    return period, ratio


def cents(pitch, true):
    return 1200.0 * np.log2(np.asarray(pitch, np.float64) / true)
