"""Build-authored NumPy restatement of the phase-vocoder TIME STRETCH (vp_stft_time_stretch; kernels vp_k_stft_pv_stretch and
vp_k_stft_pv2k_stretch of csrc/vp_stft_stretch.inc): no reference counterpart, parity unpinned by nature.  Test
infrastructure only.

The stage is stft_reference.stft_roundtrip(x, F, hop, ratio) with exactly these changes.  The output row has T samples, nF = (T - F) //
hop + 1 frames are written and samples no frame covers stay 0; the input x has n_in >= F samples; pos is an integer table [nF].
  position   frame f is x[q_f : q_f + F], q_f = clamp(pos[f], 0, n_in - F); it is still overlap-added at output offset f hop.  Window,
             1 / sum w^2 scale, rounds of four frames, the gather, real bins 0 and F / 2: unchanged.
  advance    D_0 = hop; D_f = clamp(q_f - q_(f-1), 1, F) for f >= 1 (any table is defined and finite).
  unwrap     in turns: d = (p - p_prev) / 2 pi - (k D_f) / F; d -= rint(d); fk = k + d (F / D_f).  The nominal term is the UNREDUCED
             exact quotient (an integer product over a power of two); at D_f = hop it is stft_roundtrip's k (1 / O).
  synthesis  inc = sf / O turns, as it was: the synthesis hop is hop.

Two statements, as for every phase-vocoder reference here: "radians" (the accumulator, cos and sin in radians, the gather a loop: the
form of stft_reference.py) and "turns" (the accumulator in turns, exp(2 pi i frac), the gather vectorised: the form of
pv_cases._turns_frame).  BOTH take the unwrap's nominal term as the exact (k D) / F and the phase difference as (p - p_prev) / TWO_PI.
Bins 0 and F / 2 are real, their phases exactly 0 or half a turn on both sides, so for them d lands exactly on +-1/2 whenever (k D) / F
is a half-integer or the bin's sign flips; with k (2 pi D / F) in the radians form, or with the nominal term reduced mod 1, the tie
breaks differently in the two forms (measured: up to 4e-3 apart).

advance="hop" is the MUTANT the teeth test needs: a stage that unwraps with hop instead of D_f.  Four more MUTANTS, the plausible wrong
kernels at the clamps (tests/pv_stretch_cases.py's edge tables reach them): "nohigh" D_f = max(step, 1), no upper clamp; "abs" D_f =
clamp(|step|, 1, F); "lowhop" a step below 1 becomes hop; "qmax-1" q clamped to n_in - F - 1.  The default "delta" is the definition.
"""
import numpy as np

from stft_reference import ROUND, TWO_PI, window


def clamp_positions(pos, n_in, F):
    return np.clip(np.asarray(pos, np.int64), 0, n_in - F)


ADVANCES = ("delta", "hop", "nohigh", "abs", "lowhop", "qmax-1")


def advances(q, hop, F, advance="delta"):
    """D_f of the clamped positions q; advance: "delta" (the definition) or a mutant's."""
    d = np.empty(len(q), np.int64)
    d[:1] = hop
    step = np.diff(q)
    if advance == "hop":
        d[1:] = hop
    elif advance == "nohigh":
        d[1:] = np.maximum(step, 1)
    elif advance == "abs":
        d[1:] = np.clip(np.abs(step), 1, F)
    elif advance == "lowhop":
        d[1:] = np.minimum(np.where(step < 1, hop, step), F)
    else:
        d[1:] = np.clip(step, 1, F)
    return d


def _gather_loop(m, fk, ratio, nb):
    idx = np.floor(np.arange(nb) * ratio + 0.5).astype(np.int64)
    sm, sf = np.zeros(nb), np.zeros(nb)
    for kk in range(nb):                             # increasing k: magnitudes add, the last frequency stays
        t = idx[kk]
        if 0 <= t < nb:
            sm[t] += m[kk]
            sf[t] = fk[kk] * ratio
    return sm, sf


def _gather_vector(m, fk, ratio, nb):
    k = np.arange(nb)
    tgt = np.floor(k * ratio + 0.5).astype(np.int64)
    ok = (tgt >= 0) & (tgt < nb)
    sm = np.zeros(nb)
    np.add.at(sm, tgt[ok], m[ok])
    last = np.full(nb, -1)
    np.maximum.at(last, tgt[ok], k[ok])
    return sm, np.where(last >= 0, fk[np.maximum(last, 0)] * ratio, 0.0)


def stretch_roundtrip(x, pos, T, F=1024, hop=256, ratio=1.0, form="radians", advance="delta"):
    """x: float [n_in], pos: int [nF] -> float64 [T]."""
    x = np.asarray(x, np.float64)
    n_in = len(x)
    nF = (T - F) // hop + 1
    assert n_in >= F and len(pos) == nF and form in ("radians", "turns") and advance in ADVANCES
    q = clamp_positions(pos, n_in - 1, F) if advance == "qmax-1" else clamp_positions(pos, n_in, F)
    D = advances(q, hop, F, advance)
    w = window(F)
    scale = 1.0 / np.sum(w[::hop] ** 2)
    nb, O = F // 2 + 1, F // hop
    k = np.arange(nb)
    y = np.zeros(T)
    p_prev, carry, sp = np.zeros(nb), np.zeros(nb), np.zeros(nb)
    for f in range(nF):
        X = np.fft.rfft(x[q[f]:q[f] + F] * w)
        m, p = np.abs(X), np.arctan2(X.imag, X.real)
        d = (p - p_prev) / TWO_PI - (k * int(D[f])) / F
        d -= np.rint(d)
        fk = k + d * (F / int(D[f]))
        p_prev = p
        if form == "radians":
            sm, sf = _gather_loop(m, fk, ratio, nb)
            inc = (TWO_PI / O) * sf
            sp = carry + inc if f % ROUND == 0 else sp + inc
            if f % ROUND == ROUND - 1 or f == nF - 1:
                carry = sp - TWO_PI * np.rint(sp * (1.0 / TWO_PI))
            Y = sm * (np.cos(sp) + 1j * np.sin(sp))
        else:
            sm, sf = _gather_vector(m, fk, ratio, nb)
            inc = sf / O
            sp = carry + inc if f % ROUND == 0 else sp + inc
            frac = sp - np.rint(sp)
            if f % ROUND == ROUND - 1:
                carry = frac
            Y = sm * np.exp(2j * np.pi * frac)
        Y[0] = Y[0].real
        Y[-1] = Y[-1].real
        y[f * hop:f * hop + F] += np.fft.irfft(Y, F) * w
    return y * scale


def stretch_positions(n_frames, hop, stretch, n_in, frame_len):
    """The formula of vp_stretch_positions: pos[f] = min(floor(f hop / stretch), n_in - frame_len), int32 [n_frames]."""
    return np.minimum(np.floor(np.arange(n_frames, dtype=np.int64) * hop / float(stretch)), n_in - frame_len).astype(np.int32)
