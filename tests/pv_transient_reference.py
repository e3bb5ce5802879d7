"""Build-authored NumPy definition of the TRANSIENT-PRESERVING locked time stretch (vp_stft_onset_flux, vp_onset_pick,
vp_stretch_positions_transient, vp_stft_time_stretch_locked_reset; kernels vp_k_stft_onset_flux of csrc/vp_stft_onset.inc and
vp_k_stft_pv_stretch_lock_reset of csrc/vp_stft_stretch_reset.inc).  No reference counterpart -- parity unpinned by
nature.  Test infrastructure only.

The scheme: do not stretch across an attack, and restart the phases at it.

  onset_flux(x, F, hop) -> flux[nG], mass[nG]        nG = (n_in - F) // hop + 1, the input's OWN frame grid g hop
      M_g = |rfft(x[g hop : g hop + F] window(F))|, bins 0 .. F / 2;  mass[g] = sum_k M_g[k];
      flux[0] = 0, flux[g] = sum_k max(M_g[k] - M_(g-1)[k], 0): the rectified spectral flux.

  pick_onsets(flux, mass, thr) -> uint8[nG]          thr in [0, 1]
      frame g is an onset iff  flux[g] > 0,  flux[g] >= thr mass[g],  flux[g] > flux[g-1]  and  flux[g] >= flux[g+1];
      a missing neighbour counts as -inf, a NaN anywhere in a comparison is "no".

  plan_positions(onsets, nF, hop, stretch, n_in, F, K) -> pos int32[nF], reset uint8[nF]      K in [1, 8], default max(F / (2 hop), 1)
      base[f] = min(floor(f hop / stretch), n_in - F): vp_stretch_positions's formula, in double.  Anchors start as [(0, 0)].  The onsets g
      in increasing order: fc = floor(g stretch + 0.5), a = fc - K, b = fc + K; g is accepted iff
          g - K >= 0,  g + K <= nG - 1,  a > the last anchor's frame,  b < nF - 1,
          (g - K) hop >= the last anchor's position,  (g + K) hop <= base[nF - 1];
      then the anchors (a, (g - K) hop) and (b, (g + K) hop) are appended and reset[a] = 1.  The last anchor is (nF - 1, base[nF - 1]).
      Between consecutive anchors (f0, p0), (f1, p1): pos[f] = p0 + ((f - f0) (p1 - p0)) // (f1 - f0), in 64-bit integers: a span comes
      out exactly hop apart, the table is non-decreasing.  WITH NO ACCEPTED ONSET THE TABLE IS THE TWO-ANCHOR LINE from (0, 0) to
      (nF - 1, base[nF - 1]), not `base` (they differ where floor(f hop / stretch) and the integer line round apart, and where base clamps).

  stretch_locked_reset_roundtrip(x, pos, T, ratio, reset)
      tests/pv_stretch_lock_reference.py's stretch_locked_roundtrip with ONE change in rule 4: on a frame with reset[f] != 0, th[P] = 0 for
      every peak P (instead of theta[P] + nu[P] (r hop - D) / F, wrapped).  Everything else is unchanged: pprev = p on every frame,
      theta[k] = th[own[k]], and a frame without peaks gives Y = 0 and leaves theta, flagged or not.
      At ratio 1 and D = hop the advance nu (r hop - D) / F is exactly 0, so theta stays 0 through a span that starts with a reset: the
      stage is the identity there, Y = X bit for bit.

Two statements of the stage, as for every phase-vocoder reference here: stretch_locked_reset_roundtrip (turns, rfft, vectorised) and
stretch_locked_reset_roundtrip_b (radians, the full complex fft, explicit loops).

`mutant` names a deliberately wrong variant (the tests' teeth; tests/pv_transient_cases.py names the case that sees each):
  stage   noreset     the reset forgotten                 late_reset  the reset one frame late
          reset_prev  the reset zeroes pprev too
  flux    norect      the flux without rectification      flux_next   the flux against frame g + 1
  pick    pick_ge     flux[g] >= flux[g-1] on the left
  plan    fc_floor    fc = floor(g stretch)               span_short  the span K - 1

Out of scope: a streaming form, 2048-point frames, sub-bin offsets, single precision, detection on the device end to end, resets in the
pitch-shift-only calls.
"""
import numpy as np

import pv_lock_reference as LR
import pv_stretch_reference as SR
from stft_reference import TWO_PI, window

STAGE_MUTANTS = ("noreset", "late_reset", "reset_prev")
FLUX_MUTANTS = ("norect", "flux_next")
PICK_MUTANTS = ("pick_ge",)
PLAN_MUTANTS = ("fc_floor", "span_short")
MUTANTS = STAGE_MUTANTS + FLUX_MUTANTS + PICK_MUTANTS + PLAN_MUTANTS
K_MIN, K_MAX = 1, 8


def default_span(F, hop):
    return max(F // (2 * hop), 1)


# ---- 1. the onset flux ----------------------------------------------------------------------------------------------------------------------
def frame_magnitudes(x, F, hop):
    """M [nG][F / 2 + 1] over the input's own grid."""
    x = np.asarray(x, np.float64)
    nG = (len(x) - F) // hop + 1
    assert nG >= 1, len(x)
    w = window(F)
    return np.stack([np.abs(np.fft.rfft(x[g * hop:g * hop + F] * w)) for g in range(nG)])


def onset_flux(x, F=1024, hop=256, mutant=None):
    assert mutant is None or mutant in FLUX_MUTANTS, mutant
    M = frame_magnitudes(x, F, hop)
    mass = M.sum(axis=1)
    flux = np.zeros(len(M))
    for g in range(1, len(M)):
        if mutant == "flux_next":
            d = M[min(g + 1, len(M) - 1)] - M[g]
        else:
            d = M[g] - M[g - 1]
        flux[g] = (d if mutant == "norect" else np.maximum(d, 0.0)).sum()
    return flux, mass


def flux_bound(x, F, hop):
    """The derived bound of a double-precision implementation's flux[g] and mass[g] against onset_flux, per frame [nG]:
    4 * 513 * log2(F) * 2^-53 * (||x_g w||_2 + ||x_(g-1) w||_2)  (x_(-1) = 0)."""
    x = np.asarray(x, np.float64)
    nG = (len(x) - F) // hop + 1
    w = window(F)
    n = np.array([np.sqrt(np.sum((x[g * hop:g * hop + F] * w) ** 2)) for g in range(nG)])
    return 4.0 * (F // 2 + 1) * np.log2(F) * 2.0 ** -53 * (n + np.concatenate(([0.0], n[:-1])))


# ---- 2. the pick ------------------------------------------------------------------------------------------------------------------------------
def pick_onsets(flux, mass, thr, mutant=None):
    assert mutant is None or mutant in PICK_MUTANTS, mutant
    flux, mass = np.asarray(flux, np.float64), np.asarray(mass, np.float64)
    assert flux.shape == mass.shape and flux.ndim == 1 and 0.0 <= thr <= 1.0
    n = len(flux)
    out = np.zeros(n, np.uint8)
    with np.errstate(invalid="ignore"):
        for g in range(n):
            left = -np.inf if g == 0 else flux[g - 1]
            right = -np.inf if g == n - 1 else flux[g + 1]
            rises = flux[g] >= left if mutant == "pick_ge" else flux[g] > left
            out[g] = bool(flux[g] > 0.0) and bool(flux[g] >= thr * mass[g]) and bool(rises) and bool(flux[g] >= right)
    return out


def pick_margins(flux, mass, thr):
    """The distance of every comparison of every frame from its edge, relative to mass[g]: [nG][4] (inf for a missing neighbour)."""
    flux, mass = np.asarray(flux, np.float64), np.asarray(mass, np.float64)
    n = len(flux)
    m = np.full((n, 4), np.inf)
    for g in range(n):
        s = mass[g] if mass[g] > 0 else 1.0
        m[g, 0] = abs(flux[g]) / s
        m[g, 1] = abs(flux[g] - thr * mass[g]) / s
        if g > 0:
            m[g, 2] = abs(flux[g] - flux[g - 1]) / s
        if g < n - 1:
            m[g, 3] = abs(flux[g] - flux[g + 1]) / s
    return m


# ---- 3. the plan ------------------------------------------------------------------------------------------------------------------------------
def plan_positions(onsets, nF, hop, stretch, n_in, F=1024, K=None, mutant=None, why=None):
    """-> pos int32 [nF], reset uint8 [nF].  `why`: a list that receives, per onset, the name of the first condition that rejected it
    (or "accepted")."""
    assert mutant is None or mutant in PLAN_MUTANTS, mutant
    K = default_span(F, hop) if K is None else int(K)
    assert K_MIN <= K <= K_MAX and nF >= 0 and n_in >= F and 0.25 <= stretch <= 4.0
    nG = (n_in - F) // hop + 1
    onsets = np.asarray(onsets)
    assert onsets.shape == (nG,), (onsets.shape, nG)
    pos, reset = np.zeros(nF, np.int32), np.zeros(nF, np.uint8)
    if nF == 0:
        return pos, reset
    base_last = min(int(np.floor(float((nF - 1) * hop) / float(stretch))), n_in - F)
    Ks = K - 1 if mutant == "span_short" else K
    anchors = [(0, 0)]
    for g in np.nonzero(onsets)[0]:
        g = int(g)
        fc = int(np.floor(g * float(stretch))) if mutant == "fc_floor" else int(np.floor(g * float(stretch) + 0.5))
        a, b = fc - Ks, fc + Ks
        lf, lp = anchors[-1]
        conds = (("g-K", g - Ks >= 0), ("g+K", g + Ks <= nG - 1), ("a", a > lf), ("b", b < nF - 1),
                 ("pos-lo", (g - Ks) * hop >= lp), ("pos-hi", (g + Ks) * hop <= base_last))
        bad = [name for name, ok in conds if not ok]
        if why is not None:
            why.append(bad[0] if bad else "accepted")
        if bad:
            continue
        anchors += [(a, (g - Ks) * hop), (b, (g + Ks) * hop)]
        reset[a] = 1
    if nF - 1 > anchors[-1][0]:
        anchors.append((nF - 1, base_last))
    for (f0, p0), (f1, p1) in zip(anchors[:-1], anchors[1:]):
        for f in range(f0, f1 + 1):
            pos[f] = p0 + ((f - f0) * (p1 - p0)) // (f1 - f0)
    return pos, reset


def spans(reset, K):
    """[(a, b)] of the plan's spans (the first and last frame of each), from its reset flags."""
    return [(int(a), int(a) + 2 * K) for a in np.nonzero(reset)[0]]


# ---- 4. the stage with the reset ----------------------------------------------------------------------------------------------------------------
def reset_stage(X, r, D, st, F, hop, flagged, mutant=None):
    """pv_stretch_lock_reference.stretch_lock_stage with the reset: one frame, st (LR.LockState) is updated, returns Y."""
    nb = len(X)
    N = nb - 1
    k = np.arange(nb)
    m = np.abs(X)
    p = np.arctan2(X.imag, X.real) / TWO_PI
    d = p - st.pprev - (k * D) / F
    d -= np.rint(d)
    nu = k + d * (F / D)
    mp = np.concatenate(([-1.0, -1.0], m, [-1.0, -1.0]))
    c = mp[2:-2]
    pk = (c > 0) & (c > mp[1:-3]) & (c > mp[0:-4]) & (c >= mp[3:-1]) & (c >= mp[4:])
    P = np.nonzero(pk)[0]
    st.pprev = np.zeros(nb) if (mutant == "reset_prev" and flagged) else p
    Y = np.zeros(nb, complex)
    if len(P) == 0:
        return Y
    own = LR.nearest(P, nb)
    newth = np.zeros(nb)
    if not flagged:                                               # rule 4; reset: th[P] = 0 for every peak
        t = st.theta[P] + nu[P] * ((r * hop - D) * (1.0 / F))
        newth[P] = t - np.rint(t)
    Pp = np.floor(P * r + 0.5).astype(np.int64)
    keep = Pp <= N
    Ps, Pa = Pp[keep], P[keep]
    if len(Ps):
        src = np.zeros(nb, np.int64)
        src[Ps] = Pa
        owns = LR.nearest(Ps, nb)
        pa = src[owns]
        kk = k - (owns - pa)
        kc = np.clip(kk, 0, N)
        ok = (kk >= 0) & (kk <= N) & (own[kc] == pa)
        Y = np.where(ok, X[kc] * np.exp(2j * np.pi * newth[pa]), 0)
    st.theta = newth[own]
    Y[0] = Y[0].real
    Y[-1] = Y[-1].real
    return Y


def _flags(reset, nF, mutant):
    fl = np.asarray(reset).reshape(-1) != 0
    assert fl.shape == (nF,), (fl.shape, nF)
    if mutant == "noreset":
        fl = np.zeros(nF, bool)
    elif mutant == "late_reset":
        fl = np.concatenate(([False], fl[:-1]))
    return fl


def stretch_locked_reset_roundtrip(x, pos, T, ratio=1.0, reset=None, F=1024, hop=256, mutant=None, perturb=None):
    """x: float [n_in], pos: int [nF], ratio: a scalar or [nF], reset: [nF] (any non-zero is set; None: no reset) -> float64 [T].
    `perturb` (eps, seed): the conditioning probe of pv_stretch_lock_reference.stretch_locked_roundtrip, same draws."""
    x = np.asarray(x, np.float64)
    assert mutant is None or mutant in STAGE_MUTANTS, mutant
    n_in = len(x)
    nF = (T - F) // hop + 1
    assert n_in >= F and len(pos) == nF, (n_in, len(pos), nF)
    q = SR.clamp_positions(pos, n_in, F)
    D = SR.advances(q, hop, F, "delta")
    fl = _flags(np.zeros(nF) if reset is None else reset, nF, mutant)
    w = window(F)
    scale = 1.0 / np.sum(w[::hop] ** 2)
    r = LR.frame_ratios(ratio, nF)
    st = LR.LockState(F // 2 + 1)
    rng = np.random.default_rng([perturb[1], 41]) if perturb is not None else None
    y = np.zeros(T)
    for f in range(nF):
        X = np.fft.rfft(x[q[f]:q[f] + F] * w)
        if perturb is not None:
            e = rng.standard_normal(len(X)) + 1j * rng.standard_normal(len(X))
            e[0], e[-1] = e[0].real, e[-1].real
            X = X + perturb[0] * np.abs(X).max() * e
        Y = reset_stage(X, r[f], int(D[f]), st, F, hop, bool(fl[f]), mutant)
        y[f * hop:f * hop + F] += np.fft.irfft(Y, F) * w
    return y * scale


def reset_stage_b(X, r, D, st, F, hop, flagged):
    """reset_stage stated a second way: radians (st.pprev and st.theta hold radians), explicit loops."""
    nb = len(X)
    N = nb - 1
    m = np.abs(X)
    p = np.angle(X)
    Y = np.zeros(nb, complex)
    peaks = []
    for k in range(nb):
        c = m[k]
        if not c > 0:
            continue
        if any(0 <= j <= N and not c > m[j] for j in (k - 1, k - 2)):
            continue
        if any(0 <= j <= N and not c >= m[j] for j in (k + 1, k + 2)):
            continue
        peaks.append(k)
    if peaks:
        own = LR._owners(peaks, nb)
        th = {}
        for P in peaks:
            if flagged:
                th[P] = 0.0
                continue
            d = p[P] / TWO_PI - st.pprev[P] / TWO_PI - (P * D) / F
            d -= np.rint(d)
            nu = P + d * F / D
            t = st.theta[P] + TWO_PI * (nu * (r * hop - D) / F)
            th[P] = t - TWO_PI * np.rint(t / TWO_PI)
        moved = [(int(np.floor(P * r + 0.5)), P) for P in peaks]
        moved = [(a, b) for a, b in moved if a <= N]
        if moved:
            back = dict(moved)
            towner = LR._owners([a for a, _ in moved], nb)
            for kk in range(nb):
                Ps = towner[kk]
                P = back[Ps]
                k = kk - (Ps - P)
                if 0 <= k <= N and own[k] == P:
                    Y[kk] = X[k] * np.exp(1j * th[P])
        st.theta = np.array([th[own[k]] for k in range(nb)])
    st.pprev = p
    Y[0] = Y[0].real
    Y[N] = Y[N].real
    return Y


def stretch_locked_reset_roundtrip_b(x, pos, T, ratio=1.0, reset=None, F=1024, hop=256):
    """The second statement: radians, the full complex transform, loops; positions, advances and flags written out."""
    x = np.asarray(x, np.float64)
    n_in = len(x)
    nF = (T - F) // hop + 1
    assert n_in >= F and len(pos) == nF
    w = window(F)
    scale = 1.0 / np.sum(w[::hop] ** 2)
    N = F // 2
    r = LR.frame_ratios(ratio, nF)
    st = LR.LockState(N + 1)
    y = np.zeros(T)
    q_prev = None
    for f in range(nF):
        q = min(max(int(pos[f]), 0), n_in - F)
        D = hop if q_prev is None else min(max(q - q_prev, 1), F)
        q_prev = q
        Xf = np.fft.fft(x[q:q + F] * w)
        flagged = reset is not None and int(reset[f]) != 0
        Yh = reset_stage_b(Xf[:N + 1], float(r[f]), D, st, F, hop, flagged)
        Y = np.concatenate((Yh, np.conj(Yh[1:N][::-1])))
        y[f * hop:f * hop + F] += np.fft.ifft(Y).real * w
    return y * scale


# ---- 5. the whole scheme on one recording -----------------------------------------------------------------------------------------------------------
def transient_stretch(x, stretch, thr, F=1024, hop=256, K=None, ratio=1.0, T=None):
    """flux -> pick -> plan -> stage: (y float64 [T], pos, reset, onsets).  T: the output's length, default the stretched input's."""
    x = np.asarray(x, np.float32)
    n_in = len(x)
    T = int(round(n_in * stretch)) if T is None else T
    nF = (T - F) // hop + 1
    flux, mass = onset_flux(x, F, hop)
    on = pick_onsets(flux, mass, thr)
    pos, reset = plan_positions(on, nF, hop, stretch, n_in, F, K)
    return stretch_locked_reset_roundtrip(x, pos, T, ratio, reset, F, hop), pos, reset, on
