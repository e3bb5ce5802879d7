"""Build-authored NumPy definition of the PEAK-LOCKED phase-vocoder TIME STRETCH (vp_stft_time_stretch_locked; kernel
vp_k_stft_pv_stretch_lock of csrc/vp_stft_stretch_lock.inc).  No reference counterpart -- parity unpinned by nature.
Test infrastructure only.

Framing, positions and advances are tests/pv_stretch_reference.py's: the output row has T samples, nF = (T - F) // hop + 1 frames are
written and samples no frame covers stay 0; the input x has n_in >= F samples; pos is an integer table [nF];
  q_f = clamp(pos[f], 0, n_in - F);  D_0 = hop, D_f = clamp(q_f - q_(f-1), 1, F) for f >= 1;
frame f is x[q_f : q_f + F] and is overlap-added at output sample f hop; the window and the 1 / sum w^2 scale are unchanged.

The stage is tests/pv_lock_reference.py's lock_stage, rules 1 - 8, with two changes (phases in TURNS):
  1. unwrap    d = p - pprev - (k D_f) / F, d -= rint(d);  nu = k + d (F / D_f).  The nominal term is the exact integer product over a
               power of two, as in the stretch definition; pprev = p on every frame, silent ones included.
  4. rotation  per peak P: t = theta[P] + nu[P] ((r hop - D_f) / F), th[P] = t - rint(t).  The analysis phase of a partial advances
               nu D / F turns from frame to frame, the synthesis must advance r nu hop / F: the region's rotation grows by the difference.
               At D_f = hop this is nu (r - 1) / O; evaluated as nu * ((r * hop - D) * (1.0 / F)) it gives lock_stage's bits (r hop and
               hop (r - 1) are exact: hop and F are powers of two, r - 1 is exact on [0.5, 2]).
Peaks, ownership, the shift P' = floor(P r + 0.5), the gather, the propagation of theta, silent frames and the real bins 0 and N are
lock_stage's.  r is per frame, clamped to [0.5, 2] with NaN -> 0.5 (pv_lock_reference.clamp_ratio).

Two statements, as for every phase-vocoder reference here: stretch_locked_roundtrip (turns, rfft, vectorised) and
stretch_locked_roundtrip_b (phases and angles kept in radians, the full complex fft, explicit loops for peaks, ownership and the gather).
BOTH take the unwrap's nominal term as the exact (k D) / F and wrap in turns.  Bin N is real: its phase is exactly 0 or half a turn on
both sides, and with an odd D the value (N D) / F is a half-integer, so d sits exactly on +-1/2 without any sign flip; the tie falls by
rint's rule (half to even) in both forms and in the kernel -- a rule, not a rounding error.

`mutant` names a deliberately wrong variant of the first form (the tests' teeth):
  hop     the unwrap takes hop instead of D_f (nominal term k / O, frequency k + d O); the rotation keeps D_f
  nod     the rotation is left at nu (r - 1) / O: the D term forgotten
  late    the ratio table one frame late
  nohigh  D_f = max(q_f - q_(f-1), 1): no upper clamp at F
and the EDGE_MUTANTS, which only frames without a peak, the exact tie of the unwrap and a peak shifted onto bin N can tell from the
definition (tests/pv_stretch_lock_edge_cases.py names the case that sees each):
  silent_theta      a frame without peaks zeroes theta          silent_prev  a frame without peaks leaves pprev
  tie_away          the unwrap rounds a half away from zero (C's round) instead of to even (rint)
  drop_n            a peak with P' == N is dropped
  hop_after_silent  the frame behind a frame without peaks takes hop as its advance

`trace` collects the stage's intermediates per frame: pv_lock_reference.lock_stage's keys (P, own, Ps, Pa, owns, r, silent, gone, tie)
and the frame's q and D; `tie` holds the peaks whose unwrap d sat exactly on +-1/2 (every bin, not only 0 and N).  With trace=None nothing
changes (tests/test_pv_stretch_lock_edges_cpu.py asserts the bits on the 384 gate cases).
"""
import numpy as np

import pv_lock_reference as LR
import pv_stretch_reference as SR
from stft_reference import TWO_PI, window

MUTANTS = ("hop", "nod", "late", "nohigh")
EDGE_MUTANTS = ("silent_theta", "silent_prev", "tie_away", "drop_n", "hop_after_silent")


def stretch_lock_stage(X, r, D, st, F, hop, mutant=None, trace=None):
    """One frame of the stage: X complex [nb], r the clamped ratio, D the frame's analysis advance; st (LR.LockState) is updated;
    returns Y.  `trace`: a list that receives one dict per frame (the module's note; the caller adds q)."""
    nb = len(X)
    N = nb - 1
    O = F // hop
    k = np.arange(nb)
    m = np.abs(X)
    p = np.arctan2(X.imag, X.real) / TWO_PI
    Du = hop if mutant == "hop" else D
    d = p - st.pprev - (k * Du) / F
    d -= np.sign(d) * np.floor(np.abs(d) + 0.5) if mutant == "tie_away" else np.rint(d)
    nu = k + d * (F / Du)
    mp = np.concatenate(([-1.0, -1.0], m, [-1.0, -1.0]))
    c = mp[2:-2]
    pk = (c > 0) & (c > mp[1:-3]) & (c > mp[0:-4]) & (c >= mp[3:-1]) & (c >= mp[4:])
    P = np.nonzero(pk)[0]
    if not (mutant == "silent_prev" and len(P) == 0):
        st.pprev = p
    Y = np.zeros(nb, complex)
    if len(P) == 0:
        if mutant == "silent_theta":
            st.theta = np.zeros(nb)
        if trace is not None:
            e = np.zeros(0, np.int64)
            trace.append(dict(P=e, own=None, Ps=e, Pa=e, owns=None, r=float(r), silent=True, gone=False, tie=(), D=int(D)))
        return Y
    own = LR.nearest(P, nb)
    if mutant == "nod":
        t = st.theta[P] + nu[P] * (r - 1.0) / O
    else:
        t = st.theta[P] + nu[P] * ((r * hop - D) * (1.0 / F))
    newth = np.zeros(nb)
    newth[P] = t - np.rint(t)
    Pp = np.floor(P * r + 0.5).astype(np.int64)
    keep = (Pp < N) if mutant == "drop_n" else (Pp <= N)
    Ps, Pa = Pp[keep], P[keep]
    owns = None
    if len(Ps):
        src = np.zeros(nb, np.int64)
        src[Ps] = Pa
        owns = LR.nearest(Ps, nb)
        pa = src[owns]
        kk = k - (owns - pa)
        kc = np.clip(kk, 0, N)
        ok = (kk >= 0) & (kk <= N) & (own[kc] == pa)
        Y = np.where(ok, X[kc] * np.exp(2j * np.pi * newth[pa]), 0)
    if trace is not None:
        trace.append(dict(P=P, own=own, Ps=Ps, Pa=Pa, owns=owns, r=float(r), silent=False, gone=len(Ps) == 0,
                          tie=tuple(int(e) for e in P if abs(d[e]) == 0.5), D=int(D)))
    st.theta = newth[own]
    Y[0] = Y[0].real
    Y[-1] = Y[-1].real
    return Y


def _frames(x, pos, T, F, hop, mutant=None):
    n_in = len(x)
    nF = (T - F) // hop + 1
    assert n_in >= F and len(pos) == nF, (n_in, len(pos), nF)
    q = SR.clamp_positions(pos, n_in, F)
    return nF, q, SR.advances(q, hop, F, "nohigh" if mutant == "nohigh" else "delta")


def stretch_locked_roundtrip(x, pos, T, ratio=1.0, F=1024, hop=256, mutant=None, perturb=None, trace=None):
    """x: float [n_in], pos: int [nF], ratio: a scalar or [nF] -> float64 [T].  `perturb` (eps, seed): the conditioning probe of
    pv_lock_reference.locked_roundtrip -- every frame's spectrum is moved by eps times its largest magnitude before the stage.
    `trace`: stretch_lock_stage's, with every frame's q."""
    x = np.asarray(x, np.float64)
    assert mutant is None or mutant in MUTANTS + EDGE_MUTANTS, mutant
    nF, q, D = _frames(x, pos, T, F, hop, mutant)
    w = window(F)
    scale = 1.0 / np.sum(w[::hop] ** 2)
    r = LR.frame_ratios(ratio, nF)
    if mutant == "late":
        r = np.roll(r, 1)
    st = LR.LockState(F // 2 + 1)
    rng = np.random.default_rng([perturb[1], 41]) if perturb is not None else None
    y = np.zeros(T)
    behind_silent = False
    for f in range(nF):
        X = np.fft.rfft(x[q[f]:q[f] + F] * w)
        if perturb is not None:
            e = rng.standard_normal(len(X)) + 1j * rng.standard_normal(len(X))
            e[0], e[-1] = e[0].real, e[-1].real                   # (bins 0 and N of a real frame are real by construction)
            X = X + perturb[0] * np.abs(X).max() * e
        Df = hop if mutant == "hop_after_silent" and behind_silent else int(D[f])
        Y = stretch_lock_stage(X, r[f], Df, st, F, hop, mutant, trace)
        if trace is not None:
            trace[-1]["q"] = int(q[f])
        behind_silent = not np.any(X)                             # (a spectrum with a non-zero bin has a peak: its largest, leftmost)
        y[f * hop:f * hop + F] += np.fft.irfft(Y, F) * w
    return y * scale


def stretch_lock_stage_b(X, r, D, st, F, hop):
    """stretch_lock_stage stated a second way: radians (st.pprev and st.theta hold radians), explicit loops."""
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
            d = p[P] / TWO_PI - st.pprev[P] / TWO_PI - (P * D) / F   # (the unwrap in turns, the nominal term the exact quotient)
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


def stretch_locked_roundtrip_b(x, pos, T, ratio=1.0, F=1024, hop=256):
    """The second statement: radians, the full complex transform, loops; positions and advances written out."""
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
        Yh = stretch_lock_stage_b(Xf[:N + 1], float(r[f]), D, st, F, hop)
        Y = np.concatenate((Yh, np.conj(Yh[1:N][::-1])))
        y[f * hop:f * hop + F] += np.fft.ifft(Y).real * w
    return y * scale


def plain_stretch(x, pos, T, ratio=1.0, F=1024, hop=256):
    """The plain time stretch with a pitch ratio on top (pv_stretch_reference, turns form): what the locked one is compared with."""
    return SR.stretch_roundtrip(x, pos, T, F, hop, ratio, "turns")
