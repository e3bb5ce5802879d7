"""Build-authored NumPy definition of the peak-locked phase-vocoder pitch shift with SUB-BIN region offsets
(vp_stft_pitch_shift_locked_subbin, vp_pv_process_blocks_locked_subbin_device; csrc/vp_stft_lockf.inc).  No reference counterpart --
PARITY UNPINNED by nature, like its parent tests/pv_lock_reference.py.  Test infrastructure only.

Framing, the clamp of r and steps 1 - 5, 7 and 8 are the parent's, statement for statement (peaks, ownership, th[P],
P' = floor(P r + 0.5), peaks with P' > N dropped, the propagation of theta, silent frames).  The parent moves a peak's region by the
INTEGER P' - P while its angle advances at the true frequency nu (r - 1) / O: the lobe then sits up to half a bin, plus the peak's own
sub-bin position, from the frequency its phase turns at, and successive frames do not add up in the overlap-add (a 0.5 tone leaves at
0.38).  Here (Laroche & Dolson's remedy) the region is translated by a real-valued offset and the spectrum interpolated.  With m = |X|:

  5b. centre    per kept peak P: delta = 0 if P is 0 or N, else delta = (m[P-1] - m[P+1]) / 2 (m[P-1] - 2 m[P] + m[P+1]) (the vertex of
                the parabola through the three LINEAR magnitudes: continuous when a neighbour tends to 0, no phase history; the peak rule
                makes the denominator negative and puts delta in [-1/2, 1/2]; the value is clamped there, which only rounding can make
                bite); c = P + delta, D = c (r - 1)
  6'. synthesis bin kk belongs to the nearest P' (the lower on equal distance), its peak is P.  u = kk - D, u0 = floor(u), f = u - u0.
                f == 0: one tap k = u0 of weight 1.  Otherwise six taps k_j = u0 + j, j = -2 .. 3, x_j = f - j,
                w_j = sinc(x_j) (1/2 + 1/2 cos(pi x_j / 3)), sinc(x) = sin(pi x) / (pi x).  A tap counts only if 0 <= k_j <= N and
                own[k_j] == P (no mirroring).  Y[kk] = exp(2 pi i th[P]) sum_j w_j (-1)^(kk - k_j) X[k_j]; bins 0 and N keep their real
                parts.

The alternating sign belongs to the definition, in the single-tap case too: a frame starts at the window's first sample, so the spectrum
of a windowed sinusoid changes sign from bin to bin, and interpolating without the factor cancels the lobe.  At r = 1, D is exactly 0
and the stage is the identity.  The statement is continuous in u (a tap enters or leaves at |x| = 3 with weight 0): the discrete
decisions are the parent's -- peaks, owners, P', the unwrap's rint.

lockf_roundtrip is that statement (turns, rfft, vectorised over the bins); lockf_roundtrip_b states it a second way -- radians, the full
complex fft, loops over bins and taps, the weights from math.sin and math.cos one tap at a time -- as the check of the first.  `mutant`
names a deliberately wrong variant of the NEW steps of the first form (the tests' teeth): nosign, nopar, notaper, leak, round, four,
mirror.  `trace` and `perturb` are the parent's (the trace's dicts also carry delta and D per peak).
"""
import math

import numpy as np

import pv_lock_reference as L
import pv_stream_reference as P
from stft_reference import TWO_PI, window

# nosign  the (-1)^(kk - k_j) factor dropped            nopar   delta = 0 (the peak's bin is its centre)
# notaper sinc truncated to six taps, no Hann taper      leak    taps ignore ownership
# round   D rounded to an integer                        four    taps -1 .. 2 only
# mirror  taps outside 0 .. N reflected, not dropped
MUTANTS = ("nosign", "nopar", "notaper", "leak", "round", "four", "mirror")

clamp_ratio, nearest, frame_ratios, LockState, gpu_bound = L.clamp_ratio, L.nearest, L.frame_ratios, L.LockState, L.gpu_bound


def centre_offset(m, P):
    """delta of step 5b for the peaks P (int array) of the magnitudes m."""
    N = len(m) - 1
    mp = np.concatenate(([0.0], m, [0.0]))
    a, c, b = mp[P], mp[P + 1], mp[P + 2]
    inner = (P > 0) & (P < N)
    den = np.where(inner, a - 2.0 * c + b, -1.0)
    return np.where(inner, np.fmin(np.fmax(0.5 * (a - b) / den, -0.5), 0.5), 0.0)


def tap_weight(x, taper=True):
    w = np.sinc(x)
    return w * (0.5 + 0.5 * np.cos(np.pi * x / 3.0)) if taper else w


def lockf_stage(X, r, st, O, mutant=None, trace=None):
    """One frame of the stage: X complex [nb], r the clamped ratio; st (a LockState) is updated; returns Y."""
    nb = len(X)
    N = nb - 1
    k = np.arange(nb)
    m = np.abs(X)
    p = np.arctan2(X.imag, X.real) / TWO_PI
    d = p - st.pprev - k / O
    d -= np.rint(d)
    nu = k + d * O
    mp = np.concatenate(([-1.0, -1.0], m, [-1.0, -1.0]))
    c = mp[2:-2]
    pk = (c > 0) & (c > mp[1:-3]) & (c > mp[0:-4]) & (c >= mp[3:-1]) & (c >= mp[4:])
    Pk = np.nonzero(pk)[0]
    st.pprev = p
    Y = np.zeros(nb, complex)
    if len(Pk) == 0:
        if trace is not None:
            e = np.zeros(0, np.int64)
            trace.append(dict(P=e, own=None, Ps=e, Pa=e, owns=None, r=float(r), silent=True, gone=False, tie=(), delta=np.zeros(0), D=np.zeros(0)))
        return Y
    own = nearest(Pk, nb)
    t = st.theta[Pk] + nu[Pk] * (r - 1.0) / O
    newth = np.zeros(nb)
    newth[Pk] = t - np.rint(t)
    Pp = np.floor(Pk * r + 0.5).astype(np.int64)
    keep = Pp <= N
    Ps, Pa = Pp[keep], Pk[keep]
    # 5b
    delta = np.zeros(len(Pk)) if mutant == "nopar" else centre_offset(m, Pk)
    D = (Pk + delta) * (r - 1.0)
    if mutant == "round":
        D = np.rint(D)
    owns = None
    if len(Ps):
        # 6'
        src = np.zeros(nb, np.int64)
        src[Ps] = Pa
        Dof = np.zeros(nb)
        Dof[Pk] = D
        owns = nearest(Ps, nb)
        pa = src[owns]
        u = k - Dof[pa]
        u0f = np.floor(u)
        f = u - u0f
        u0 = u0f.astype(np.int64)
        one = f == 0.0
        acc = np.zeros(nb, complex)
        for j in (range(-1, 3) if mutant == "four" else range(-2, 4)):
            kj = u0 + j
            w = np.where(one, 1.0 if j == 0 else 0.0, tap_weight(f - j, mutant != "notaper"))
            if mutant == "mirror":
                kj = np.where(kj < 0, -kj, np.where(kj > N, 2 * N - kj, kj))
            ok = (kj >= 0) & (kj <= N)
            kc = np.clip(kj, 0, N)
            if mutant != "leak":
                ok &= own[kc] == pa
            sign = 1.0 if mutant == "nosign" else 1.0 - 2.0 * ((k - kj) & 1)
            acc += np.where(ok, w * sign * X[kc], 0.0)
        Y = acc * np.exp(2j * np.pi * newth[pa])
    if trace is not None:
        ends = [e for e in (0, N) if pk[e]]
        trace.append(dict(P=Pk, own=own, Ps=Ps, Pa=Pa, owns=owns, r=float(r), silent=False, gone=len(Ps) == 0,
                          tie=tuple(e for e in ends if abs(d[e]) == 0.5), delta=delta, D=D))
    st.theta = newth[own]
    Y[0] = Y[0].real
    Y[-1] = Y[-1].real
    return Y


def lockf_roundtrip(x, ratio, F=1024, hop=256, mutant=None, trace=None, perturb=None):
    """x: float array [T]; ratio: scalar or [nFrames] -> float64 [T].  `perturb` (eps, seed): the parent's conditioning probe -- every
    frame's spectrum is moved by eps times its largest magnitude (seeded complex noise; real at bins 0 and N) before the stage."""
    x = np.asarray(x, np.float64)
    T = len(x)
    w = window(F)
    scale = 1.0 / np.sum(w[::hop] ** 2)
    nF = (T - F) // hop + 1
    O = F // hop
    r = frame_ratios(ratio, nF)
    st = LockState(F // 2 + 1)
    rng = np.random.default_rng([perturb[1], 41]) if perturb is not None else None
    y = np.zeros(T)
    for f in range(nF):
        X = np.fft.rfft(x[f * hop:f * hop + F] * w)
        if perturb is not None:
            e = rng.standard_normal(len(X)) + 1j * rng.standard_normal(len(X))
            e[0], e[-1] = e[0].real, e[-1].real
            X = X + perturb[0] * np.abs(X).max() * e
        Y = lockf_stage(X, r[f], st, O, mutant, trace)
        y[f * hop:f * hop + F] += np.fft.irfft(Y, F) * w
    return y * scale


def lockf_stage_b(X, r, st, O):
    """lockf_stage stated a second way: radians (st.pprev and st.theta hold radians), explicit loops over peaks, bins and taps."""
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
        own = L._owners(peaks, nb)
        th, off = {}, {}
        for Pk in peaks:
            d = p[Pk] / TWO_PI - st.pprev[Pk] / TWO_PI - Pk / O
            d -= np.rint(d)
            nu = Pk + d * O
            t = st.theta[Pk] + TWO_PI * (nu * (r - 1.0)) / O
            th[Pk] = t - TWO_PI * np.rint(t / TWO_PI)
            delta = 0.0
            if 0 < Pk < N:
                lo, mid, hi = float(m[Pk - 1]), float(m[Pk]), float(m[Pk + 1])
                delta = min(max(0.5 * (lo - hi) / (lo - 2.0 * mid + hi), -0.5), 0.5)
            off[Pk] = (Pk + delta) * (r - 1.0)
        moved = [(int(np.floor(Pk * r + 0.5)), Pk) for Pk in peaks]
        moved = [(a, b) for a, b in moved if a <= N]
        if moved:
            back = dict(moved)
            towner = L._owners([a for a, _ in moved], nb)
            for kk in range(nb):
                Pk = back[towner[kk]]
                u = kk - off[Pk]
                u0 = math.floor(u)
                f = u - u0
                taps = [(u0, 1.0)] if f == 0.0 else [(u0 + j, math.sin(math.pi * (f - j)) / (math.pi * (f - j)) * (0.5 + 0.5 * math.cos(math.pi * (f - j) / 3.0)))
                                                     for j in range(-2, 4)]
                acc = 0j
                for kj, wj in taps:
                    if 0 <= kj <= N and own[kj] == Pk:
                        acc += wj * (-1) ** ((kk - kj) % 2) * X[kj]
                Y[kk] = acc * np.exp(1j * th[Pk])
        st.theta = np.array([th[own[k]] for k in range(nb)])
    st.pprev = p
    Y[0] = Y[0].real
    Y[N] = Y[N].real
    return Y


def lockf_roundtrip_b(x, ratio, F=1024, hop=256):
    """The second statement: radians, the full complex transform, loops."""
    x = np.asarray(x, np.float64)
    T = len(x)
    w = window(F)
    scale = 1.0 / np.sum(w[::hop] ** 2)
    nF = (T - F) // hop + 1
    N = F // 2
    O = F // hop
    r = frame_ratios(ratio, nF)
    st = LockState(N + 1)
    y = np.zeros(T)
    for f in range(nF):
        Xf = np.fft.fft(x[f * hop:f * hop + F] * w)
        Yh = lockf_stage_b(Xf[:N + 1], r[f], st, O)
        Y = np.concatenate((Yh, np.conj(Yh[1:N][::-1])))
        y[f * hop:f * hop + F] += np.fft.ifft(Y).real * w
    return y * scale


class LockfStreamRef(P.PvStreamRef):
    """pv_stream_reference.PvStreamRef's call bookkeeping with the sub-bin locked stage: process(x, ratio) one block at a time is
    vp_pv_process_blocks_locked_subbin_device driven block by block -- every frame of the call takes the call's ratio."""

    def __init__(self, N, hop=256, F=1024, ratio=1.0, trace=None, mutant=None):
        self.trace, self.mutant = trace, mutant
        super().__init__(N, hop, F, ratio)

    def reset(self):
        super().reset()
        self.lock = LockState(self.F // 2 + 1)

    def _frame(self, seg, f, ratio):
        Y = lockf_stage(np.fft.rfft(seg * self.w), float(clamp_ratio(ratio)), self.lock, self.F // self.hop, self.mutant, self.trace)
        return np.fft.irfft(Y, self.F) * self.w


def by_block(x, N, hop, block_ratio, trace=None):
    """x [T] (T a multiple of N) streamed block by block, block b with block_ratio[b] -> the streaming call's output [T] (float64)."""
    r = LockfStreamRef(N, hop, trace=trace)
    return np.concatenate([r.process(x[b * N:(b + 1) * N], block_ratio[b]) for b in range(len(x) // N)])
