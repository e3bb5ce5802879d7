"""Build-authored NumPy definition of the PEAK-LOCKED phase-vocoder pitch shift (vp_stft_pitch_shift_locked,
vp_pv_process_blocks_locked_device; csrc/vp_stft_lock.inc).  No reference counterpart -- PARITY UNPINNED by
nature.  Test infrastructure only.

The framing is stft_reference.stft_roundtrip's (window, scale, overlap-add, frames f = 0 .. (T - F) / hop); the stage between the two
transforms is Laroche & Dolson's (1999) identity phase locking with integer offsets.  Per stream pprev[k] = 0, theta[k] = 0; per frame,
with the ratio r clamped to [0.5, 2] (fmax first: a NaN is 0.5), phases in TURNS:

  1. analysis   X = rfft(frame w), m = |X|, p = atan2(im, re) / 2 pi; d = p - pprev - k / O, d -= rint(d); nu = k + d O; pprev = p
  2. peaks      m[k] > 0, m[k] > m[k-1], m[k-2], m[k] >= m[k+1], m[k+2] (a neighbour outside 0 .. N does not count)
  3. ownership  own[k] = the nearest peak, the lower one on equal distance
  4. rotation   per peak P: t = theta[P] + (nu[P] (r - 1)) / O, th[P] = t - rint(t)
  5. shift      P' = floor(P r + 0.5); a peak with P' > N takes no part in the synthesis (its th is kept)
  6. synthesis  bin kk belongs to the nearest P' (the lower on equal distance); its source is k = kk - (P' - P); if 0 <= k <= N and
                own[k] == P then Y[kk] = X[k] exp(2 pi i th[P]), else 0; bins 0 and N keep their real parts
  7. propagate  theta[k] = th[own[k]] for every k
  8. a frame without peaks (all zeros) gives Y = 0 and leaves theta

locked_roundtrip is that statement (turns, rfft).  locked_roundtrip_b states the same stage a second way -- phases and angles kept in
radians, the full complex fft, explicit loops for peaks, ownership and the gather -- as the check of the first.  `mutant` names a
deliberately wrong variant of the first form (the tests' teeth): noprop, tieup, ratio, floor, noown, late, strict, and the EDGE_MUTANTS
that only frames without a peak, frames that lose every peak past N and sparse masks can tell from the definition.  `trace` collects the
stage's intermediates per frame (lock_stage); with trace=None nothing changes (tests/test_pv_lock_edges_cpu.py asserts the bits).

The unwrap of the second form divides its radians by 2 pi and wraps in turns, like the first.  Bins 0 and N of a real frame are real:
their phases are exactly 0 or half a turn (pi / 2 pi is exactly 0.5 in binary), so when such a bin is a peak and changes sign between two
frames, d = +-1/2 - k / O sits EXACTLY on the wrap, and rint (half to even, k / O an integer there) resolves it by the sign of
p - pprev -- a rule, not a rounding error; the kernels compute the same exact values (rfft_split leaves the two bins' imaginary parts
+0).  Wrapped in radians the same tie sits on the rounding error of pi - 2 pi k / O and falls either way: with the unwrap in radians 11
of the 96 gate cases (all at hop 512 and r < 1, where the choice turns the region of bin N by r - 1 turns) differed by up to 0.08.
"""
import numpy as np

import pv_stream_reference as P
from stft_reference import TWO_PI, window

MUTANTS = ("noprop", "tieup", "ratio", "floor", "noown", "late", "strict")
# wrong variants at the EDGES of the stage (tests/pv_lock_edge_cases.py names the case that sees each):
#   silent_theta  a frame without peaks zeroes theta            silent_prev  a frame without peaks leaves pprev
#   gone_theta    a frame whose peaks all leave past N does not advance theta
#   drop_n        a peak with P' == N is dropped                top_lost     a peak at bin N is not a peak
#   no_lower      bins below the lowest peak (below the lowest shifted peak) have no owner: zero output, theta 0
#   near_only     a bin more than 64 bins from both of its neighbours takes the upper one
EDGE_MUTANTS = ("silent_theta", "silent_prev", "gone_theta", "drop_n", "no_lower", "near_only", "top_lost")


def clamp_ratio(r):
    r = np.asarray(r, np.float64)
    return np.fmin(np.fmax(np.where(np.isnan(r), 0.5, r), 0.5), 2.0)


def nearest(idx, n, tie_up=False, near_only=False):
    """Owner of each of n bins among the sorted, non-empty idx; ties to the lower (tie_up: to the upper; near_only: the edge mutant)."""
    idx = np.asarray(idx, np.int64)
    k = np.arange(n)
    j = np.searchsorted(idx, k, side="right") - 1                 # last idx <= k, or -1
    lo = idx[np.clip(j, 0, len(idx) - 1)]
    hi = idx[np.clip(j + 1, 0, len(idx) - 1)]
    dlo = np.where(j >= 0, k - lo, n + 1)
    dhi = np.where(j + 1 < len(idx), hi - k, n + 1)
    up = (dhi < dlo) if not tie_up else (dhi <= dlo)
    if near_only:
        up = up | ((dlo > 64) & (dhi > 64) & (j >= 0) & (j + 1 < len(idx)))
    return np.where(up, hi, lo)


def frame_ratios(ratio, nF):
    """A scalar or a per-frame curve -> float64 [nF], clamped."""
    r = np.asarray(ratio, np.float64)
    if r.ndim == 0:
        r = np.full(nF, float(r))
    assert r.shape == (nF,), (r.shape, nF)
    return clamp_ratio(r)


class LockState:
    """pprev and theta of one stream."""

    def __init__(self, nb=513):
        self.pprev = np.zeros(nb)
        self.theta = np.zeros(nb)


def lock_stage(X, r, st, O, mutant=None, trace=None):
    """One frame of the stage: X complex [nb], r the clamped ratio; st is updated; returns Y.  `trace`: a list that receives one dict of
    the definition's intermediates per frame (P, own, Ps, Pa, owns: int arrays, owns None where no shifted peak is left; r; silent: no
    peak; gone: peaks, all shifted past N; tie: the peaks among bins 0 and N whose unwrap sat exactly on the half turn, a tuple)."""
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
    if mutant == "strict":
        pk = (c > 0) & (c > mp[1:-3]) & (c > mp[0:-4]) & (c > mp[3:-1]) & (c > mp[4:])
    else:
        pk = (c > 0) & (c > mp[1:-3]) & (c > mp[0:-4]) & (c >= mp[3:-1]) & (c >= mp[4:])
    if mutant == "top_lost":
        pk[N] = False
    P = np.nonzero(pk)[0]
    if not (mutant == "silent_prev" and len(P) == 0):
        st.pprev = p
    Y = np.zeros(nb, complex)
    if len(P) == 0:
        if mutant == "silent_theta":
            st.theta = np.zeros(nb)
        if trace is not None:
            e = np.zeros(0, np.int64)
            trace.append(dict(P=e, own=None, Ps=e, Pa=e, owns=None, r=float(r), silent=True, gone=False, tie=()))
        return Y
    tie = mutant == "tieup"
    near = mutant == "near_only"
    own = nearest(P, nb, tie, near)
    t = st.theta[P] + nu[P] * ((r if mutant == "ratio" else r - 1.0)) / O
    newth = np.zeros(nb)
    newth[P] = t - np.rint(t)
    Pp = np.floor(P * r + (0.0 if mutant == "floor" else 0.5)).astype(np.int64)
    keep = (Pp < N) if mutant == "drop_n" else (Pp <= N)
    Ps, Pa = Pp[keep], P[keep]
    if mutant == "floor" and len(Ps):                             # (floor(P r) need not be distinct: the last one stays)
        Ps, first = np.unique(Ps[::-1], return_index=True)
        Pa = Pa[::-1][first]
    owns = None
    if len(Ps):
        src = np.zeros(nb, np.int64)
        src[Ps] = Pa
        owns = nearest(Ps, nb, tie, near)
        pa = src[owns]
        kk = k - (owns - pa)
        kc = np.clip(kk, 0, N)
        ok = (kk >= 0) & (kk <= N)
        if mutant != "noown":
            ok &= own[kc] == pa
        if mutant == "no_lower":
            ok &= (k >= Ps[0]) & (kk >= P[0])
        Y = np.where(ok, X[kc] * np.exp(2j * np.pi * newth[pa]), 0)
    if trace is not None:
        ends = [e for e in (0, N) if pk[e]]
        trace.append(dict(P=P, own=own, Ps=Ps, Pa=Pa, owns=owns, r=float(r), silent=False, gone=len(Ps) == 0,
                          tie=tuple(e for e in ends if abs(d[e]) == 0.5)))
    if mutant == "gone_theta" and len(Ps) == 0:
        pass
    elif mutant == "noprop":
        st.theta = st.theta.copy()
        st.theta[P] = newth[P]
    else:
        st.theta = newth[own]
        if mutant == "no_lower":
            st.theta = np.where(k >= P[0], st.theta, 0.0)
    Y[0] = Y[0].real
    Y[-1] = Y[-1].real
    return Y


def locked_roundtrip(x, ratio, F=1024, hop=256, mutant=None, trace=None, perturb=None):
    """x: float array [T]; ratio: scalar or [nFrames] -> float64 [T].  `trace`: lock_stage's.  `perturb` (eps, seed): the conditioning
    probe -- every frame's spectrum is moved by eps times its largest magnitude (seeded complex noise; real at bins 0 and N) before the
    stage."""
    x = np.asarray(x, np.float64)
    T = len(x)
    w = window(F)
    scale = 1.0 / np.sum(w[::hop] ** 2)
    nF = (T - F) // hop + 1
    O = F // hop
    r = frame_ratios(ratio, nF)
    if mutant == "late":
        r = np.roll(r, 1)
    st = LockState(F // 2 + 1)
    rng = np.random.default_rng([perturb[1], 41]) if perturb is not None else None
    y = np.zeros(T)
    for f in range(nF):
        X = np.fft.rfft(x[f * hop:f * hop + F] * w)
        if perturb is not None:
            e = rng.standard_normal(len(X)) + 1j * rng.standard_normal(len(X))
            e[0], e[-1] = e[0].real, e[-1].real                   # (bins 0 and N of a real frame are real by construction)
            X = X + perturb[0] * np.abs(X).max() * e
        Y = lock_stage(X, r[f], st, O, mutant, trace)
        y[f * hop:f * hop + F] += np.fft.irfft(Y, F) * w
    return y * scale


def _owners(idx, nb):
    """Two sweeps: the last of idx at or below each bin, the first above it; the nearer one, the lower on a tie."""
    marked = set(idx)
    below, above, last = [None] * nb, [None] * nb, None
    for kk in range(nb):
        if kk in marked:
            last = kk
        below[kk] = last
    last = None
    for kk in range(nb - 1, -1, -1):
        above[kk] = last
        if kk in marked:
            last = kk
    out = []
    for kk in range(nb):
        lo, hi = below[kk], above[kk]
        out.append(hi if lo is None else lo if hi is None or kk - lo <= hi - kk else hi)
    return out


def lock_stage_b(X, r, st, O):
    """lock_stage stated a second way: radians (st.pprev and st.theta hold radians), explicit loops."""
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
        own = _owners(peaks, nb)
        th = {}
        for P in peaks:
            d = p[P] / TWO_PI - st.pprev[P] / TWO_PI - P / O          # (the unwrap in turns: see the module's note on real bins)
            d -= np.rint(d)
            nu = P + d * O
            t = st.theta[P] + TWO_PI * (nu * (r - 1.0)) / O
            th[P] = t - TWO_PI * np.rint(t / TWO_PI)
        moved = [(int(np.floor(P * r + 0.5)), P) for P in peaks]
        moved = [(a, b) for a, b in moved if a <= N]
        if moved:
            back = dict(moved)
            towner = _owners([a for a, _ in moved], nb)
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


def locked_roundtrip_b(x, ratio, F=1024, hop=256):
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
        Yh = lock_stage_b(Xf[:N + 1], r[f], st, O)
        Y = np.concatenate((Yh, np.conj(Yh[1:N][::-1])))
        y[f * hop:f * hop + F] += np.fft.ifft(Y).real * w
    return y * scale


class LockStreamRef(P.PvStreamRef):
    """pv_stream_reference.PvStreamRef's call bookkeeping (frames computed in the call in which their last sample arrives, latency
    F - gcd(N, hop), reset) with the locked stage: process(x, ratio) one block at a time is vp_pv_process_blocks_locked_device driven
    block by block -- every frame of the call takes the call's ratio."""

    def __init__(self, N, hop=256, F=1024, ratio=1.0, trace=None, mutant=None):
        self.trace, self.mutant = trace, mutant
        super().__init__(N, hop, F, ratio)

    def reset(self):
        super().reset()
        self.lock = LockState(self.F // 2 + 1)

    def _frame(self, seg, f, ratio):
        Y = lock_stage(np.fft.rfft(seg * self.w), float(clamp_ratio(ratio)), self.lock, self.F // self.hop, self.mutant, self.trace)
        return np.fft.irfft(Y, self.F) * self.w


def by_block(x, N, hop, block_ratio, trace=None):
    """x [T] (T a multiple of N) streamed block by block, block b with block_ratio[b] -> the streaming call's output [T] (float64)."""
    r = LockStreamRef(N, hop, trace=trace)
    return np.concatenate([r.process(x[b * N:(b + 1) * N], block_ratio[b]) for b in range(len(x) // N)])


def gpu_bound(ref, hop, F=1024):
    """The GPU gate: float32 output of O overlapping frames."""
    return 4.0 * (F // hop) * 2.0 ** -24 * max(1.0, float(np.max(np.abs(ref))) if len(ref) else 1.0)
