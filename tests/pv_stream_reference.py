"""NumPy restatement of the STREAMING phase vocoder (include/vp_amd.h vp_pv_*, csrc/vp_stft.hip vp_k_pv_stream): the one-shot stage
of tests/stft_reference.py (imported, not edited) driven call by call, with per-stream state.  Test infrastructure only.

Semantics restated here (one stream; a handle is S of them):
  * frame f covers samples [f hop, f hop + F) of everything the stream received since create / reset and is computed in the call in
    which its last sample arrives, with the ratio of that call -- the ratio schedule is per frame;
  * the synthesis accumulator runs in the one-shot's rounds of four frames by global frame index: sp = carry + inc at a round's first
    frame, sp + inc after it, carry = wrap(sp) at its last; a round that a call cuts simply continues in the next call;
  * latency L = F - gcd(N, hop): output sample t is one-shot sample t - L (0 before the stream's first sample).
The arithmetic is stft_reference.stft_roundtrip's, operation for operation: streamed with a constant ratio it reproduces that
function delayed by L.
"""
import math

import numpy as np

import stft_reference as R


def latency(N, hop, F=1024):
    return F - math.gcd(int(N), int(hop))


class PvStreamRef:
    def __init__(self, N, hop=256, F=1024, ratio=1.0):
        self.N, self.hop, self.F = int(N), int(hop), int(F)
        self.L = latency(N, hop, F)
        self.w = R.window(F)
        self.scale = 1.0 / np.sum(self.w[::hop] ** 2)
        self.ratio = ratio
        self.frame_ratios = []              # ratio each frame was computed with, by global frame index (since the last reset)
        self.reset()

    def reset(self):
        """Like a fresh stream (the ratio stays)."""
        nb = self.F // 2 + 1
        self.n = 0                          # samples received
        self.nf = 0                         # frames computed
        self.hist = np.zeros(0)             # samples [nf hop, n)
        self.p_prev = np.zeros(nb)
        self.carry = np.zeros(nb)           # the accumulator at the last round's end (wrapped)
        self.sp = np.zeros(nb)              # ... and within the round in progress
        self.y0 = -self.L                   # one-shot sample index of self.y[0]: the next one to emit
        self.y = np.zeros(self.L + self.F)  # overlap-add sums (float64, unscaled, as stft_roundtrip)
        self.frame_ratios = []

    def finished_before(self):
        """One-shot samples below this index are finished (every frame that covers them is in)."""
        return self.nf * self.hop

    def _frame(self, seg, f, ratio):
        F, hop = self.F, self.hop
        nb = F // 2 + 1
        k = np.arange(nb)
        O = F // hop
        expct = R.TWO_PI / O
        X = np.fft.rfft(seg * self.w)
        m, p = np.abs(X), np.arctan2(X.imag, X.real)
        d = p - self.p_prev - k * expct
        d -= R.TWO_PI * np.rint(d * (1.0 / R.TWO_PI))
        fk = k + d * (O * (1.0 / R.TWO_PI))
        self.p_prev = p
        idx = np.floor(k * ratio + 0.5).astype(np.int64)
        sm, sf = np.zeros(nb), np.zeros(nb)
        for kk in range(nb):
            t = idx[kk]
            if 0 <= t < nb:
                sm[t] += m[kk]
                sf[t] = fk[kk] * ratio
        inc = expct * sf
        if f % R.ROUND == 0:
            self.sp = self.carry + inc
        else:
            self.sp = self.sp + inc
        if f % R.ROUND == R.ROUND - 1:
            self.carry = self.sp - R.TWO_PI * np.rint(self.sp * (1.0 / R.TWO_PI))
        X = sm * (np.cos(self.sp) + 1j * np.sin(self.sp))
        X[0] = X[0].real
        X[-1] = X[-1].real
        return np.fft.irfft(X, F) * self.w

    def process(self, x, ratio=None):
        """One call: x float [M] (any number of samples; the handle's calls are whole blocks) -> output [M] (float64).  `ratio`: the
        ratio in force for this call (None: the previous one)."""
        if ratio is not None:
            self.ratio = ratio
        x = np.asarray(x, np.float64)
        M = len(x)
        F, hop = self.F, self.hop
        buf = np.concatenate([self.hist, x])           # samples [nf hop, n + M)
        base = self.nf * hop
        Rn = self.n + M
        fb = (Rn - F) // hop + 1 if Rn >= F else 0
        end = Rn - self.L                               # one-shot samples [y0, end) leave in this call
        need = max(end, (fb - 1) * hop + F if fb > 0 else 0) - self.y0
        if need > len(self.y):
            self.y = np.concatenate([self.y, np.zeros(need - len(self.y))])
        for f in range(self.nf, fb):
            seg = buf[f * hop - base:f * hop - base + F]
            o = f * hop - self.y0
            self.y[o:o + F] += self._frame(seg, f, self.ratio)
            self.frame_ratios.append(self.ratio)
        self.nf = fb
        out = self.y[:M] * self.scale
        out[:max(0, min(M, -self.y0))] = 0.0            # (before the stream's first sample: nothing was ever added there anyway)
        self.y = np.concatenate([self.y[M:], np.zeros(M)])
        self.y0 += M
        self.n = Rn
        self.hist = buf[fb * hop - base:]
        return out


def stream(x, N, hop=256, ratio=1.0, calls=None):
    """Streams the signal x [T] (T a multiple of N) through one PvStreamRef in calls of `calls` blocks each (a list, cycled; default one
    block per call) and returns the concatenated output [T] and the stream object."""
    s = PvStreamRef(N, hop, ratio=ratio)
    x = np.asarray(x, np.float64)
    T = len(x)
    assert T % N == 0
    calls = calls or [1]
    out, pos, i = [], 0, 0
    while pos < T:
        k = min(calls[i % len(calls)], (T - pos) // N)
        out.append(s.process(x[pos:pos + k * N]))
        pos += k * N
        i += 1
    return np.concatenate(out), s
