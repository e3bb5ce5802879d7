"""Build-authored NumPy definition of the FORMANT-PRESERVING phase-vocoder pitch shift (vp_stft_pitch_shift_formant,
vp_pv_process_blocks_formant_device; csrc/vp_stft_formant.inc).  No reference counterpart -- PARITY UNPINNED by
nature.  Test infrastructure only.

Everything of stft_reference.stft_roundtrip with a per-frame ratio (pv_curve_cases.frame_loop: analysis, unwrap, gather into sm[kk],
sf[kk], accumulator in rounds of four, overlap-add) stays.  Between the gather and X = sm (cos sp + i sin sp), with nb = F / 2 + 1,
m = |rfft(frame w)|, r the frame's pitch ratio and phi the stream's formant ratio (both clamped to [0.5, 2], fmax first: a NaN is 0.5):

    L[k]   = 0.5 log(m[k]^2 + 1e-12)                           k = 0 .. nb - 1
    c      = irfft(L, F)                                       (real, even, length F)
    c[n]  *= lw[n],  lw[0 .. nc - 1] = 1, lw[nc] = 0.5, lw[nc + 1 .. F - nc - 1] = 0, symmetric (lw[F - n] = lw[n])
    le     = rfft(c).real                                      the smoothed log envelope, nb values
    at(rho)[kk]: src = clip(kk (1 / rho), 0, nb - 1); i0 = min(floor(src), nb - 2); t = src - i0; le[i0] + t (le[i0 + 1] - le[i0])
    delta[kk] = clip(at(phi)[kk] - at(r)[kk], -ln 16, +ln 16)
    sm[kk] *= exp(delta[kk])

phi = 1 leaves the envelope where it was (formant preservation), phi = 2^(st / 12) moves it by st semitones, phi = r moves it with the
pitch: delta is exactly 0 and the output is frame_loop's, bit for bit.  Bins 0 and F / 2 take the gain like every other bin and then keep
their real parts.  Two forms, as every phase-vocoder case module has them: phases in radians (pv_stream_reference.PvStreamRef._frame's
arithmetic) and in turns (pv_cases._turns_frame's).
"""
import numpy as np

import pv_cases
import pv_stream_reference as P
import stft_reference as R

LN16 = float(np.log(16.0))
FLOOR = 1e-12
LIFTER_DEFAULT = 32


def clamp_ratio(r):
    """pv_curve_clamp: fmin(fmax(r, 0.5), 2.0) -- a NaN becomes 0.5."""
    r = np.asarray(r, np.float64)
    return np.fmin(np.fmax(r, 0.5), 2.0)


def lifter_window(F, nc, half=True):
    lw = np.zeros(F)
    lw[:nc] = 1.0
    lw[nc] = 0.5 if half else 1.0
    lw[F - nc:] = 1.0                                            # lw[F - n] = lw[n], n = 1 .. nc - 1
    lw[F - nc] = lw[nc]
    return lw


def envelope(m, F, nc, half=True):
    """The smoothed log envelope of the magnitudes m [nb], by two transforms."""
    L = 0.5 * np.log(m * m + FLOOR)
    c = np.fft.irfft(L, F) * lifter_window(F, nc, half)
    return np.fft.rfft(c).real


def envelope_direct(m, F, nc):
    """The same envelope with the second step as a direct cosine sum over the nc + 1 cepstral terms."""
    L = 0.5 * np.log(m * m + FLOOR)
    c = np.fft.irfft(L, F)
    k = np.arange(F // 2 + 1)
    le = np.full(F // 2 + 1, c[0])
    for n in range(1, nc + 1):
        le = le + (2.0 if n < nc else 1.0) * c[n] * np.cos(2.0 * np.pi * n * k / F)
    return le


def envelope_at(le, rho):
    nb = len(le)
    src = np.clip(np.arange(nb) * (1.0 / rho), 0.0, nb - 1.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), nb - 2)
    t = src - i0
    return le[i0] + t * (le[i0 + 1] - le[i0])


def log_gain(m, F, ratio, phi, nc, half=True):
    """(delta [nb], number of bins at the clamp)."""
    le = envelope(m, F, nc, half)
    raw = envelope_at(le, phi) - envelope_at(le, ratio)
    return np.clip(raw, -LN16, LN16), int(np.count_nonzero(np.abs(raw) >= LN16))


class FormantRef(P.PvStreamRef):
    """PvStreamRef with the formant correction in _frame (phases in radians).  phi, nc: the stream's; the pitch ratio is the frame's.
    phi = "pitch": the formant ratio of every frame is that frame's pitch ratio (the plain pitch shift)."""

    def __init__(self, N, hop=256, F=1024, ratio=1.0, phi=1.0, nc=LIFTER_DEFAULT, half=True):
        super().__init__(N, hop, F, ratio)
        self.phi, self.nc, self.half = (None if isinstance(phi, str) else float(clamp_ratio(phi))), int(nc), half
        assert self.phi is not None or phi == "pitch", phi
        self.clamped = 0                                         # (frame, bin) pairs at the +-ln 16 clamp
        self.pairs = 0

    def _gain(self, m, ratio):
        d, n = log_gain(m, self.F, ratio, ratio if self.phi is None else self.phi, self.nc, self.half)
        self.clamped += n
        self.pairs += len(m)
        return np.exp(d)

    def _frame(self, seg, f, ratio):
        ratio = float(clamp_ratio(ratio))
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
        sm = sm * self._gain(m, ratio)                           # the formant correction
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


class FormantTurns(FormantRef):
    """The second form: pv_cases._turns_frame's arithmetic.  The gain multiplies the synthesis spectrum that function returns -- the same
    product sm exp(delta) (cos + i sin), with the real factor applied last."""

    def _frame(self, seg, f, ratio):
        ratio = float(clamp_ratio(ratio))
        X = np.fft.rfft(seg * self.w)
        Y, self.p_prev, self.sp, self.carry = pv_cases._turns_frame(X, f, ratio, self.F // self.hop, self.p_prev, self.sp, self.carry)
        Y = Y * self._gain(np.abs(X), ratio)
        return np.fft.irfft(Y, self.F) * self.w


def frame_loop(x, F, hop, ratio, phi=1.0, nc=LIFTER_DEFAULT, form="radians", half=True, stats=None):
    """One stream, one-shot: x float [T], ratio [nFrames] -> float64 [T] (pv_curve_cases.frame_loop with the correction).
    stats: a dict that receives the clamp counts."""
    cls = FormantRef if form == "radians" else FormantTurns
    r = cls(F, hop, F, phi=phi, nc=nc, half=half)               # (the block size plays no part in _frame)
    x = np.asarray(x, np.float64)
    nF = (len(x) - F) // hop + 1
    assert len(ratio) == nF
    y = np.zeros(len(x))
    for f in range(nF):
        y[f * hop:f * hop + F] += r._frame(x[f * hop:f * hop + F], f, float(ratio[f]))
    if stats is not None:
        stats["clamped"] = stats.get("clamped", 0) + r.clamped
        stats["pairs"] = stats.get("pairs", 0) + r.pairs
    return y * r.scale


def by_block(x, N, hop, ratio, phi=1.0, nc=LIFTER_DEFAULT, form="radians", stats=None):
    """One stream through a fresh streaming reference, block b with ratio[b]: float64 [N len(ratio)] with the stream's latency.
    stats: a dict that receives the clamp counts."""
    cls = FormantRef if form == "radians" else FormantTurns
    r = cls(N, hop, phi=phi, nc=nc)
    y = np.concatenate([r.process(x[b * N:(b + 1) * N], float(ratio[b])) for b in range(len(ratio))])
    if stats is not None:
        stats["clamped"] = stats.get("clamped", 0) + r.clamped
        stats["pairs"] = stats.get("pairs", 0) + r.pairs
    return y
