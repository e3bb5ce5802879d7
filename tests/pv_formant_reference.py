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

WRONG names what a plausible wrong kernel would compute in the envelope stage, one deviation each; every function below takes one of the
names as an optional `wrong` (None: the definition above).  tests/test_pv_formant_edges_cpu.py asserts how far each is from the definition.
"""
import numpy as np

import pv_cases
import pv_stream_reference as P
import stft_reference as R

LN16 = float(np.log(16.0))
FLOOR = 1e-12
LIFTER_DEFAULT = 32
WRONG = ("clamp-ln8",        # the clamp at +-ln 8
         "clamp-db",         # ... at +-ln 10^(24 / 20) = 2.763 (ln 16 = 2.7726 is 24.08 dB)
         "clamp-nolow",      # no lower clamp
         "clamp-nohigh",     # no upper clamp
         "top511",           # the interpolation's source position clipped at nb - 2 instead of nb - 1
         "interp-t0",        # the interpolation weight dropped: le[i0]
         "interp-nearest",   # the nearer of the two envelope values
         "floor-1e-11", "floor-1e-13",
         "floor-none",       # log(m^2) (1e-300 keeps the logarithm of an exact zero finite)
         "floor-on-m")       # log(m + 1e-6), the floor on the magnitude


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


def log_magnitude(m, wrong=None):
    if wrong == "floor-on-m":
        return np.log(m + 1e-6)
    return 0.5 * np.log(m * m + {"floor-1e-11": 1e-11, "floor-1e-13": 1e-13, "floor-none": 1e-300}.get(wrong, FLOOR))


def envelope(m, F, nc, half=True, wrong=None):
    """The smoothed log envelope of the magnitudes m [nb], by two transforms."""
    L = log_magnitude(m, wrong)
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


def envelope_at(le, rho, wrong=None):
    nb = len(le)
    src = np.clip(np.arange(nb) * (1.0 / rho), 0.0, nb - (2.0 if wrong == "top511" else 1.0))
    i0 = np.minimum(np.floor(src).astype(np.int64), nb - 2)
    t = src - i0
    if wrong == "interp-t0":
        t = 0.0 * t
    elif wrong == "interp-nearest":
        t = np.floor(t + 0.5)
    return le[i0] + t * (le[i0 + 1] - le[i0])


def raw_log_gain(m, F, ratio, phi, nc, half=True, wrong=None):
    """at(phi) - at(r) before the clamp [nb]."""
    le = envelope(m, F, nc, half, wrong)
    return envelope_at(le, phi, wrong) - envelope_at(le, ratio, wrong)


def clamp_limits(wrong=None):
    c = {"clamp-ln8": float(np.log(8.0)), "clamp-db": float(np.log(10.0 ** (24.0 / 20.0)))}.get(wrong, LN16)
    return (-np.inf if wrong == "clamp-nolow" else -c), (np.inf if wrong == "clamp-nohigh" else c)


def log_gain(m, F, ratio, phi, nc, half=True, wrong=None):
    """(delta [nb], number of bins at the clamp)."""
    raw = raw_log_gain(m, F, ratio, phi, nc, half, wrong)
    return np.clip(raw, *clamp_limits(wrong)), int(np.count_nonzero(np.abs(raw) >= LN16))


class FormantRef(P.PvStreamRef):
    """PvStreamRef with the formant correction in _frame (phases in radians).  phi, nc: the stream's; the pitch ratio is the frame's.
    phi = "pitch": the formant ratio of every frame is that frame's pitch ratio (the plain pitch shift).  set_formant switches phi and
    nc between calls (a handle's formant, curve and plain calls)."""

    def __init__(self, N, hop=256, F=1024, ratio=1.0, phi=1.0, nc=LIFTER_DEFAULT, half=True, wrong=None):
        super().__init__(N, hop, F, ratio)
        self.half, self.wrong = half, wrong
        self.set_formant(phi, nc)
        self.clamped = 0                                         # (frame, bin) pairs at the +-ln 16 clamp
        self.clamped_hi = self.clamped_lo = 0                    # ... on either side
        self.pairs = 0

    def set_formant(self, phi, nc=None):
        self.phi = None if isinstance(phi, str) else float(clamp_ratio(phi))
        assert self.phi is not None or phi == "pitch", phi
        if nc is not None:
            self.nc = int(nc)

    def _gain(self, m, ratio):
        raw = raw_log_gain(m, self.F, ratio, ratio if self.phi is None else self.phi, self.nc, self.half, self.wrong)
        self.clamped += int(np.count_nonzero(np.abs(raw) >= LN16))
        self.clamped_hi += int(np.count_nonzero(raw >= LN16))
        self.clamped_lo += int(np.count_nonzero(raw <= -LN16))
        self.pairs += len(m)
        return np.exp(np.clip(raw, *clamp_limits(self.wrong)))

    def add_stats(self, stats):
        for k in ("clamped", "clamped_hi", "clamped_lo", "pairs"):
            stats[k] = stats.get(k, 0) + getattr(self, k)

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


def frame_loop(x, F, hop, ratio, phi=1.0, nc=LIFTER_DEFAULT, form="radians", half=True, stats=None, wrong=None):
    """One stream, one-shot: x float [T], ratio [nFrames] -> float64 [T] (pv_curve_cases.frame_loop with the correction).
    stats: a dict that receives the clamp counts."""
    cls = FormantRef if form == "radians" else FormantTurns
    r = cls(F, hop, F, phi=phi, nc=nc, half=half, wrong=wrong)  # (the block size plays no part in _frame)
    x = np.asarray(x, np.float64)
    nF = (len(x) - F) // hop + 1
    assert len(ratio) == nF
    y = np.zeros(len(x))
    for f in range(nF):
        y[f * hop:f * hop + F] += r._frame(x[f * hop:f * hop + F], f, float(ratio[f]))
    if stats is not None:
        r.add_stats(stats)
    return y * r.scale


def by_block(x, N, hop, ratio, phi=1.0, nc=LIFTER_DEFAULT, form="radians", stats=None):
    """One stream through a fresh streaming reference, block b with ratio[b]: float64 [N len(ratio)] with the stream's latency.
    stats: a dict that receives the clamp counts."""
    cls = FormantRef if form == "radians" else FormantTurns
    r = cls(N, hop, phi=phi, nc=nc)
    y = np.concatenate([r.process(x[b * N:(b + 1) * N], float(ratio[b])) for b in range(len(ratio))])
    if stats is not None:
        r.add_stats(stats)
    return y
