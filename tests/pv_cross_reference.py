"""Build-authored NumPy definition of the STFT CROSS-SYNTHESIS (vp_stft_cross_synth, vp_xs_process_blocks_device;
csrc/vp_stft_cross.inc).  No reference counterpart -- PARITY UNPINNED by nature.  Test infrastructure only.

Per stream two inputs of equal length, voice v and carrier c.  Frames, window, scale and overlap-add are stft_reference.stft_roundtrip's,
operation for operation.  Between the transforms, with nb = F / 2 + 1:

    V = rfft(w v_frame),  C = rfft(w c_frame)
    env(m) = pv_formant_reference.envelope(m, F, nc)       0.5 log(m^2 + 1e-12) -> irfft -> lifter (1 .. 1, 1/2 at nc, 0) -> rfft.real
    ev = env(|V|),  ec = env(|C|)
    d     = fmin(fmax(depth, 0), 1)                        per stream; a NaN is 0; depth None is 1
    delta = min(d (ev - ec), ln 256)                       upper clamp only: +48 dB
    Y = C exp(delta)                                       a real gain per bin: bins 0 and F / 2 stay real by themselves
    frame_out = irfft(Y, F) w

No lower clamp: a silent voice silences the carrier.  Two identities hold EXACTLY: depth 0 gives delta = +-0, exp = 1 and Y = C, the plain
round trip of the carrier; voice == carrier gives ev == ec and the same.

WRONG names what a plausible wrong kernel would compute, one deviation each; every function below takes one of the names as an optional
`wrong` (None: the definition above).  tests/test_pv_cross_reference_cpu.py asserts how far each is from the definition.
"""
import numpy as np

import pv_formant_reference as FR
import pv_stream_reference as P
import stft_reference as R

LN256 = float(np.log(256.0))
LIFTER_DEFAULT = 32
WRONG = ("floor-1e-11",          # the logarithm's floor ten times as high
         "no-whiten",            # ec = 0: the carrier's own envelope stays in
         "lifter+1",             # the lifter one sample longer
         "no-half",              # lifter weight 1 at nc
         "cap-ln128",            # the clamp at +42 dB
         "no-cap",               # no clamp
         "low-clamp",            # also clamped at -ln 256
         "swap",                 # ec - ev
         "depth-after-clamp")    # d min(ev - ec, cap)


def clamp_depth(depth):
    """fmin(fmax(depth, 0), 1): a NaN becomes 0; None (the library's NULL table) is 1."""
    return 1.0 if depth is None else float(np.fmin(np.fmax(np.float64(depth), 0.0), 1.0))


def envelopes(V, C, F, nc, wrong=None):
    """(ev, ec) [nb] each, of the magnitudes of the two spectra."""
    n = nc + 1 if wrong == "lifter+1" else nc
    half = wrong != "no-half"
    fl = "floor-1e-11" if wrong == "floor-1e-11" else None
    ev = FR.envelope(np.abs(V), F, n, half, fl)
    ec = FR.envelope(np.abs(C), F, n, half, fl)
    return ev, (np.zeros_like(ec) if wrong == "no-whiten" else ec)


def log_gain(V, C, F, depth, nc, wrong=None):
    """(delta [nb], raw d (ev - ec) [nb]) of one frame's spectra."""
    d = clamp_depth(depth)
    ev, ec = envelopes(V, C, F, nc, wrong)
    diff = (ec - ev) if wrong == "swap" else (ev - ec)
    raw = d * diff
    cap = float(np.log(128.0)) if wrong == "cap-ln128" else LN256
    if wrong == "no-cap":
        delta = raw
    elif wrong == "depth-after-clamp":
        delta = d * np.minimum(diff, cap)
    elif wrong == "low-clamp":
        delta = np.clip(raw, -cap, cap)
    else:
        delta = np.minimum(raw, cap)
    return delta, raw


def cross_frame(vseg, cseg, w, F, depth, nc, wrong=None, stats=None):
    """One output frame (windowed, unscaled) from the two input frames."""
    V = np.fft.rfft(vseg * w)
    C = np.fft.rfft(cseg * w)
    delta, raw = log_gain(V, C, F, depth, nc, wrong)
    if stats is not None:
        stats["pairs"] = stats.get("pairs", 0) + len(raw)
        stats["clamped"] = stats.get("clamped", 0) + int(np.count_nonzero(raw >= LN256))
        stats["clamped_nonzero"] = stats.get("clamped_nonzero", 0) + int(np.count_nonzero((raw >= LN256) & (np.abs(C) > 0.0)))
    return np.fft.irfft(C * np.exp(delta), F) * w


def cross_synth(v, c, F=1024, hop=256, depth=None, nc=LIFTER_DEFAULT, wrong=None, stats=None):
    """One stream, one-shot: v, c float [T] -> float64 [T] (stft_reference.stft_roundtrip's loop around cross_frame)."""
    v = np.asarray(v, np.float64)
    c = np.asarray(c, np.float64)
    assert v.shape == c.shape and v.ndim == 1
    T = len(c)
    w = R.window(F)
    scale = 1.0 / np.sum(w[::hop] ** 2)
    nF = (T - F) // hop + 1
    y = np.zeros(T)
    for f in range(nF):
        y[f * hop:f * hop + F] += cross_frame(v[f * hop:f * hop + F], c[f * hop:f * hop + F], w, F, depth, nc, wrong, stats)
    return y * scale


class CrossStreamRef:
    """The streaming form, one stream: pv_stream_reference.PvStreamRef's bookkeeping (frame grid, latency L = F - gcd(N, hop), emit) with
    two input histories and cross_frame as the stage.  Output sample t is one-shot sample t - L of everything received since create or
    reset.  depth and nc are the call's: a frame takes those of the call in which its last sample arrives."""

    def __init__(self, N, hop=256, F=1024):
        self.N, self.hop, self.F = int(N), int(hop), int(F)
        self.L = P.latency(N, hop, F)
        self.w = R.window(F)
        self.scale = 1.0 / np.sum(self.w[::hop] ** 2)
        self.reset()

    def reset(self):
        self.n = 0                          # samples received
        self.nf = 0                         # frames computed
        self.hv = np.zeros(0)               # voice samples [nf hop, n)
        self.hc = np.zeros(0)               # carrier samples [nf hop, n)
        self.y0 = -self.L                   # one-shot sample index of self.y[0]: the next one to emit
        self.y = np.zeros(self.L + self.F)  # overlap-add sums (float64, unscaled, as cross_synth)

    def process(self, v, c, depth=None, nc=LIFTER_DEFAULT):
        v = np.asarray(v, np.float64)
        c = np.asarray(c, np.float64)
        assert v.shape == c.shape
        M = len(c)
        F, hop = self.F, self.hop
        bv, bc = np.concatenate([self.hv, v]), np.concatenate([self.hc, c])
        base = self.nf * hop
        Rn = self.n + M
        fb = (Rn - F) // hop + 1 if Rn >= F else 0
        end = Rn - self.L
        need = max(end, (fb - 1) * hop + F if fb > 0 else 0) - self.y0
        if need > len(self.y):
            self.y = np.concatenate([self.y, np.zeros(need - len(self.y))])
        for f in range(self.nf, fb):
            a = f * hop - base
            o = f * hop - self.y0
            self.y[o:o + F] += cross_frame(bv[a:a + F], bc[a:a + F], self.w, F, depth, nc)
        self.nf = fb
        out = self.y[:M] * self.scale
        out[:max(0, min(M, -self.y0))] = 0.0
        self.y = np.concatenate([self.y[M:], np.zeros(M)])
        self.y0 += M
        self.n = Rn
        self.hv, self.hc = bv[fb * hop - base:], bc[fb * hop - base:]
        return out


def stream(v, c, N, hop=256, depth=None, nc=LIFTER_DEFAULT, calls=None):
    """Streams v, c [T] (T a multiple of N) through one CrossStreamRef in calls of `calls` blocks each (a list, cycled; default one block
    per call): the concatenated output [T]."""
    s = CrossStreamRef(N, hop)
    T = len(c)
    assert T % N == 0 and len(v) == T
    calls = calls or [1]
    out, pos, i = [], 0, 0
    while pos < T:
        k = min(calls[i % len(calls)], (T - pos) // N)
        out.append(s.process(v[pos:pos + k * N], c[pos:pos + k * N], depth, nc))
        pos += k * N
        i += 1
    return np.concatenate(out)
