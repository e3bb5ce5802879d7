"""The phase-vocoder test matrix: seeded signals, the list of cases that tests/test_pv_reference_cpu.py (conditioning gate) and
tests/test_gpu_pv_matrix.py (kernel against NumPy) BOTH iterate, and a second statement of the reference.  Test infrastructure only.

Why a second statement.  tests/stft_reference.py keeps its phases in radians; the kernels (csrc/vp_stft.hip) keep them in turns.  The
two forms agree to a few 1e-13 wherever no phase difference sits on a wrap tie, and differ by percent where one does (DC, a Nyquist
tone, an isolated click: a flipped wrap moves a bin's frequency by O = F / hop bins for good).  A pointwise comparison of the kernel
with the restatement therefore means something only on an input on which the restatement's own two forms agree: the gate.
roundtrip_turns / PvStreamTurns are that second form -- atan2 / 2 pi, d -= rint(d), the accumulator in turns, exp(2 pi i frac) --
written apart from stft_reference.stft_roundtrip (the bin gather is vectorised here, a loop there).

The bound of every pointwise comparison (bound()): the kernel's transforms and stage are double (1e-13 from NumPy's), its output frames
and their overlap-add float32.  An output sample is the float32 sum of O float32 terms: O roundings of the terms and at most O of the
partial sums, each 2^-24 relative to a partial sum; a factor 2 for partial sums larger than the result where frames cancel:
    |y - ref| <= 4 O 2^-24 max(1, max |ref|)       at every sample.
"""
import math
from collections import namedtuple

import numpy as np

import pv_stream_reference as P

F = 1024
FS = 48000.0
HOPS = (64, 128, 256, 512)
ROUND = 4                                   # frames per round of the kernels (VP_STFT_WAVES)
SEMITONES = (7.0, -12.0, 12.0, 0.37, -11.99)
GATE_TOL = 1e-9                             # the two forms of the reference, relative to max(1, max |ref|)


def bound(hop, ref):
    return 4.0 * (F // hop) * 2.0 ** -24 * max(1.0, float(np.abs(ref).max()))


def ratio_of(semitones):
    return 2.0 ** (semitones / 12.0)        # (the library: std::pow(2.0, semitones / 12.0))


# ---- signals (float32, seeded) --------------------------------------------------------------------------------------------------------
def harmonic(T, stream=0, seed=0):
    """Five harmonics of f0 (a semitone step per stream) plus noise at -40 dB."""
    rng = np.random.default_rng([seed, stream, 1])
    t = np.arange(T) / FS
    f0 = 110.0 * 2.0 ** (stream % 24 / 12.0)
    x = np.zeros(T)
    for h in range(1, 6):
        x += 0.3 / h * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi))
    return (x + 0.01 * rng.standard_normal(T)).astype(np.float32)


def white(T, seed=0):
    return (0.25 * np.random.default_rng([seed, 2]).standard_normal(T)).astype(np.float32)


def tone(T, freq=440.0, amp=0.4, seed=0):
    ph = np.random.default_rng([seed, 3]).uniform(0, 2 * np.pi)
    return (amp * np.sin(2 * np.pi * freq * np.arange(T) / FS + ph)).astype(np.float32)


def mixed_streams(T, seed=0):
    """The five streams of a pointwise case: three harmonic ones (different f0), white noise, a pure tone."""
    return np.stack([harmonic(T, 0, seed), white(T, seed), harmonic(T, 7, seed), tone(T, 440.0 + 37.0 * (seed % 5), 0.4, seed),
                     harmonic(T, 16, seed)])


def harmonic_streams(S, T, seed=0):
    return np.stack([harmonic(T, s, seed) for s in range(S)])


DEGENERATE = ("silence", "dc", "nyquist", "impulses", "square")


def degenerate(name, T):
    n = np.arange(T)
    if name == "silence":
        x = np.zeros(T)
    elif name == "dc":
        x = np.full(T, 0.5)
    elif name == "nyquist":
        x = 0.5 * (1.0 - 2.0 * (n & 1))
    elif name == "impulses":
        x = np.zeros(T)
        x[T // 3] = 1.0
        x[2 * T // 3 + 1] = -1.0
    elif name == "square":
        x = np.where((n // 32) & 1, -1.0, 1.0)               # full scale, period 64 samples: harmonics on exact bins
    else:
        raise KeyError(name)
    return x.astype(np.float32)


def magnitude_ceiling(x, hop):
    """2 Mf of the amplitude bound: Mf = 2 max over frames of sum_k |X_f[k]| / F (rfft of the windowed frame).  A frame's inverse
    transform is bounded by its magnitude sum (the stage moves and adds magnitudes, and drops those that leave the band), and the
    overlap-add weighs at most O frames by w <= 1 and scale = 2 / O: |y| <= 2 Mf whatever the phases are."""
    x = np.asarray(x, np.float64)
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(F) / F))
    nF = (len(x) - F) // hop + 1
    m = 0.0
    for f in range(nF):
        m = max(m, float(np.abs(np.fft.rfft(x[f * hop:f * hop + F] * w)).sum()))
    return 2.0 * (2.0 * m / F)


# ---- the second statement: phases in turns ---------------------------------------------------------------------------------------------
def _turns_frame(X, f, ratio, O, pp, acc, carry):
    """One frame of the stage in turns.  X: rfft of the windowed frame; pp: previous frame's phases, acc: accumulator within the round,
    carry: accumulator at the last round's end (all in turns).  Returns the synthesis spectrum and the three new states."""
    nb = len(X)
    k = np.arange(nb)
    p = np.arctan2(X.imag, X.real) / (2.0 * np.pi)
    d = p - pp - k / O                                          # (O a power of two: k / O exact)
    d = d - np.rint(d)
    fk = k + d * O
    tgt = np.floor(k * ratio + 0.5).astype(np.int64)
    ok = (tgt >= 0) & (tgt < nb)
    sm = np.zeros(nb)
    np.add.at(sm, tgt[ok], np.abs(X)[ok])                       # magnitudes add, in increasing k
    last = np.full(nb, -1)
    np.maximum.at(last, tgt[ok], k[ok])                         # the last k that lands on a bin leaves its frequency
    sf = np.where(last >= 0, fk[np.maximum(last, 0)] * ratio, 0.0)
    inc = sf / O
    acc = carry + inc if f % ROUND == 0 else acc + inc
    frac = acc - np.rint(acc)
    if f % ROUND == ROUND - 1:
        carry = frac
    Y = sm * np.exp(2j * np.pi * frac)
    Y[0] = Y[0].real
    Y[-1] = Y[-1].real
    return Y, p, acc, carry


def roundtrip_turns(x, F=F, hop=256, ratio=1.0):
    """The one-shot stage (what vp_stft_pitch_shift computes), phases in turns: float [T] -> float64 [T]."""
    x = np.asarray(x, np.float64)
    T, O, nb = len(x), F // hop, F // 2 + 1
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(F) / F))
    y = np.zeros(T)
    pp, acc, carry = np.zeros(nb), np.zeros(nb), np.zeros(nb)
    for f in range((T - F) // hop + 1):
        Y, pp, acc, carry = _turns_frame(np.fft.rfft(x[f * hop:f * hop + F] * w), f, ratio, O, pp, acc, carry)
        y[f * hop:f * hop + F] += np.fft.irfft(Y, F) * w
    return y * (2.0 / O)                                         # 1 / sum of w^2 over one hop grid


class PvStreamTurns(P.PvStreamRef):
    """PvStreamRef's call bookkeeping with the frame arithmetic in turns (p_prev, sp and carry then hold turns)."""

    def _frame(self, seg, f, ratio):
        Y, self.p_prev, self.sp, self.carry = _turns_frame(np.fft.rfft(seg * self.w), f, ratio, self.F // self.hop, self.p_prev,
                                                           self.sp, self.carry)
        return np.fft.irfft(Y, self.F) * self.w


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
OneShotCase = namedtuple("OneShotCase", "hop semitones T what")
StreamCase = namedtuple("StreamCase", "hop N n_blocks calls semitones")
Scenario = namedtuple("Scenario", "hop N n_blocks calls semitones changes resets")


def n_frames(T, hop):
    return (T - F) // hop + 1


def _lengths(hop):
    """(T, what): frame counts of every residue mod 4 (so the last round holds 4, 1, 2 and 3 frames), odd T (the unaligned loads), T
    that is no multiple of hop (tail samples no frame covers), and the two one-frame lengths."""
    base = 8 * F // hop                                          # about eight frame lengths (a multiple of 4)
    def t_of(nf, extra):
        return F + (nf - 1) * hop + extra
    out = [(F, "one frame, T = F"), (F + hop - 1, "one frame, T = F + hop - 1 (odd, tail)"),
           (t_of(base, 0), "frames mod 4 = 0, aligned"), (t_of(base + 1, hop - 1), "frames mod 4 = 1, odd T, longest tail"),
           (t_of(base + 2, 2), "frames mod 4 = 2, even T, tail of 2"), (t_of(base + 3, 3), "frames mod 4 = 3, odd T, tail of 3")]
    for T, _ in out[2:]:
        assert T >= 8 * F
    assert sorted(n_frames(T, hop) % 4 for T, _ in out[2:]) == [0, 1, 2, 3]
    return out


# three or four intervals per hop, always the two octaves (ratio 2 and 1/2: every second synthesis bin empty / two bins per synthesis bin)
_SEMIS_OF_HOP = {64: (12.0, -12.0, 7.0, -11.99), 128: (12.0, -12.0, 0.37, 7.0), 256: (12.0, -12.0, -11.99, 0.37), 512: (12.0, -12.0, 7.0, 0.37)}

ONE_SHOT_CASES = [OneShotCase(hop, v, T, what) for hop in HOPS for v in _SEMIS_OF_HOP[hop] for T, what in _lengths(hop)]


def one_shot_id(c):
    return f"hop{c.hop}-{c.semitones:+g}st-T{c.T}"


def one_shot_input(c):
    return mixed_streams(c.T, seed=c.hop + c.T)


def one_shot_reference(c, x, form="radians"):
    """[S][T] float64: the restatement of tests/stft_reference.py ("radians") or this file's ("turns")."""
    import stft_reference as R
    r = ratio_of(c.semitones)
    if form == "radians":
        return np.stack([R.stft_roundtrip(xs, F, c.hop, ratio=r) for xs in x])
    return np.stack([roundtrip_turns(xs, F, c.hop, r) for xs in x])


# streaming: every block size at the hops the suite never compared with NumPy.  N = 17 and 64 put several calls without a frame
# at hop 512, N = 4096 many rounds in one call; every stream its own interval, at least 10 F samples.
STREAM_HOPS = (64, 128, 512)
STREAM_BLOCKS = (17, 64, 100, 1000, 1024, 4096)
STREAM_CASES = [StreamCase(hop, N, max(-(-10 * F // N), 5), (1, 3, 16), SEMITONES) for hop in STREAM_HOPS for N in STREAM_BLOCKS]


def stream_id(c):
    return f"hop{c.hop}-N{c.N}"


def stream_input(c):
    return mixed_streams(c.N * c.n_blocks, seed=c.hop + c.N)


def call_spans(n_blocks, calls):
    """Blocks of each call: calls cycled until n_blocks are used."""
    out, b, i = [], 0, 0
    while b < n_blocks:
        k = min(calls[i % len(calls)], n_blocks - b)
        out.append(k)
        b += k
        i += 1
    return out


def stream_reference(c, x, form="radians"):
    cls = P.PvStreamRef if form == "radians" else PvStreamTurns
    y = np.zeros(x.shape)
    for s in range(x.shape[0]):
        r = cls(c.N, c.hop, ratio=ratio_of(c.semitones[s]))
        pos, out = 0, []
        for k in call_spans(c.n_blocks, c.calls):
            out.append(r.process(x[s, pos:pos + k * c.N]))
            pos += k * c.N
        y[s] = np.concatenate(out)
    return y


# one scenario per hop: interval changes on some streams between calls and resets of single streams; `changes` and `resets` are keyed
# by the index of the call they precede.  Blocks of 100 samples in calls of 1, 3, 16 and 2: the resets at calls 4 and 8 land in the
# middle of a round at every hop (asserted on the CPU) and the calls that follow them are shorter than F (100 samples).
SCENARIOS = [Scenario(hop, 100, 124, (1, 3, 16, 2), (2.0, 2.0, 2.0, 2.0),
                      {2: [(1, -7.0)], 5: [(3, 12.0), (1, 5.0)], 9: [(0, -12.0)], 14: [(3, -4.0)], 17: [(2, 0.37)]},
                      {4: [2], 8: [0], 13: [3]}) for hop in HOPS]


def scenario_id(c):
    return f"hop{c.hop}"


def scenario_input(c):
    return np.stack([harmonic(c.N * c.n_blocks, s, seed=c.hop + 1) if s != 1 else white(c.N * c.n_blocks, seed=c.hop + 1)
                     for s in range(len(c.semitones))])


def scenario_reference(c, x, form="radians", shift=0):
    """The restatement driven with the scenario's schedule; shift = +1 / -1 applies every change and reset one call late / early.
    Returns the output [S][T] and, per stream, [(call index, frames since the last reset mod 4, samples of the call)] of its resets."""
    cls = P.PvStreamRef if form == "radians" else PvStreamTurns
    spans = call_spans(c.n_blocks, c.calls)
    y = np.zeros(x.shape)
    landed = []
    for s in range(x.shape[0]):
        r = cls(c.N, c.hop, ratio=ratio_of(c.semitones[s]))
        pos, out, hits = 0, [], []
        for i, k in enumerate(spans):
            j = i - shift                                        # the call whose changes apply before call i
            ratio = None
            for st, v in c.changes.get(j, []):
                if st == s:
                    ratio = ratio_of(v)
            if s in c.resets.get(j, []):
                hits.append((i, r.nf % ROUND, k * c.N))
                r.reset()
            out.append(r.process(x[s, pos:pos + k * c.N], ratio))
            pos += k * c.N
        y[s] = np.concatenate(out)
        landed.append(hits)
    return y, landed


def latency(N, hop):
    return F - math.gcd(N, hop)
