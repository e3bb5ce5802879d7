"""Stimuli whose whole-ring sum of squares sits a chosen distance from the silence gate's threshold, at one chosen block boundary.

The gate (MyBuffer.cpp:258-261, oracle rms_level) compares Decibels::gainToDecibels(getRMSLevel) with silenceDb = -60: a sequential
double sum of x^2 over the ring in PHYSICAL order.  The kernels replace that sum with a tree sum and decide from it outside a rounding
band; inside the band they redo the sequential sum.  These stimuli put the sequential sum at thr - k ulp, thr, thr + k ulp and thr +- delta,
so that a test reaches the band and the fallback with real data.  Shared by tests/test_gate_edge_cpu.py (the oracle) and
tests/test_gpu_transitions.py (the kernels)."""
import math
import struct

import numpy as np

SILENCE_DB = -60.0


def _gate_closed(total, n, silence_db=SILENCE_DB):
    """vp_capi.hip gate_closed / oracle: gainToDecibels(sqrt(sum / n)) < silenceDb (math.* calls the host's libm, as the C code)"""
    rms = math.sqrt(total / n)
    db = max(-100.0, math.log10(rms) * 20.0) if rms > 0.0 else -100.0
    return db < silence_db


def _d2u(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _u2d(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def gate_threshold_sum(n, silence_db=SILENCE_DB):
    """The smallest sum of squares over n samples whose gate is OPEN (vp_capi.hip gate_threshold_sum: bisection over the bit
    patterns of the positive doubles; the verdict is monotone in the sum)."""
    lo, hi = 0, _d2u(1e300)
    while lo + 1 < hi:
        mid = lo + (hi - lo) // 2
        if _gate_closed(_u2d(mid), n, silence_db):
            lo = mid
        else:
            hi = mid
    return _u2d(hi)


def ulp_steps(v, k):
    """v moved by k units in the last place (k < 0: down)"""
    return _u2d(_d2u(v) + k)


def seq_sum(ring):
    """the reference's sum: sequential float64 accumulation of x^2 in physical ring order"""
    a = np.asarray(ring, np.float64)
    return float(np.cumsum(a * a)[-1])


def ring_after_block(x, geom, b):
    """The physical ring (float64 [inSize]) of one channel x (float32 [T]) after block b has been written: sample t of the stream sits
    at (toKeep + latency + t) % inSize (MyBuffer: inCounter starts at toKeep + latency), zeros where nothing has been written yet."""
    N, inSize = geom["N"], geom["inSize"]
    c0 = geom["toKeep"] + geom["latency"]
    ring = np.zeros(inSize, np.float64)
    t1 = (b + 1) * N
    t0 = max(0, t1 - inSize)
    t = np.arange(t0, t1)
    ring[(c0 + t) % inSize] = x[t0:t1]
    return ring


def deltas():
    """(label, target(thr)) pairs: thr -+ k ulp for k in 1, 2, 4, thr itself, and thr +- delta on a log grid 1e-16 .. 1e-11"""
    out = [(f"thr{k:+d}ulp", (lambda k: lambda thr: ulp_steps(thr, k))(k)) for k in (-4, -2, -1)]
    out.append(("thr", lambda thr: thr))
    out += [(f"thr{k:+d}ulp", (lambda k: lambda thr: ulp_steps(thr, k))(k)) for k in (1, 2, 4)]
    for e in (-16, -15, -14, -13, -12, -11):
        out.append((f"thr-1e{e}", (lambda d: lambda thr: thr - d)(10.0 ** e)))
        out.append((f"thr+1e{e}", (lambda d: lambda thr: thr + d)(10.0 ** e)))
    return out


def _tune(prefix, target):
    """float32 x with fl(prefix + x*x) == target (x*x of a float32 is exact in double); None if no such x"""
    r = target - prefix
    if r <= 0.0:
        return None
    x = np.float32(math.sqrt(r))
    for _ in range(4096):
        v = prefix + float(x) * float(x)
        if v == target:
            return x
        x = np.nextafter(x, np.float32(np.inf if v < target else 0.0))
    return None


def _tune_below(prefix, goal):
    """the largest float32 x with fl(prefix + x*x) <= goal"""
    x = np.float32(math.sqrt(max(goal - prefix, 0.0)))
    while x > 0 and prefix + float(x) * float(x) > goal:
        x = np.nextafter(x, np.float32(0.0))
    while True:
        y = np.nextafter(x, np.float32(np.inf))
        if prefix + float(y) * float(y) > goal:
            return x
        x = y


def build(geom, n_blocks, target_block, targets, fs=44100.0, channel=0, loud=None, loud_blocks=0, seed=5, other=None):
    """float32 [S][3][n_blocks * N], S = len(targets).

    Channel `channel` of stream s (0: the voice ring; 1: the synth ring's channel 0, the vocoder's second gate) is built so that, after
    block `target_block` has been written, the sequential ring sum equals targets[s] exactly:
      * blocks [0, loud_blocks): a loud sine, amplitude loud[s] (list of (amplitude, phase)), when loud is given;
      * then zeros up to the target ring's oldest sample (at least one block of them after a loud passage: the boundary where the last
        loud samples leave decides far from the threshold, so the target boundary is the first one whose band is small);
      * the target ring: a quiet 220 Hz sine scaled to a sum just under the target, then the ring's last two PHYSICAL positions tuned
        (a coarse sample near 1e-5, a fine one near 1e-7) so that the sequential sum lands on the target;
      * blocks after the target: the quiet sine goes on.
    The other channels: `other` (float32 [3][T]) where given, else a loud sine on the non-gated channels and zeros on channel 2.
    Returns (x, sums): sums[s] is the ring sum the builder verified with a float64 cumulative sum."""
    N, inSize = geom["N"], geom["inSize"]
    T = n_blocks * N
    S = len(targets)
    t1 = (target_block + 1) * N
    r0 = t1 - inSize                                            # the target ring's oldest sample
    assert r0 >= 0, "the target ring must hold no zeros of the start"
    if loud is not None:
        assert r0 >= (loud_blocks + 1) * N, "a block of zeros between the loud passage and the target ring"
    c0 = geom["toKeep"] + geom["latency"]
    phys = (c0 + np.arange(r0, t1)) % inSize                    # physical position of every sample of the target ring
    order = np.argsort(phys)
    t_last, t_prev = r0 + order[-1], r0 + order[-2]            # the samples at the last two physical positions
    tt = np.arange(T) / fs
    x = np.zeros((S, 3, T), np.float32)
    sums = []
    for s, target in enumerate(targets):
        if other is not None:
            x[s] = other[s % len(other)]
        else:
            x[s, 1 - channel if channel in (0, 1) else 0] = (0.3 * np.sin(2 * np.pi * (180.0 + 7 * s) * tt)).astype(np.float32)
            x[s, 2] = 0.0
        sig = np.zeros(T, np.float32)
        if loud is not None:
            a, ph = loud[s]
            sig[:loud_blocks * N] = (a * np.sin(2 * np.pi * 220.0 * tt[:loud_blocks * N] + ph)).astype(np.float32)
        q = np.sin(2 * np.pi * (220.0 + 3 * s) * tt[r0:] + 0.1 * s)
        # scale the quiet part so that the ring's sum without the two tuned samples is ~1e-10 under the target
        ring_q = q[:inSize].copy()
        ring_q[[t_last - r0, t_prev - r0]] = 0.0
        k = math.sqrt((target - 1e-10) / float(np.sum(ring_q * ring_q)))
        sig[r0:] = (k * q).astype(np.float32)
        sig[t_last] = 0.0
        sig[t_prev] = 0.0
        ring = ring_after_block(sig, geom, target_block)
        assert ring[-1] == 0.0 and ring[-2] == 0.0
        pre = seq_sum(ring[:-2])
        # coarse: fl(pre + x1^2) just under target - 1e-15; fine: the rest, exactly
        x1 = _tune_below(pre, target - 2e-15)
        mid = pre + float(x1) * float(x1)
        x2 = _tune(mid, target)
        assert x2 is not None, (s, target, mid)
        sig[t_prev], sig[t_last] = x1, x2
        ring = ring_after_block(sig, geom, target_block)
        got = seq_sum(ring)
        assert got == target, (s, got, target)
        x[s, channel] = sig
        sums.append(got)
    return np.ascontiguousarray(x), sums
