"""The phase vocoder on the GPU against NumPy at every hop, length and edge (vp_stft_pitch_shift, vp_pv_*; kernels
vp_k_stft_fused<true, false> and vp_k_pv_stream of csrc/vp_stft.hip).  The cases and the reference come from tests/pv_cases.py, the
same list whose conditioning tests/test_pv_reference_cpu.py gates: every pointwise comparison here is on an input on which the
restatement's two arithmetic forms agree to 1e-9, and is held at EVERY sample to
    |y - ref| <= 4 O 2^-24 max(1, max |ref|),   O = F / hop
(float32 output frames and float32 overlap-add of O terms; pv_cases.py derives it).  Degenerate inputs (silence, DC, a Nyquist tone,
clicks, a square wave on exact bins) sit on wrap ties where no pointwise reference exists; they are held to properties that do not
depend on a wrap decision.  Output buffers start as NaN: an unwritten sample shows."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

F = K.F


# ---- running the two entry points --------------------------------------------------------------------------------------------------------
def _one_shot(x, semis, hop, handle=None):
    """vp_stft_pitch_shift on x [S][T]; semis: one interval, or one per stream (then one batch call per distinct interval)."""
    from vocoderproject_amd import StftRoundTrip
    S, T = x.shape
    st = handle or StftRoundTrip(S, T, F, hop)
    assert st.fused
    per_stream = [float(semis)] * S if np.isscalar(semis) else [float(v) for v in semis]
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    y = np.full_like(x, np.nan)
    for v in sorted(set(per_stream)):
        d_out = torch.full_like(d_in, float("nan"))
        st.pitch_shift(d_in, d_out, v)
        torch.cuda.synchronize()
        o = d_out.cpu().numpy()
        for s in range(S):
            if per_stream[s] == v:
                y[s] = o[s]
    if handle is None:
        st.close()
    return y


def _blocks(x, N):
    S, T = x.shape
    return torch.from_numpy(np.ascontiguousarray(x.reshape(S, T // N, N).transpose(1, 0, 2))).cuda()


def _unblocks(d):
    nb, S, N = d.shape
    return d.cpu().numpy().transpose(1, 0, 2).reshape(S, nb * N)


def _stream(ps, x, calls, before_call=None):
    """x [S][T] (whole blocks) through ps.process_device in calls of calls[i % len] blocks, no synchronisation between the calls;
    before_call(i) runs in front of call i (interval changes, resets)."""
    d_in = _blocks(x, ps.N)
    d_out = torch.full_like(d_in, float("nan"))
    b = 0
    for i, k in enumerate(K.call_spans(d_in.shape[0], calls)):
        if before_call:
            before_call(i)
        ps.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k)
        b += k
    torch.cuda.synchronize()
    return _unblocks(d_out)


def _new_stream(S, N, hop, semis):
    from vocoderproject_amd import PhaseVocoderStream
    ps = PhaseVocoderStream(S, N, hop=hop)
    assert ps.latency == K.latency(N, hop)
    for s, v in enumerate(semis):
        ps.set_semitones(v, stream=s)
    return ps


# ---- comparing -------------------------------------------------------------------------------------------------------------------------------
def _pointwise(y, ref, hop, what):
    """Every sample of every stream within the bound; the project's older pair (rms, share of samples beyond 1e-5) too."""
    assert y.shape == ref.shape and y.dtype == np.float32
    assert not np.isnan(y).any(), f"{what}: {int(np.isnan(y).sum())} samples unwritten or NaN, first at {np.argwhere(np.isnan(y))[0]}"
    err = np.abs(y.astype(np.float64) - ref)
    bnd = K.bound(hop, ref)
    rms = float(np.sqrt((err ** 2).mean()))
    share = float((err > 1e-5).mean())
    print(f"PVMATRIX {what} max_err {err.max():.3e} bound {bnd:.3e} err/bound {err.max() / bnd:.3f} rms {rms:.3e} share>1e-5 {share:.2e}")
    if err.max() > bnd:
        s, t = np.unravel_index(np.argmax(err), err.shape)
        f_lo, f_hi = max(0, (t - F) // hop + 1), t // hop
        bad = int((err > bnd).sum())
        raise AssertionError(f"{what}: {bad} samples beyond the bound {bnd:.3e}; worst {err.max():.3e} at stream {s} sample {t} "
                             f"(frames {f_lo}..{f_hi} cover it), y {y[s, t]!r} ref {ref[s, t]!r}; first bad sample "
                             f"{np.argwhere(err > bnd)[0]}")
    assert rms < 1e-4 and share < 1e-3, (what, rms, share)
    return float(err.max()), bnd


def _bits(a, b, what):
    assert a.shape == b.shape, what
    assert not np.isnan(a).any() and not np.isnan(b).any(), what
    if not np.array_equal(a, b):
        d = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(d)} samples differ, first at {d[0]}, max {np.abs(a.astype(np.float64) - b).max():.3g}")


def _delayed(one, L):
    """The one-shot output [S][T] as the stream emits it: L zeros first."""
    out = np.zeros_like(one)
    out[:, L:] = one[:, :one.shape[1] - L]
    return out


# ---- a. the one-shot against NumPy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.ONE_SHOT_CASES, ids=K.one_shot_id)
def test_one_shot_against_numpy(case):
    x = K.one_shot_input(case)
    y = _one_shot(x, case.semitones, case.hop)
    ref = K.one_shot_reference(case, x)
    _pointwise(y, ref, case.hop, f"one-shot {K.one_shot_id(case)} ({case.what})")
    covered = (K.n_frames(case.T, case.hop) - 1) * case.hop + F
    assert np.all(y[:, covered:] == 0), "samples no frame covers must come out 0"
    assert np.sqrt((ref ** 2).mean()) > 0.01                                    # (a comparison of something)


# ---- b. the stream against NumPy, directly ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.STREAM_CASES, ids=K.stream_id)
def test_stream_against_numpy(case):
    x = K.stream_input(case)
    ps = _new_stream(x.shape[0], case.N, case.hop, case.semitones)
    y = _stream(ps, x, case.calls)
    ps.close()
    ref = K.stream_reference(case, x)
    L = K.latency(case.N, case.hop)
    assert np.all(y[:, :L] == 0), "the latency's samples are exact zeros"
    _pointwise(y, ref, case.hop, f"stream {K.stream_id(case)}")
    assert np.sqrt((ref ** 2).mean()) > 0.01


@pytest.mark.parametrize("case", K.SCENARIOS, ids=K.scenario_id)
def test_stream_scenario_against_numpy(case):
    """Interval changes between calls, a reset in the middle of a round, a reset followed by a call shorter than a frame -- against the
    restatement driven with the same schedule; the schedule one call early or late is outside the bound."""
    x = K.scenario_input(case)
    ps = _new_stream(x.shape[0], case.N, case.hop, case.semitones)

    def before_call(i):
        for s, v in case.changes.get(i, []):
            ps.set_semitones(v, stream=s)
        for s in case.resets.get(i, []):
            ps.reset(s)

    y = _stream(ps, x, case.calls, before_call)
    ps.close()
    ref, landed = K.scenario_reference(case, x)
    assert any(fr != 0 and m < F for hits in landed for _, fr, m in hits)
    assert np.all(y[:, :K.latency(case.N, case.hop)] == 0)
    _, bnd = _pointwise(y, ref, case.hop, f"scenario {K.scenario_id(case)}")
    for sh in (-1, 1):
        other = K.scenario_reference(case, x, shift=sh)[0]
        worst = float(np.abs(y - other).max())
        print(f"PVMATRIX scenario {K.scenario_id(case)} schedule shifted by {sh:+d}: max_err {worst:.3e} bound {bnd:.3e}")
        assert worst > bnd, sh


# ---- c. stream == one-shot, bit for bit, at the hops never run -------------------------------------------------------------------------
@pytest.mark.parametrize("hop,N", [(64, 48), (64, 64), (64, 1500), (512, 200), (512, 512), (512, 1500)])
def test_stream_is_the_one_shot_bit_for_bit(hop, N):
    S = 37
    semis = [K.SEMITONES[s % len(K.SEMITONES)] for s in range(S)]
    x = K.harmonic_streams(S, N * max(-(-6 * F // N), 5), seed=hop + N)
    ps = _new_stream(S, N, hop, semis)
    y = _stream(ps, x, (1, 3, 16))
    ps.close()
    _bits(y, _delayed(_one_shot(x, semis, hop), K.latency(N, hop)), f"hop {hop} N {N}")
    assert np.abs(y).max() > 0.1


# ---- d. degenerate inputs, through both entry points ------------------------------------------------------------------------------------
DEG_SEMIS = (7.0, -12.0, 0.37, 12.0)


@pytest.mark.parametrize("hop", K.HOPS)
@pytest.mark.parametrize("name", K.DEGENERATE)
def test_degenerate_inputs(name, hop):
    """Silence gives exact zeros.  DC, a Nyquist tone, two clicks and a square wave sit on wrap ties (tests/test_pv_reference_cpu.py
    records that the reference's own two forms disagree there), so: every sample finite, |y| <= 2 Mf (1 + 1e-6) -- a frame's inverse
    transform is bounded by its magnitude sum, the overlap-add weighs at most O frames by w <= 1 and 2 / O -- and the stream equals
    the one-shot delayed by L bit for bit.  One odd length (unaligned loads) and one of whole blocks."""
    N, calls = 100, (1, 3, 16)
    for T in (8 * F + hop + 3, N * 90):
        x = np.stack([K.degenerate(name, T)] * len(DEG_SEMIS))
        y = _one_shot(x, DEG_SEMIS, hop)
        assert np.isfinite(y).all(), (name, hop, T)
        if name == "silence":
            assert np.all(y == 0)
        top = K.magnitude_ceiling(x[0], hop) * (1 + 1e-6)
        print(f"PVMATRIX degenerate {name} hop{hop} T{T}: max |y| {np.abs(y).max():.4f} ceiling {top:.4f}")
        assert np.abs(y).max() <= top
    ps = _new_stream(len(DEG_SEMIS), N, hop, DEG_SEMIS)
    ys = _stream(ps, x, calls)
    ps.close()
    _bits(ys, _delayed(y, K.latency(N, hop)), f"{name} hop {hop}: stream against one-shot")
    if name == "silence":
        assert np.all(ys == 0)


@pytest.mark.parametrize("hop", K.HOPS)
def test_power_of_two_homogeneity(hop):
    """Every operation of the stage commutes with a power-of-two scale while nothing under- or overflows: the output for x 2^e is the
    output for x times 2^e, bit for bit.  An absolute threshold or a single-precision intermediate would break it."""
    N = 256
    x = K.mixed_streams(N * 28 + 1, seed=hop)                                  # odd T for the one-shot
    semis = K.SEMITONES
    y0 = _one_shot(x, semis, hop)
    ps = _new_stream(5, N, hop, semis)
    s0 = _stream(ps, x[:, :-1], (1, 3, 16))
    assert np.abs(y0).max() > 0.1 and np.abs(s0).max() > 0.1
    for e in (-40, 12):
        c = np.float32(2.0 ** e)
        _bits(_one_shot(x * c, semis, hop), y0 * c, f"hop {hop}: one-shot, x 2^{e}")
        ps.reset()
        _bits(_stream(ps, x[:, :-1] * c, (1, 3, 16)), s0 * c, f"hop {hop}: stream, x 2^{e}")
    ps.close()


@pytest.mark.parametrize("hop", K.HOPS)
def test_stream_rows_are_independent(hop):
    """Permuting the S input rows permutes the output rows, bit for bit (odd T: odd rows of the one-shot start unaligned)."""
    S, N = 37, 100
    perm = np.random.default_rng(hop).permutation(S)
    x = K.harmonic_streams(S, N * 52 + 1, seed=hop)
    x[5] = K.white(x.shape[1], seed=hop)
    xp = np.ascontiguousarray(x[perm])
    y = _one_shot(x, -5.0, hop)
    _bits(_one_shot(xp, -5.0, hop), y[perm], f"hop {hop}: one-shot rows")
    semis = [K.SEMITONES[s % len(K.SEMITONES)] for s in range(S)]
    a = _new_stream(S, N, hop, semis)
    b = _new_stream(S, N, hop, [semis[p] for p in perm])
    ya = _stream(a, x[:, :-1], (1, 3, 16))
    yb = _stream(b, xp[:, :-1], (1, 3, 16))
    a.close()
    b.close()
    _bits(yb, ya[perm], f"hop {hop}: stream rows")
    assert np.abs(y).max() > 0.1 and np.abs(ya).max() > 0.1


@pytest.mark.parametrize("hop", K.HOPS)
def test_no_state_survives_a_one_shot_call(hop):
    from vocoderproject_amd import StftRoundTrip
    x = K.mixed_streams(6 * F + hop + 3, seed=hop + 9)
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    first = _one_shot(x, 7.0, hop, handle=st)
    second = _one_shot(x, -5.0, hop, handle=st)
    third = _one_shot(x, 7.0, hop, handle=st)
    st.close()
    _bits(first, _one_shot(x, 7.0, hop), f"hop {hop}: first call")
    _bits(second, _one_shot(x, -5.0, hop), f"hop {hop}: second call, other interval")
    _bits(third, first, f"hop {hop}: the first interval again")
    assert not np.array_equal(first, second)
