"""The phase-vocoder pitch shift along a ratio curve on the GPU (include/vp_amd.h vp_stft_pitch_shift_curve,
vp_pv_process_blocks_curve_device; kernels vp_k_stft_pv_curve, vp_k_stft_pv2k_curve, vp_k_pv_stream_curve of csrc/vp_stft_curve.inc):
against the NumPy reference of a per-frame ratio on every case of tests/pv_curve_cases.py (whose conditioning
tests/test_pv_curve_reference_cpu.py gates), bit-identical to the fixed-interval kernels wherever the curve is constant, the streaming
call bit-identical to single-block calls with vp_pv_set_semitones in front of each, the one-shot and the streaming call identical to each
other, the clamp, and the neighbours on the same handle."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_curve_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

CALLS = (1, 3, 16, 4)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _curve(st, x, d_ratio=None, semitones=None):
    """One vp_stft_pitch_shift_curve call on x [S][T]; the output starts as NaN, so every sample must have been written."""
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    st.pitch_shift_curve(d_in, d_out, semitones=semitones, d_ratio=d_ratio)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


# ---- 1. one-shot against NumPy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CC.CASES, ids=CC.case_id)
def test_one_shot_curve_matches_numpy(c):
    from vocoderproject_amd import StftRoundTrip
    x, ref = CC.case_input(c), CC.reference(c)
    T = CC.length(c)
    st = StftRoundTrip(CC.N_STREAMS, T, c.F, c.hop)
    assert st.n_frames == c.nF
    y = _curve(st, x, semitones=CC.semitones_of(c))
    st.close()
    assert np.all(np.isfinite(y))
    for s in range(CC.N_STREAMS):
        err, bnd = np.abs(y[s] - ref[s]).max(), CC.bound(c, ref[s])
        print(f"CURVE {CC.case_id(c)} stream {s}: err {err:.3g} bound {bnd:.3g}")
        assert err <= bnd, (s, err, bnd)
    covered = (c.nF - 1) * c.hop + c.F
    assert np.all(y[:, covered:] == 0) and y[:, covered:].shape[1] == (3 if c.nF == 19 else 0)   # samples no frame covers


def test_one_curve_for_every_stream_is_broadcast():
    from vocoderproject_amd import StftRoundTrip
    c = CC.CurveCase(1024, 256, 19, "glide")
    x = CC.case_input(c)
    st = StftRoundTrip(CC.N_STREAMS, CC.length(c), c.F, c.hop)
    row = CC.semitones_of(c)[0]
    y1 = _curve(st, x, semitones=row)
    y2 = _curve(st, x, semitones=np.tile(row, (CC.N_STREAMS, 1)))
    assert len(st._curve_tables) == 1                                                # one table per handle and shape
    st.close()
    assert np.array_equal(y1, y2)
    ref = CC.reference(c)
    assert np.abs(y1[0] - ref[0]).max() <= CC.bound(c, ref[0])


# ---- 2. a curve that is constant per stream is the fixed-interval kernel, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("F,hop", [(1024, 256), (1024, 512), (2048, 256), (2048, 512)])
def test_constant_curve_is_bit_identical_to_pitch_shift(F, hop):
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios
    nF = 19
    T = F + (nF - 1) * hop + 3
    x = pv_cases.mixed_streams(T, seed=hop + 5)
    st = StftRoundTrip(CC.N_STREAMS, T, F, hop)
    ratio = np.repeat(semitones_to_ratios(pv_cases.SEMITONES)[:, None], nF, axis=1)
    y = _curve(st, x, d_ratio=_dev(ratio, np.float64))
    d_in = _dev(x, np.float32)
    d_out = torch.empty_like(d_in)
    for s, v in enumerate(pv_cases.SEMITONES):
        st.pitch_shift(d_in, d_out, v)
        torch.cuda.synchronize()
        o = d_out.cpu().numpy()
        assert np.array_equal(y[s], o[s]), (s, v, np.abs(y[s] - o[s]).max())
    st.close()


# ---- 3. streaming: the curve call against single-block calls with set_semitones in front of each -------------------------------------------
def _blocks(x, N):
    S, T = x.shape
    return _dev(x.reshape(S, T // N, N).transpose(1, 0, 2), np.float32)


def _rows(d):
    nb, S, N = d.shape
    return d.cpu().numpy().transpose(1, 0, 2).reshape(S, nb * N)


@pytest.mark.parametrize("hop", [128, 512])
@pytest.mark.parametrize("N", [100, 256, 1024])
def test_streaming_curve_is_bit_identical_to_single_block_calls(N, hop):
    from vocoderproject_amd import PhaseVocoderStream, semitones_to_ratios
    S, nb, tail = CC.N_STREAMS, 24, 2
    rng = np.random.default_rng([N, hop, 3])
    semis = rng.uniform(-12.0, 12.0, (nb, S))
    held = list(pv_cases.SEMITONES)                                                   # the interval of the plain calls
    x = pv_cases.mixed_streams(N * (nb + tail), seed=hop + N)
    spans = pv_cases.call_spans(nb, CALLS)
    assert spans == [1, 3, 16, 4]
    reset_call, reset_stream = 2, 2                                                  # pending before the call of 16 blocks (block 4 on)
    d_in = _blocks(x, N)

    a = PhaseVocoderStream(S, N, hop=hop)
    for s, v in enumerate(held):
        a.set_semitones(v, stream=s)                                                 # pending at the first curve call: stored, not used
    ya = torch.full_like(d_in, float("nan"))
    b0 = 0
    for i, k in enumerate(spans):
        if i == reset_call:
            a.reset(reset_stream)
        if i == 1:
            a.process_device(d_in[b0:b0 + k], ya[b0:b0 + k], n_blocks=k, semitones_per_block=semis[b0:b0 + k])
        else:
            a.process_device(d_in[b0:b0 + k], ya[b0:b0 + k], n_blocks=k, d_ratio=_dev(semitones_to_ratios(semis[b0:b0 + k]), np.float64))
        b0 += k
    for s, v in enumerate(held):
        assert a.semitones(s) == v
    a.process_device(d_in[nb:], ya[nb:], n_blocks=tail)                              # a plain call: the held intervals again

    b = PhaseVocoderStream(S, N, hop=hop)                                            # the twin never sees a curve call
    yb = torch.full_like(d_in, float("nan"))
    for blk in range(nb):
        if blk == sum(spans[:reset_call]):
            b.reset(reset_stream)
        for s in range(S):
            b.set_semitones(semis[blk, s], stream=s)
        b.process_device(d_in[blk], yb[blk])
    for s, v in enumerate(held):
        b.set_semitones(v, stream=s)
    b.process_device(d_in[nb:], yb[nb:], n_blocks=tail)
    torch.cuda.synchronize()
    ya, yb = _rows(ya), _rows(yb)
    a.close()
    b.close()
    assert np.all(np.isfinite(ya)) and np.all(np.isfinite(yb))
    for s in range(S):
        assert np.array_equal(ya[s, :nb * N], yb[s, :nb * N]), (s, "curve calls", np.abs(ya[s] - yb[s]).max())
        assert np.array_equal(ya[s, nb * N:], yb[s, nb * N:]), (s, "the plain call behind them")
    assert np.abs(ya[:, nb * N:]).max() > 0


def test_streaming_curve_matches_numpy():
    """The per-block schedule against the NumPy restatement driven block by block (hop 128, N = 100: blocks that end inside a round)."""
    from vocoderproject_amd import PhaseVocoderStream
    import pv_stream_reference as P
    S, N, hop, nb = CC.N_STREAMS, 100, 128, 24
    semis = np.random.default_rng([N, hop, 4]).uniform(-12.0, 12.0, (nb, S))
    x = pv_cases.mixed_streams(N * nb, seed=hop + N)
    ps = PhaseVocoderStream(S, N, hop=hop)
    d_in = _blocks(x, N)
    d_out = torch.full_like(d_in, float("nan"))
    b0 = 0
    for k in pv_cases.call_spans(nb, CALLS):
        ps.process_device(d_in[b0:b0 + k], d_out[b0:b0 + k], n_blocks=k, semitones_per_block=semis[b0:b0 + k])
        b0 += k
    torch.cuda.synchronize()
    y = _rows(d_out)
    ps.close()
    for s in range(S):
        r = P.PvStreamRef(N, hop)
        ref = np.concatenate([r.process(x[s, blk * N:(blk + 1) * N], pv_cases.ratio_of(semis[blk, s])) for blk in range(nb)])
        assert np.abs(y[s] - ref).max() <= pv_cases.bound(hop, ref), s


# ---- 4. the one-shot curve against the streaming curve --------------------------------------------------------------------------------------
# (64, 256): a first call in which no frame completes; (256, 256): the call of 16 blocks starts at the stream's frame 1, wavefront 1's
@pytest.mark.parametrize("N,hop,nb", [(1024, 256, 8), (100, 128, 60), (256, 512, 24), (64, 256, 128), (256, 256, 32)])
def test_one_shot_and_streaming_curves_agree_bit_for_bit(N, hop, nb):
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, semitones_to_ratios
    S, F, T = CC.N_STREAMS, 1024, N * nb
    x = pv_cases.mixed_streams(T, seed=hop + N + 1)
    tab = semitones_to_ratios(np.random.default_rng([N, hop, 5]).uniform(-12.0, 12.0, (nb, S)))       # [nb][S]
    nF = (T - F) // hop + 1
    blk = (np.arange(nF) * hop + F - 1) // N                                          # the block in which frame f's last sample arrives
    assert blk.max() < nb and len(set(blk)) > 3
    st = StftRoundTrip(S, T, F, hop)
    y1 = _curve(st, x, d_ratio=_dev(tab[blk].T, np.float64))
    st.close()
    ps = PhaseVocoderStream(S, N, hop=hop)
    d_in = _blocks(x, N)
    d_out = torch.full_like(d_in, float("nan"))
    b0 = 0
    for k in pv_cases.call_spans(nb, CALLS):
        ps.process_device(d_in[b0:b0 + k], d_out[b0:b0 + k], n_blocks=k, d_ratio=_dev(tab[b0:b0 + k], np.float64))
        b0 += k
    torch.cuda.synchronize()
    y2 = _rows(d_out)
    L = ps.latency
    ps.close()
    n = min(nF * hop, T - L)                                                          # finished one-shot samples that the stream has emitted
    assert n > 2 * F
    assert np.all(y2[:, :L] == 0)
    for s in range(S):
        assert np.array_equal(y2[s, L:L + n], y1[s, :n]), (s, np.abs(y2[s, L:L + n] - y1[s, :n]).max())


def test_run_with_a_curve_is_the_loop_over_process_device():
    from vocoderproject_amd import PhaseVocoderStream
    S, N, T = 3, 256, 5000
    x = pv_cases.mixed_streams(T, seed=2)[:S]
    ps = PhaseVocoderStream(S, N)
    L = ps.latency
    nb = -(-(T + L) // N)
    curve = np.linspace(-12.0, 12.0, nb)[:, None] * np.array([1.0, -1.0, 0.5])
    y = ps.run(x, blocks_per_call=16, curve=curve)
    ps.reset()
    xp = np.zeros((S, nb * N), np.float32)
    xp[:, :T] = x
    d_in = _blocks(xp, N)
    d_out = torch.empty_like(d_in)
    for blk in range(nb):
        ps.process_device(d_in[blk], d_out[blk], semitones_per_block=curve[blk:blk + 1])
    torch.cuda.synchronize()
    ref = _rows(d_out)[:, L:L + T]
    ps.close()
    assert y.shape == x.shape and np.array_equal(y, ref) and np.abs(y).max() > 0


# ---- 5. the clamp -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1024, 2048])
def test_ratios_are_clamped_and_a_nan_becomes_one_half(F):
    from vocoderproject_amd import StftRoundTrip
    c = CC.CurveCase(F, 256, 19, "vibrato")
    x, clean = CC.case_input(c), CC.ratios_of(c)
    dirty, clamped = clean.copy(), clean.copy()
    for f, v, w in ((2, 0.1, 0.5), (5, 7.0, 2.0), (6, float("nan"), 0.5), (11, -1.0, 0.5), (18, float("inf"), 2.0)):
        dirty[2, f], clamped[2, f] = v, w
    st = StftRoundTrip(CC.N_STREAMS, CC.length(c), F, 256)
    yd = _curve(st, x, d_ratio=_dev(dirty, np.float64))                              # (returns VP_OK: the wrapper raises otherwise)
    yc = _curve(st, x, d_ratio=_dev(clamped, np.float64))
    y0 = _curve(st, x, d_ratio=_dev(clean, np.float64))
    st.close()
    assert np.all(np.isfinite(yd))
    assert np.array_equal(yd[2], yc[2]) and not np.array_equal(yd[2], y0[2])
    for s in (0, 1, 3, 4):
        assert np.array_equal(yd[s], y0[s]), s


# ---- 6. the neighbours ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1024, 2048])
def test_round_trip_and_pitch_shift_keep_their_bits_around_a_curve_call(F):
    from vocoderproject_amd import StftRoundTrip
    c = CC.CurveCase(F, 512, 19, "steps")
    x = CC.case_input(c)
    st = StftRoundTrip(CC.N_STREAMS, CC.length(c), F, 512)
    d_in = _dev(x, np.float32)

    def both():
        o1, o2 = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
        st(d_in, o1)
        st.pitch_shift(d_in, o2, -5.0)
        torch.cuda.synchronize()
        return o1.cpu().numpy(), o2.cpu().numpy()
    r0, p0 = both()
    y = _curve(st, x, semitones=CC.semitones_of(c))
    r1, p1 = both()
    st.close()
    assert np.array_equal(r0, r1) and np.array_equal(p0, p1) and not np.array_equal(y, p0)


def test_streaming_curve_calls_allocate_nothing():
    from vocoderproject_amd import PhaseVocoderStream, semitones_to_ratios
    S, N, k = 4, 256, 3
    ps = PhaseVocoderStream(S, N)
    d_in = _dev(np.random.default_rng(1).standard_normal((k, S, N)) * 0.1, np.float32)
    d_out = torch.empty_like(d_in)
    d_ratio = _dev(semitones_to_ratios(np.random.default_rng(2).uniform(-12, 12, (k, S))), np.float64)
    n0 = ps.debug_alloc_count()
    for _ in range(20):
        ps.process_device(d_in, d_out, n_blocks=k, d_ratio=d_ratio)
    torch.cuda.synchronize()
    assert ps.debug_alloc_count() == n0 and n0 > 0
    ps.close()
