"""The peak-locked phase-vocoder pitch shift on the GPU (include/vp_amd.h vp_stft_pitch_shift_locked, vp_pv_process_blocks_locked_device;
kernels vp_k_stft_pv_lock and vp_k_pv_stream_lock of csrc/vp_stft_lock.inc): against the NumPy definition tests/pv_lock_reference.py on
the cases of tests/pv_lock_cases.py (whose conditioning tests/test_pv_lock_reference_cpu.py gates), the identity at ratio 1, the streaming
call bit-identical to the one-shot under every grouping, resets and changes of kind on one handle, independence of the streams,
homogeneity, silence, degenerate inputs, more workgroups than compute units, argument errors, no allocation, and what the stage is for:
a shifted tone keeps its level.  The PVLOCK lines (-s) are what profiles/pv_lock_errors.txt is made of."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_lock_cases as LC  # noqa: E402
import pv_lock_reference as LR  # noqa: E402
import stft_reference  # noqa: E402

pytestmark = pytest.mark.gpu

S, F = len(LC.GPU_STREAMS), LC.F
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4              # include/vp_amd.h


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _locked(st, x, ratio):
    """One vp_stft_pitch_shift_locked call on x [S][T] with a table of ratios; the output starts as NaN, so every sample must have been
    written."""
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    d_ratio = _dev(ratio, np.float64)
    rc = st.L.vp_stft_pitch_shift_locked(st.h, d_in.data_ptr(), d_out.data_ptr(), d_ratio.data_ptr(), _cur())
    torch.cuda.synchronize()
    assert rc == 0, (rc, st.L.vp_stft_last_error(st.h))
    return d_out.cpu().numpy()


def _one_shot(x, ratio, hop):
    from vocoderproject_amd import StftRoundTrip
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    y = _locked(st, x, ratio)
    st.close()
    return y


def _blocks(x, N):
    n, T = x.shape
    return _dev(x.reshape(n, T // N, N).transpose(1, 0, 2), np.float32)


def _rows(d):
    nb, n, N = d.shape
    return d.cpu().numpy().transpose(1, 0, 2).reshape(n, nb * N)


def _stream_locked(ps, d_in, d_tab, spans, b0=0, d_out=None):
    """Locked calls of `spans` blocks each from block b0 on; returns the device output [n_blocks][S][N] (NaN where no call wrote)."""
    if d_out is None:
        d_out = torch.full_like(d_in, float("nan"))
    for k in spans:
        rc = ps.L.vp_pv_process_blocks_locked_device(ps.h, d_in[b0:b0 + k].data_ptr(), d_out[b0:b0 + k].data_ptr(), d_tab[b0:b0 + k].data_ptr(), k, _cur())
        assert rc == 0, rc
        b0 += k
    return d_out


# ---- 1. one-shot against NumPy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nF", LC.GPU_NF)
@pytest.mark.parametrize("hop", LC.GPU_HOPS)
def test_one_shot_locked_matches_numpy(hop, nF):
    """Mixed content, every residue mod 4 of the last round, a tail of hop - 1 samples no frame covers, every curve."""
    from vocoderproject_amd import StftRoundTrip
    x = LC.gpu_input(hop, nF)
    T = x.shape[1]
    st = StftRoundTrip(S, T, F, hop)
    assert st.n_frames == nF
    for name in LC.GPU_CURVES:
        ref = LC.gpu_reference(hop, nF, name)
        y = _locked(st, x, LC.gpu_ratios(name, hop, nF))
        assert np.all(np.isfinite(y))
        for s in range(S):
            err, bnd = np.abs(y[s] - ref[s]).max(), LC.bound(hop, ref[s])
            print(f"PVLOCK one-shot hop{hop}-nF{nF}-{name} stream {s} ({LC.GPU_STREAMS[s]}): err {err:.3g} bound {bnd:.3g} err/bound {err / bnd:.3f}")
            assert err <= bnd, (name, s, err, bnd)
        covered = (nF - 1) * hop + F
        assert np.all(y[:, covered:] == 0) and y[:, covered:].shape[1] == hop - 1       # samples no frame covers
    st.close()


def test_the_python_entry_builds_the_same_tables():
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios
    hop, nF = 256, 7
    x = LC.gpu_input(hop, nF)
    st = StftRoundTrip(S, x.shape[1], F, hop)
    semis = np.random.default_rng(5).uniform(-12.0, 12.0, (S, nF))
    want = _locked(st, x, semitones_to_ratios(semis))
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    st.pitch_shift_locked(d_in, d_out, semitones=semis)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)
    st.pitch_shift_locked(d_in, d_out, semitones=semis[0])                            # one curve for every stream
    torch.cuda.synchronize()
    st.close()
    assert np.array_equal(d_out.cpu().numpy()[0], want[0])


# ---- 2. identity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", LC.GPU_HOPS)
def test_ratio_one_is_the_round_trip(hop):
    """r = 1 everywhere: the stage is the identity.  Against vp_stft_roundtrip (double precision) on the same handle within the bound, and
    against the NumPy round trip without a stage; the count of bit-equal samples is recorded (the rotation multiplies by the polynomial's
    cos 0, one unit in the last place above 1, so equality to the bit is not promised)."""
    from vocoderproject_amd import StftRoundTrip
    nF = 7
    x = LC.gpu_input(hop, nF)
    st = StftRoundTrip(S, x.shape[1], F, hop)
    y = _locked(st, x, np.ones((S, nF)))
    d_in = _dev(x, np.float32)
    d_rt = torch.full_like(d_in, float("nan"))
    st(d_in, d_rt)
    torch.cuda.synchronize()
    st.close()
    rt = d_rt.cpu().numpy()
    print(f"PVLOCK identity hop{hop}: {int((y == rt).sum())} of {y.size} samples bit-equal to vp_stft_roundtrip, max diff {np.abs(y - rt).max():.3g}")
    for s in range(S):
        ref = stft_reference.stft_roundtrip(x[s], F, hop)
        bnd = LC.bound(hop, ref)
        assert np.abs(y[s] - rt[s]).max() <= bnd and np.abs(y[s] - ref).max() <= bnd, (s, np.abs(y[s] - rt[s]).max(), bnd)


# ---- 3. streaming equals one-shot, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", LC.STREAM_BLOCKS)
@pytest.mark.parametrize("hop", LC.GPU_HOPS)
def test_streaming_locked_is_bit_identical_to_the_one_shot(hop, N):
    from vocoderproject_amd import PhaseVocoderStream
    x, tab = LC.stream_input(hop, N), LC.stream_ratios(hop, N)
    nb, T = tab.shape[0], x.shape[1]
    per_frame = LC.per_frame(tab, N, hop, T)
    y1 = _one_shot(x, per_frame, hop)
    ps = PhaseVocoderStream(S, N, hop=hop)
    n0 = ps.debug_alloc_count()
    d_out = _stream_locked(ps, _blocks(x, N), _dev(tab, np.float64), pv_cases.call_spans(nb, LC.STREAM_CALLS))
    torch.cuda.synchronize()
    assert ps.debug_alloc_count() == n0 and n0 > 0
    L = ps.latency
    ps.close()
    y2 = _rows(d_out)
    n = min(per_frame.shape[1] * hop, T - L)                                         # finished one-shot samples that the stream has emitted
    assert n > 2 * F and np.all(y2[:, :L] == 0) and np.all(np.isfinite(y2))
    for s in range(S):
        assert np.array_equal(y2[s, L:L + n], y1[s, :n]), (s, np.abs(y2[s, L:L + n] - y1[s, :n]).max())


@pytest.mark.parametrize("hop,N", [(64, 17), (128, 1000), (256, 256), (512, 64), (256, 4096)])
def test_grouping_of_the_calls_changes_no_bit(hop, N):
    from vocoderproject_amd import PhaseVocoderStream
    x, tab = LC.stream_input(hop, N), LC.stream_ratios(hop, N)
    nb = tab.shape[0]
    d_in, d_tab = _blocks(x, N), _dev(tab, np.float64)
    outs = []
    for g in (1, 3, 16):
        ps = PhaseVocoderStream(S, N, hop=hop)
        outs.append(_rows(_stream_locked(ps, d_in, d_tab, pv_cases.call_spans(nb, (g,)))))
        ps.close()
    assert np.all(np.isfinite(outs[0])) and np.abs(outs[0]).max() > 0.05
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_streaming_locked_matches_numpy_block_by_block():
    """N = 100 at hop 128: blocks that end inside a round; the reference is driven block by block."""
    from vocoderproject_amd import PhaseVocoderStream
    hop, N = 128, 100
    nb = 62
    x = np.stack([LC.SIGNALS[s](N * nb, seed=hop + N) for s in LC.GPU_STREAMS])
    tab = LC.ratio_of(np.random.default_rng([hop, N, 37]).uniform(-13.0, 13.0, (nb, S)))
    ps = PhaseVocoderStream(S, N, hop=hop)
    y = _rows(_stream_locked(ps, _blocks(x, N), _dev(tab, np.float64), pv_cases.call_spans(nb, LC.STREAM_CALLS)))
    ps.close()
    for s in range(S):
        ref = LR.by_block(x[s], N, hop, tab[:, s])
        err, bnd = np.abs(y[s] - ref).max(), LC.bound(hop, ref)
        print(f"PVLOCK stream N{N}-hop{hop} stream {s} ({LC.GPU_STREAMS[s]}): err {err:.3g} bound {bnd:.3g} err/bound {err / bnd:.3f}")
        assert err <= bnd, (s, err, bnd)


# ---- 4. state -----------------------------------------------------------------------------------------------------------------------------------
def _schedule_input(N, nb, hop):
    x = np.stack([LC.SIGNALS[s](N * nb, seed=hop + 11) for s in LC.GPU_STREAMS])
    tab = LC.ratio_of(np.random.default_rng([hop, N, 38]).uniform(-12.0, 12.0, (nb, S)))
    return x, tab


@pytest.mark.parametrize("hop", [64, 256])
def test_a_reset_in_the_middle_of_a_round_restarts_that_stream_alone(hop):
    from vocoderproject_amd import PhaseVocoderStream
    N, nb, cut = 100, 60, 27                                                         # the reset lands before block 27: sample 2700
    x, tab = _schedule_input(N, nb, hop)
    assert ((cut * N - F) // hop + 1) % 4 != 0                                       # frames so far: not at a round's end
    d_in, d_tab = _blocks(x, N), _dev(tab, np.float64)
    a = PhaseVocoderStream(S, N, hop=hop)
    d_a = _stream_locked(a, d_in, d_tab, [cut])
    a.reset(2)
    _stream_locked(a, d_in, d_tab, [nb - cut], cut, d_a)
    ya = _rows(d_a)
    a.close()
    b = PhaseVocoderStream(S, N, hop=hop)                                            # never reset
    yb = _rows(_stream_locked(b, d_in, d_tab, [nb]))
    b.close()
    f = PhaseVocoderStream(S, N, hop=hop)                                            # a fresh handle from the cut on
    d_f = _stream_locked(f, d_in[cut:].contiguous(), d_tab[cut:].contiguous(), [nb - cut])
    yf = _rows(d_f)
    f.close()
    for s in range(S):
        if s == 2:
            assert np.array_equal(ya[s, :cut * N], yb[s, :cut * N]) and np.array_equal(ya[s, cut * N:], yf[s])
            assert not np.array_equal(ya[s, cut * N:], yb[s, cut * N:])
        else:
            assert np.array_equal(ya[s], yb[s]), s


def test_a_reset_between_kinds_gives_the_fresh_call_s_bits():
    """locked -> reset -> plain equals a fresh plain call; plain -> reset -> locked equals a fresh locked call."""
    from vocoderproject_amd import PhaseVocoderStream
    N, hop, nb, cut = 256, 256, 24, 9
    x, tab = _schedule_input(N, nb, hop)
    d_in, d_tab = _blocks(x, N), _dev(tab, np.float64)
    tail_in, tail_tab = d_in[cut:].contiguous(), d_tab[cut:].contiguous()

    def plain(ps, din, out):
        ps.process_device(din, out, n_blocks=din.shape[0])

    a = PhaseVocoderStream(S, N, hop=hop)
    a.set_semitones(5.0)
    _stream_locked(a, d_in, d_tab, [cut])
    a.reset()
    out_a = torch.full_like(tail_in, float("nan"))
    plain(a, tail_in, out_a)
    f = PhaseVocoderStream(S, N, hop=hop)
    f.set_semitones(5.0)
    out_f = torch.full_like(tail_in, float("nan"))
    plain(f, tail_in, out_f)
    torch.cuda.synchronize()
    assert np.array_equal(out_a.cpu().numpy(), out_f.cpu().numpy()) and np.all(np.isfinite(out_f.cpu().numpy()))
    a.close()
    f.close()

    b = PhaseVocoderStream(S, N, hop=hop)
    b.set_semitones(-3.0)
    head = torch.full_like(d_in[:cut], float("nan"))
    plain(b, d_in[:cut].contiguous(), head)
    b.reset()
    out_b = _stream_locked(b, tail_in, tail_tab, [nb - cut])
    g = PhaseVocoderStream(S, N, hop=hop)
    g.set_semitones(-3.0)
    out_g = _stream_locked(g, tail_in, tail_tab, [nb - cut])
    torch.cuda.synchronize()
    assert np.array_equal(out_b.cpu().numpy(), out_g.cpu().numpy()) and np.abs(out_g.cpu().numpy()).max() > 0.05
    b.close()
    g.close()


def test_kinds_alternating_without_resets_are_finite_and_grouping_changes_no_bit():
    """plain / curve / locked / formant calls on one handle, no reset: the two arrays of the record are shared, the output is defined."""
    from vocoderproject_amd import PhaseVocoderStream
    N, hop = 100, 128
    kinds = ["plain", "curve", "locked", "formant", "locked", "plain", "locked", "curve"]
    spans = [3, 5, 7, 2, 16, 4, 1, 6]
    nb = sum(spans)
    x, tab = _schedule_input(N, nb, hop)
    d_in, d_tab = _blocks(x, N), _dev(tab, np.float64)

    def drive(single):
        ps = PhaseVocoderStream(S, N, hop=hop)
        ps.set_semitones(4.0)
        d_out = torch.full_like(d_in, float("nan"))
        b0 = 0
        for k, kind in zip(spans, kinds):
            for lo, n in ([(b0, k)] if not single else [(b0 + j, 1) for j in range(k)]):
                kw = {}
                if kind != "plain":
                    kw["d_ratio"] = d_tab[lo:lo + n]
                if kind == "formant":
                    kw["formant_semitones"] = 0.0
                if kind == "locked":
                    kw["locked"] = True
                ps.process_device(d_in[lo:lo + n], d_out[lo:lo + n], n_blocks=n, **kw)
            b0 += k
        torch.cuda.synchronize()
        ps.close()
        return _rows(d_out)

    ya, yb = drive(False), drive(True)
    assert np.all(np.isfinite(ya)) and np.abs(ya).max() > 0.05
    assert np.array_equal(ya, yb)


def test_forty_pending_changes_in_front_of_a_locked_call():
    """More pending changes than a call's arguments carry (16): update launches in front of the locked call, which neither uses nor loses
    the intervals; the pending reset of stream 1 applies."""
    from vocoderproject_amd import PhaseVocoderStream
    S2, N, hop, nb = 40, 256, 256, 12
    x = pv_cases.harmonic_streams(S2, N * nb, seed=9)
    tab = LC.ratio_of(np.random.default_rng(39).uniform(-12.0, 12.0, (nb, S2)))
    d_in, d_tab = _blocks(x, N), _dev(tab, np.float64)
    a = PhaseVocoderStream(S2, N, hop=hop)
    d_a = _stream_locked(a, d_in, d_tab, [5])
    for s in range(S2):
        a.set_semitones(-12.0 + 0.6 * s, stream=s)
    a.reset(1)
    _stream_locked(a, d_in, d_tab, [nb - 5], 5, d_a)
    torch.cuda.synchronize()
    assert [a.semitones(s) for s in range(S2)] == [-12.0 + 0.6 * s for s in range(S2)]
    b = PhaseVocoderStream(S2, N, hop=hop)
    yb = _rows(_stream_locked(b, d_in, d_tab, [nb]))
    f = PhaseVocoderStream(S2, N, hop=hop)
    yf = _rows(_stream_locked(f, d_in[5:].contiguous(), d_tab[5:].contiguous(), [nb - 5]))
    ya = _rows(d_a)
    for s in range(S2):
        if s == 1:
            assert np.array_equal(ya[s, 5 * N:], yf[s])
        else:
            assert np.array_equal(ya[s], yb[s]), s
    # the intervals were stored: a plain call on a and on a handle that was only told them give the same bits after a reset
    a.reset()
    f.reset()
    for s in range(S2):
        f.set_semitones(-12.0 + 0.6 * s, stream=s)
    oa, of = torch.full_like(d_in[:4], float("nan")), torch.full_like(d_in[:4], float("nan"))
    a.process_device(d_in[:4].contiguous(), oa, n_blocks=4)
    f.process_device(d_in[:4].contiguous(), of, n_blocks=4)
    torch.cuda.synchronize()
    assert np.array_equal(oa.cpu().numpy(), of.cpu().numpy())
    for p in (a, b, f):
        p.close()


# ---- 5. independence and homogeneity -----------------------------------------------------------------------------------------------------------
def test_rows_are_independent_scaling_by_a_power_of_two_scales_the_bits_and_silence_is_zero():
    hop, nF = 128, 7
    x = LC.gpu_input(hop, nF)
    r = LC.gpu_ratios("steps", hop, nF)
    y = _one_shot(x, r, hop)
    perm = np.array([3, 0, 5, 1, 4, 2])
    assert np.array_equal(_one_shot(x[perm], r[perm], hop), y[perm])
    for e in (-6, 3):
        assert np.array_equal(_one_shot(x * np.float32(2.0 ** e), r, hop), y * np.float32(2.0 ** e)), e
    x0 = x.copy()
    x0[2] = 0.0
    y0 = _one_shot(x0, r, hop)
    assert np.all(y0[2] == 0) and np.array_equal(np.delete(y0, 2, 0), np.delete(y, 2, 0))


@pytest.mark.parametrize("hop", [64, 512])
def test_degenerate_inputs_stay_finite_and_bounded(hop):
    from vocoderproject_amd import PhaseVocoderStream
    nF = 9
    T = LC.length(nF, hop, 5)
    x = np.stack([pv_cases.degenerate(n, T) for n in LC.DEGENERATE])
    n = len(x)
    for name in ("steps", "outside"):
        r = np.stack([LC.curve(name, nF, hop, s) for s in range(n)])
        y = _one_shot(x, r, hop)
        assert np.all(np.isfinite(y)) and np.all(y[0] == 0)
        for s in range(n):                                                           # a translation and a rotation of the bins: no frame gains magnitude
            assert np.abs(y[s]).max() <= pv_cases.magnitude_ceiling(x[s], hop) + 1e-6, (name, s)
    N, nb = 100, 30
    xs = np.stack([pv_cases.degenerate(nm, N * nb) for nm in LC.DEGENERATE])
    tab = np.stack([LC.curve("steps", nb, hop, s) for s in range(n)]).T
    ps = PhaseVocoderStream(n, N, hop=hop)
    ys = _rows(_stream_locked(ps, _blocks(xs, N), _dev(tab, np.float64), pv_cases.call_spans(nb, LC.STREAM_CALLS)))
    ps.close()
    assert np.all(np.isfinite(ys)) and np.all(ys[0] == 0)


def test_three_hundred_streams():
    """More workgroups than compute units, one-shot and streaming; a sample of the streams against NumPy, the two kernels bit for bit."""
    from vocoderproject_amd import PhaseVocoderStream
    BIG, hop, N, nb = 300, 256, 256, 12
    T = N * nb
    x = pv_cases.harmonic_streams(BIG, T, seed=hop + 3)
    tab = np.stack([LC.curve("steps", nb, hop, s) for s in range(BIG)]).T             # [nb][BIG]
    per_frame = LC.per_frame(tab, N, hop, T)
    y1 = _one_shot(x, per_frame, hop)
    for s in (0, 1, 149, 255, 256, 299):
        ref = LR.locked_roundtrip(x[s], per_frame[s], F, hop)
        err, bnd = np.abs(y1[s] - ref).max(), LC.bound(hop, ref)
        print(f"PVLOCK big stream {s}: err {err:.3g} bound {bnd:.3g} err/bound {err / bnd:.3f}")
        assert err <= bnd, (s, err, bnd)
    ps = PhaseVocoderStream(BIG, N, hop=hop)
    y2 = _rows(_stream_locked(ps, _blocks(x, N), _dev(tab, np.float64), [5, 7]))
    L = ps.latency
    ps.close()
    n = min(per_frame.shape[1] * hop, T - L)
    assert np.array_equal(y2[:, L:L + n], y1[:, :n])


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_reported_before_the_device_is_touched():
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, VpError
    st2 = StftRoundTrip(2, 8192, 2048, 512)
    d = torch.zeros((2, 8192), dtype=torch.float32, device="cuda")
    o = torch.full_like(d, 7.0)
    r = torch.ones((2, st2.n_frames), dtype=torch.float64, device="cuda")
    rc = st2.L.vp_stft_pitch_shift_locked(st2.h, d.data_ptr(), o.data_ptr(), r.data_ptr(), _cur())
    assert rc == VP_ERR_GEOMETRY and b"2048-point frames are not built" in st2.L.vp_stft_last_error(st2.h)
    with pytest.raises(VpError) as e:
        st2.pitch_shift_locked(d, o, d_ratio=r)
    assert "2048-point" in str(e.value)
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    st2.close()
    st = StftRoundTrip(2, 8192, 1024, 256)
    L = st.L
    r = torch.ones((2, st.n_frames), dtype=torch.float64, device="cuda")
    i_, o_, r_ = d.data_ptr(), o.data_ptr(), r.data_ptr()
    assert L.vp_stft_pitch_shift_locked(None, i_, o_, r_, _cur()) == VP_ERR_INVALID_ARG
    for args in ((None, o_, r_), (i_, None, r_), (i_, o_, None)):
        assert L.vp_stft_pitch_shift_locked(st.h, *args, _cur()) == VP_ERR_INVALID_ARG
        assert b"locked: null" in L.vp_stft_last_error(st.h)
    st.close()
    ps = PhaseVocoderStream(2, 256)
    x = torch.zeros((2, 256), dtype=torch.float32, device="cuda")
    bo = torch.full_like(x, 7.0)
    br = torch.ones((1, 2), dtype=torch.float64, device="cuda")
    i_, o_, r_ = x.data_ptr(), bo.data_ptr(), br.data_ptr()
    assert L.vp_pv_process_blocks_locked_device(None, i_, o_, r_, 1, _cur()) == VP_ERR_INVALID_ARG
    for args in ((None, o_, r_, 1), (i_, None, r_, 1), (i_, o_, None, 1), (i_, o_, r_, 0), (i_, o_, r_, -3)):
        assert L.vp_pv_process_blocks_locked_device(ps.h, *args, _cur()) == VP_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((bo == 7.0).all())
    y = torch.full_like(x, 7.0)
    for kw in (dict(formant_semitones=0.0), dict(d_formant=torch.ones(2, dtype=torch.float64, device="cuda"))):
        with pytest.raises((VpError, ValueError)):
            ps.process_device(x, y, locked=True, **kw)
    with pytest.raises((VpError, ValueError)):
        ps.run(np.zeros((2, 512), np.float32), locked=True, formant_semitones=0.0)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    ps.close()


def test_forty_locked_calls_allocate_nothing():
    from vocoderproject_amd import PhaseVocoderStream
    N, hop, nb = 64, 128, 40
    x, tab = _schedule_input(N, nb, hop)
    ps = PhaseVocoderStream(S, N, hop=hop)
    n0 = ps.debug_alloc_count()
    d_in, d_tab = _blocks(x, N), _dev(tab, np.float64)
    y = _rows(_stream_locked(ps, d_in, d_tab, [1] * nb))
    assert ps.debug_alloc_count() == n0 and n0 > 0 and np.all(np.isfinite(y))
    ps.close()


# ---- 7. behaviour ---------------------------------------------------------------------------------------------------------------------------------
def test_a_tone_lands_on_the_shifted_frequency_and_keeps_more_of_its_level_than_the_plain_shift():
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios
    fs, hop, T = 44100.0, 256, 32768
    x = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(T) / fs)).astype(np.float32)[None].repeat(2, 0)
    st = StftRoundTrip(2, T, F, hop)
    d_in = _dev(x, np.float32)
    lk, pl = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    st.pitch_shift_locked(d_in, lk, semitones=np.full(st.n_frames, 7.0))
    st.pitch_shift(d_in, pl, 7.0)
    torch.cuda.synchronize()
    st.close()
    lk, pl = lk.cpu().numpy()[0], pl.cpu().numpy()[0]
    seg = lk[4096:4096 + 16384] * np.hanning(16384)
    spec = np.abs(np.fft.rfft(seg))
    k = int(np.argmax(spec))
    a, b, c = np.log(spec[k - 1:k + 2])
    peak = (k + 0.5 * (a - c) / (a - 2 * b + c)) * fs / 16384
    want = 440.0 * float(semitones_to_ratios(np.array([7.0]))[0])
    print(f"PVLOCK tone: peak {peak:.2f} Hz, wanted {want:.2f} Hz")
    assert abs(peak - want) < 3.0, (peak, want)
    _, amp_l = LC.ripple(lk)
    _, amp_p = LC.ripple(pl)
    print(f"PVLOCK tone: amplitude locked {amp_l:.3f}, plain {amp_p:.3f}, input 0.5")
    assert abs(amp_l - 0.5) < abs(amp_p - 0.5), (amp_l, amp_p)


def test_autotune_locked_is_the_tracker_then_the_locked_call():
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, StreamingPitchTracker
    fs, hop, T = 44100.0, 256, 16384
    x = np.stack([LC.voice(T, s, 140.0 + 23.0 * s, 8) for s in range(2)])
    st = StftRoundTrip(2, T, F, hop)
    d_in = _dev(x, np.float32)
    out, parts = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    period, ratio = st.autotune(d_in, out, fs, locked=True)
    p2, r2 = st.track_pitch(d_in, fs)
    st.pitch_shift_locked(d_in, parts, d_ratio=r2)
    torch.cuda.synchronize()
    st.close()
    assert torch.equal(period, p2) and torch.equal(ratio, r2) and np.array_equal(out.cpu().numpy(), parts.cpu().numpy())
    assert np.all(np.isfinite(out.cpu().numpy()))
    N, nb = 512, 32
    a, ta = PhaseVocoderStream(2, N, hop=hop), StreamingPitchTracker(2, N, fs)
    b, tb = PhaseVocoderStream(2, N, hop=hop), StreamingPitchTracker(2, N, fs)
    blk = _blocks(x, N)
    oa, ob = torch.full_like(blk, float("nan")), torch.full_like(blk, float("nan"))
    for b0 in range(0, nb, 8):
        pa, ra = a.autotune_device(ta, blk[b0:b0 + 8], oa[b0:b0 + 8], n_blocks=8, locked=True)
        pb, rb = tb.process_device(blk[b0:b0 + 8], n_blocks=8)
        b.process_device(blk[b0:b0 + 8], ob[b0:b0 + 8], n_blocks=8, d_ratio=rb, locked=True)
        assert torch.equal(ra, rb) and torch.equal(pa, pb)
    torch.cuda.synchronize()
    assert np.array_equal(oa.cpu().numpy(), ob.cpu().numpy()) and np.all(np.isfinite(oa.cpu().numpy()))
    for p in (a, b, ta, tb):
        p.close()
