"""The peak-locked phase-vocoder pitch shift with sub-bin region offsets on the GPU (include/vp_amd.h vp_stft_pitch_shift_locked_subbin,
vp_pv_process_blocks_locked_subbin_device; kernels vp_k_stft_pv_lockf and vp_k_pv_stream_lockf of csrc/vp_stft_lockf.inc): against the
NumPy definition tests/pv_lockf_reference.py on the items of tests/pv_lockf_cases.py (whose conditioning
tests/test_pv_lockf_reference_cpu.py gates), the identity at ratio 1, the streaming call bit-identical to the one-shot under every block
size and grouping, resets and changes of kind on one handle, independence of the streams, more workgroups than compute units, silence
and degenerate inputs, what the stage is for (a shifted tone keeps its level), argument errors, and the Python and C++ entries.  The
PVLOCKF lines (-s) are what profiles/pv_lockf_errors.txt is made of."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_lock_cases as LC  # noqa: E402
import pv_lockf_cases as FC  # noqa: E402
import pv_lockf_reference as FR  # noqa: E402

pytestmark = pytest.mark.gpu

S, F = len(LC.GPU_STREAMS), LC.F
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4              # include/vp_amd.h


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(st, x, ratio, entry="vp_stft_pitch_shift_locked_subbin"):
    """One one-shot call of `entry` on x [S][T] with a table of ratios; the output starts as NaN, so every sample must have been written."""
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    d_ratio = _dev(ratio, np.float64)
    rc = getattr(st.L, entry)(st.h, d_in.data_ptr(), d_out.data_ptr(), d_ratio.data_ptr(), _cur())
    torch.cuda.synchronize()
    assert rc == 0, (rc, st.L.vp_stft_last_error(st.h))
    return d_out.cpu().numpy()


def _one_shot(x, ratio, hop):
    from vocoderproject_amd import StftRoundTrip
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    y = _call(st, x, ratio)
    st.close()
    return y


def _blocks(x, N):
    n, T = x.shape
    return _dev(x.reshape(n, T // N, N).transpose(1, 0, 2), np.float32)


def _rows(d):
    nb, n, N = d.shape
    return d.cpu().numpy().transpose(1, 0, 2).reshape(n, nb * N)


def _stream(ps, d_in, d_tab, spans, b0=0, d_out=None):
    """Sub-bin calls of `spans` blocks each from block b0 on; returns the device output [n_blocks][S][N] (NaN where no call wrote)."""
    if d_out is None:
        d_out = torch.full_like(d_in, float("nan"))
    for k in spans:
        rc = ps.L.vp_pv_process_blocks_locked_subbin_device(ps.h, d_in[b0:b0 + k].data_ptr(), d_out[b0:b0 + k].data_ptr(), d_tab[b0:b0 + k].data_ptr(), k, _cur())
        assert rc == 0, rc
        b0 += k
    return d_out


# ---- 1. one-shot against NumPy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nF", LC.GPU_NF)
@pytest.mark.parametrize("hop", LC.GPU_HOPS)
def test_one_shot_matches_numpy(hop, nF):
    """Mixed content, every residue mod 4 of the last round, a tail of hop - 1 samples no frame covers, every admitted curve and stream."""
    from vocoderproject_amd import StftRoundTrip
    x = LC.gpu_input(hop, nF)
    T = x.shape[1]
    st = StftRoundTrip(S, T, F, hop)
    assert st.n_frames == nF
    for name in LC.GPU_CURVES:
        ref = FC.gpu_reference(hop, nF, name)
        y = _call(st, x, LC.gpu_ratios(name, hop, nF))
        assert np.all(np.isfinite(y))
        for s in FC.admitted(hop, nF, name):
            err, bnd = np.abs(y[s] - ref[s]).max(), FC.bound(hop, ref[s])
            print(f"PVLOCKF one-shot hop{hop}-nF{nF}-{name} stream {s} ({LC.GPU_STREAMS[s]}): err {err:.3g} bound {bnd:.3g} err/bound {err / bnd:.3f}")
            assert err <= bnd, (name, s, err, bnd)
        covered = (nF - 1) * hop + F
        assert np.all(y[:, covered:] == 0) and y[:, covered:].shape[1] == hop - 1       # samples no frame covers
    st.close()


# ---- 2. identity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", LC.GPU_HOPS)
def test_ratio_one_is_the_round_trip(hop):
    """r = 1 everywhere: D = 0, one tap of weight 1, the stage is the identity.  Against vp_stft_roundtrip (double precision) on the same
    handle within the gate; the number of samples bit-equal to vp_stft_pitch_shift_locked is recorded (equality is not promised)."""
    from vocoderproject_amd import StftRoundTrip
    nF = 7
    x = LC.gpu_input(hop, nF)
    st = StftRoundTrip(S, x.shape[1], F, hop)
    y = _call(st, x, np.ones((S, nF)))
    yi = _call(st, x, np.ones((S, nF)), "vp_stft_pitch_shift_locked")
    d_in = _dev(x, np.float32)
    d_rt = torch.full_like(d_in, float("nan"))
    st(d_in, d_rt)
    torch.cuda.synchronize()
    st.close()
    rt = d_rt.cpu().numpy()
    print(f"PVLOCKF identity hop{hop}: {int((y == yi).sum())} of {y.size} samples bit-equal to vp_stft_pitch_shift_locked, {int((y == rt).sum())} to "
          f"vp_stft_roundtrip, max diff {np.abs(y - rt).max():.3g}")
    for s in range(S):
        bnd = FC.bound(hop, rt[s])
        assert np.abs(y[s] - rt[s]).max() <= bnd, (s, np.abs(y[s] - rt[s]).max(), bnd)


# ---- 3. streaming equals one-shot, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", FC.STREAM_BLOCKS)
@pytest.mark.parametrize("hop", LC.GPU_HOPS)
def test_streaming_is_bit_identical_to_the_one_shot(hop, N):
    from vocoderproject_amd import PhaseVocoderStream
    x, tab = LC.stream_input(hop, N), LC.stream_ratios(hop, N)
    nb, T = tab.shape[0], x.shape[1]
    per_frame = LC.per_frame(tab, N, hop, T)
    y1 = _one_shot(x, per_frame, hop)
    ps = PhaseVocoderStream(S, N, hop=hop)
    n0 = ps.debug_alloc_count()
    d_out = _stream(ps, _blocks(x, N), _dev(tab, np.float64), pv_cases.call_spans(nb, FC.STREAM_CALLS))
    torch.cuda.synchronize()
    assert ps.debug_alloc_count() == n0 and n0 > 0
    L = ps.latency
    ps.close()
    y2 = _rows(d_out)
    n = min(per_frame.shape[1] * hop, T - L)                                         # finished one-shot samples that the stream has emitted
    assert n > 2 * F and np.all(y2[:, :L] == 0) and np.all(np.isfinite(y2))
    for s in range(S):
        assert np.array_equal(y2[s, L:L + n], y1[s, :n]), (s, np.abs(y2[s, L:L + n] - y1[s, :n]).max())


@pytest.mark.parametrize("hop,N", [(64, 17), (128, 1000), (256, 256), (512, 64), (256, 1024)])
def test_grouping_of_the_calls_changes_no_bit(hop, N):
    from vocoderproject_amd import PhaseVocoderStream
    x, tab = LC.stream_input(hop, N), LC.stream_ratios(hop, N)
    nb = tab.shape[0]
    d_in, d_tab = _blocks(x, N), _dev(tab, np.float64)
    outs = []
    for g in FC.STREAM_CALLS:
        ps = PhaseVocoderStream(S, N, hop=hop)
        outs.append(_rows(_stream(ps, d_in, d_tab, pv_cases.call_spans(nb, (g,)))))
        ps.close()
    assert np.all(np.isfinite(outs[0])) and np.abs(outs[0]).max() > 0.05
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ---- 4. state -----------------------------------------------------------------------------------------------------------------------------------
def _schedule_input(N, nb, hop):
    x = np.stack([LC.SIGNALS[s](N * nb, seed=hop + 11) for s in LC.GPU_STREAMS])
    tab = LC.ratio_of(np.random.default_rng([hop, N, 38]).uniform(-12.0, 12.0, (nb, S)))
    return x, tab


@pytest.mark.parametrize("hop", [64, 256])
def test_a_reset_restarts_one_stream_alone_and_a_reset_of_all_gives_a_fresh_handle_s_bits(hop):
    from vocoderproject_amd import PhaseVocoderStream
    N, nb, cut = 100, 60, 27                                                         # the reset lands before block 27: sample 2700
    x, tab = _schedule_input(N, nb, hop)
    assert ((cut * N - F) // hop + 1) % 4 != 0                                       # frames so far: not at a round's end
    d_in, d_tab = _blocks(x, N), _dev(tab, np.float64)
    a = PhaseVocoderStream(S, N, hop=hop)
    d_a = _stream(a, d_in, d_tab, [cut])
    a.reset(2)
    _stream(a, d_in, d_tab, [nb - cut], cut, d_a)
    ya = _rows(d_a)
    b = PhaseVocoderStream(S, N, hop=hop)                                            # never reset
    yb = _rows(_stream(b, d_in, d_tab, [nb]))
    f = PhaseVocoderStream(S, N, hop=hop)                                            # a fresh handle from the cut on
    yf = _rows(_stream(f, d_in[cut:].contiguous(), d_tab[cut:].contiguous(), [nb - cut]))
    for s in range(S):
        if s == 2:
            assert np.array_equal(ya[s, :cut * N], yb[s, :cut * N]) and np.array_equal(ya[s, cut * N:], yf[s])
            assert not np.array_equal(ya[s, cut * N:], yb[s, cut * N:])
        else:
            assert np.array_equal(ya[s], yb[s]), s
    b.reset()                                                                        # every stream: the handle is as good as new
    assert np.array_equal(_rows(_stream(b, d_in[cut:].contiguous(), d_tab[cut:].contiguous(), [nb - cut])), yf)
    for p in (a, b, f):
        p.close()


def test_a_subbin_call_between_the_other_kinds_is_finite_and_allocates_nothing():
    """plain / curve / locked / formant / sub-bin calls on one handle, no reset: the two arrays of the record are shared, the output is
    defined and finite, single-block calls give the same bits, and the handle's allocation count does not move."""
    from vocoderproject_amd import PhaseVocoderStream
    N, hop = 100, 128
    kinds = ["plain", "subbin", "curve", "subbin", "locked", "subbin", "formant", "subbin", "plain"]
    spans = [3, 5, 7, 2, 16, 4, 1, 6, 3]
    nb = sum(spans)
    x, tab = _schedule_input(N, nb, hop)
    d_in, d_tab = _blocks(x, N), _dev(tab, np.float64)

    def drive(single):
        ps = PhaseVocoderStream(S, N, hop=hop)
        ps.set_semitones(4.0)
        n0 = ps.debug_alloc_count()
        ps.process_device(d_in[:1], torch.empty_like(d_in[:1]), n_blocks=1, d_ratio=d_tab[:1], formant_semitones=0.0)   # (the formant table is made once)
        ps.reset()
        n1 = ps.debug_alloc_count()
        d_out = torch.full_like(d_in, float("nan"))
        b0 = 0
        for k, kind in zip(spans, kinds):
            for lo, n in ([(b0, k)] if not single else [(b0 + j, 1) for j in range(k)]):
                kw = {}
                if kind != "plain":
                    kw["d_ratio"] = d_tab[lo:lo + n]
                if kind == "formant":
                    kw["formant_semitones"] = 0.0
                if kind in ("locked", "subbin"):
                    kw["locked"] = True
                if kind == "subbin":
                    kw["subbin"] = True
                ps.process_device(d_in[lo:lo + n], d_out[lo:lo + n], n_blocks=n, **kw)
            b0 += k
        torch.cuda.synchronize()
        assert ps.debug_alloc_count() == n1 and n1 >= n0 > 0
        ps.close()
        return _rows(d_out)

    ya, yb = drive(False), drive(True)
    assert np.all(np.isfinite(ya)) and np.abs(ya).max() > 0.05
    assert np.array_equal(ya, yb)


# ---- 5. independence ---------------------------------------------------------------------------------------------------------------------------
def test_a_stream_alone_equals_the_stream_in_the_batch():
    hop, nF = 128, 7
    x = LC.gpu_input(hop, nF)
    r = LC.gpu_ratios("steps", hop, nF)
    y = _one_shot(x, r, hop)
    for s in range(S):
        assert np.array_equal(_one_shot(x[s:s + 1], r[s:s + 1], hop)[0], y[s]), s
    perm = np.array([3, 0, 5, 1, 4, 2])
    assert np.array_equal(_one_shot(x[perm], r[perm], hop), y[perm])
    x0 = x.copy()
    x0[2] = 0.0
    y0 = _one_shot(x0, r, hop)
    assert np.all(y0[2] == 0) and np.array_equal(np.delete(y0, 2, 0), np.delete(y, 2, 0))


def test_three_hundred_streams_of_two_frames():
    """More workgroups than compute units, one-shot and streaming: a sample of the streams alone equals the stream in the batch, the two
    kernels agree bit for bit."""
    from vocoderproject_amd import PhaseVocoderStream
    BIG, hop, nF = 300, 256, 2
    T = LC.length(nF, hop)
    x = pv_cases.harmonic_streams(BIG, T, seed=hop + 3)
    r = np.stack([LC.curve("steps", nF, hop, s) for s in range(BIG)])
    y = _one_shot(x, r, hop)
    assert np.all(np.isfinite(y)) and np.all(np.abs(y).max(axis=1) > 1e-3)
    pick = [0, 1, 149, 255, 256, 299]
    assert np.array_equal(_one_shot(x[pick], r[pick], hop), y[pick])
    N, nb = 256, 9                                                                    # the same two frames, streamed: blocks 0 .. 4 hold them
    xs = np.zeros((BIG, N * nb), np.float32)
    xs[:, :T] = x
    tab = np.ones((nb, BIG))
    tab[3], tab[4] = r[:, 0], r[:, 1]                                                 # frame f's last sample arrives in block 3 + f
    ps = PhaseVocoderStream(BIG, N, hop=hop)
    y2 = _rows(_stream(ps, _blocks(xs, N), _dev(tab, np.float64), [4, 5]))
    L = ps.latency
    ps.close()
    assert L == F - N and np.array_equal(y2[:, L:L + nF * hop], y[:, :nF * hop])


# ---- 6. silence and degenerate inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [64, 512])
def test_silence_is_zero_and_degenerate_inputs_stay_finite(hop):
    from vocoderproject_amd import PhaseVocoderStream
    nF = 9
    T = LC.length(nF, hop, 5)
    x = np.stack([pv_cases.degenerate(n, T) for n in LC.DEGENERATE])
    n = len(x)
    assert LC.DEGENERATE == ("silence", "dc", "nyquist", "impulses")
    for name in ("steps", "outside"):
        r = np.stack([LC.curve(name, nF, hop, s) for s in range(n)])
        y = _one_shot(x, r, hop)
        assert np.all(np.isfinite(y)) and np.all(y[0] == 0)
    N, nb = 100, 30
    xs = np.stack([pv_cases.degenerate(nm, N * nb) for nm in LC.DEGENERATE])
    tab = np.stack([LC.curve("steps", nb, hop, s) for s in range(n)]).T
    ps = PhaseVocoderStream(n, N, hop=hop)
    ys = _rows(_stream(ps, _blocks(xs, N), _dev(tab, np.float64), pv_cases.call_spans(nb, FC.STREAM_CALLS)))
    ps.close()
    assert np.all(np.isfinite(ys)) and np.all(ys[0] == 0)
    # every peak of every sounding frame leaves past N: nothing is synthesised; the next call on the data at r = 1 is the round trip
    xg, tr = FC.shifted_out(hop, 7), []
    FR.lockf_roundtrip(xg, 2.0, F, hop, trace=tr)
    assert any(t["gone"] for t in tr) and all(t["gone"] or t["silent"] for t in tr)
    yg = _one_shot(xg[None], np.full((1, 7), 2.0), hop)
    assert np.all(yg == 0)
    y1 = _one_shot(xg[None], np.ones((1, 7)), hop)
    assert np.all(np.isfinite(y1)) and np.abs(y1).max() > 1e-3


# ---- 7. what it is for ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semitones", FC.PURPOSE_SEMITONES)
def test_a_shifted_tone_keeps_its_level(semitones):
    """The 227.3 Hz tone of the quality table, one stream: the GPU level is within 0.005 of the NumPy definition's and above the integer
    kernel's on the same handle by at least half the difference the two definitions show."""
    from vocoderproject_amd import StftRoundTrip
    hop = 256
    x = LC.quality_tone(FC.PURPOSE_TONE)[None]
    st = StftRoundTrip(1, x.shape[1], F, hop)
    r = np.full((1, st.n_frames), float(LC.ratio_of(semitones)))
    yf = _call(st, x, r)
    yi = _call(st, x, r, "vp_stft_pitch_shift_locked")
    st.close()
    lf, li = LC.ripple(yf[0])[1], LC.ripple(yi[0])[1]
    di, df = FC.purpose_levels(semitones)
    print(f"PVLOCKF level {FC.PURPOSE_TONE} Hz {semitones:+g} st: GPU sub-bin {lf:.4f} integer {li:.4f}; NumPy sub-bin {df:.4f} integer {di:.4f}; input 0.5")
    assert abs(lf - df) <= FC.LEVEL_TOL, (lf, df)
    assert df > di and lf - li >= 0.5 * (df - di), (lf, li, df, di)


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device_and_leave_the_handle_as_new():
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, VpError
    st2 = StftRoundTrip(2, 8192, 2048, 512)
    d = torch.zeros((2, 8192), dtype=torch.float32, device="cuda")
    o = torch.full_like(d, 7.0)
    r = torch.ones((2, st2.n_frames), dtype=torch.float64, device="cuda")
    L = st2.L
    rc = L.vp_stft_pitch_shift_locked_subbin(st2.h, d.data_ptr(), o.data_ptr(), r.data_ptr(), _cur())
    assert rc == VP_ERR_GEOMETRY
    assert L.vp_stft_last_error(st2.h) == b"locked subbin: 2048-point frames are not built (the peak-locked stage exists for 1024-point frames only)"
    assert L.vp_stft_pitch_shift_locked_subbin(st2.h, None, o.data_ptr(), r.data_ptr(), _cur()) == VP_ERR_INVALID_ARG      # pointers before geometry
    with pytest.raises(VpError) as e:
        st2.pitch_shift_locked(d, o, d_ratio=r, subbin=True)
    assert "2048-point" in str(e.value)
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    st2.close()

    hop, nF = 256, 5
    x = LC.gpu_input(hop, nF)
    ratio = LC.gpu_ratios("steps", hop, nF)
    st = StftRoundTrip(S, x.shape[1], F, hop)
    d_in, d_r = _dev(x, np.float32), _dev(ratio, np.float64)
    o = torch.full_like(d_in, 7.0)
    i_, o_, r_ = d_in.data_ptr(), o.data_ptr(), d_r.data_ptr()
    assert L.vp_stft_pitch_shift_locked_subbin(None, i_, o_, r_, _cur()) == VP_ERR_INVALID_ARG
    for args in ((None, o_, r_), (i_, None, r_), (i_, o_, None)):
        assert L.vp_stft_pitch_shift_locked_subbin(st.h, *args, _cur()) == VP_ERR_INVALID_ARG
        assert L.vp_stft_last_error(st.h) == b"locked subbin: null input, output or ratio table"
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    got = _call(st, x, ratio)                                                         # the valid call behind the refused ones
    st.close()
    assert np.array_equal(got, _one_shot(x, ratio, hop))                              # ... equals a fresh handle's

    N, nb = 256, 8
    xs, tab = _schedule_input(N, nb, hop)
    ps = PhaseVocoderStream(S, N, hop=hop)
    d_b, d_t = _blocks(xs, N), _dev(tab, np.float64)
    bo = torch.full_like(d_b, 7.0)
    i_, o_, r_ = d_b.data_ptr(), bo.data_ptr(), d_t.data_ptr()
    assert L.vp_pv_process_blocks_locked_subbin_device(None, i_, o_, r_, 1, _cur()) == VP_ERR_INVALID_ARG
    for args in ((None, o_, r_, 1), (i_, None, r_, 1), (i_, o_, None, 1), (i_, o_, r_, 0), (i_, o_, r_, -3)):
        assert L.vp_pv_process_blocks_locked_subbin_device(ps.h, *args, _cur()) == VP_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((bo == 7.0).all())
    y = torch.full_like(d_b, 7.0)
    with pytest.raises(ValueError):
        ps.process_device(d_b, y, n_blocks=nb, d_ratio=d_t, subbin=True)              # subbin without locked
    with pytest.raises(ValueError):
        ps.process_device(d_b, y, n_blocks=nb, d_ratio=d_t, locked=True, subbin=True, formant_semitones=0.0)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    got = _rows(_stream(ps, d_b, d_t, [nb]))
    ps.close()
    fresh = PhaseVocoderStream(S, N, hop=hop)
    want = _rows(_stream(fresh, d_b, d_t, [nb]))
    fresh.close()
    assert np.array_equal(got, want) and np.abs(want).max() > 0.05


# ---- 9. the Python and C++ entries ------------------------------------------------------------------------------------------------------------------
def test_the_python_entries_build_the_same_tables_as_the_raw_call():
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, semitones_to_ratios
    hop, nF = 256, 7
    x = LC.gpu_input(hop, nF)
    st = StftRoundTrip(S, x.shape[1], F, hop)
    semis = np.random.default_rng(5).uniform(-12.0, 12.0, (S, nF))
    want = _call(st, x, semitones_to_ratios(semis))
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    st.pitch_shift_locked(d_in, d_out, semitones=semis, subbin=True)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)
    st.pitch_shift_locked(d_in, d_out, semitones=semis)                               # without the keyword: the integer call
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), _call(st, x, semitones_to_ratios(semis), "vp_stft_pitch_shift_locked"))
    st.close()
    N, nb = 256, 10
    xs, _ = _schedule_input(N, nb, hop)
    semi_b = np.random.default_rng(6).uniform(-12.0, 12.0, (nb, S))
    a = PhaseVocoderStream(S, N, hop=hop)
    want = _rows(_stream(a, _blocks(xs, N), _dev(semitones_to_ratios(semi_b), np.float64), [4, 6]))
    a.close()
    b = PhaseVocoderStream(S, N, hop=hop)
    d_b = _blocks(xs, N)
    d_o = torch.full_like(d_b, float("nan"))
    b.process_device(d_b[:4], d_o[:4], n_blocks=4, semitones_per_block=semi_b[:4], locked=True, subbin=True)
    b.process_device(d_b[4:], d_o[4:], n_blocks=6, semitones_per_block=semi_b[4:], locked=True, subbin=True)
    torch.cuda.synchronize()
    assert np.array_equal(_rows(d_o), want)
    b.reset()
    y = b.run(xs, blocks_per_call=4, curve=semi_b, locked=True, subbin=True)          # run: aligned with its input, the latency off
    L = b.latency
    b.close()
    assert np.array_equal(y[:, :N * nb - L], want[:, L:])


def test_autotune_with_subbin_is_the_tracker_then_the_subbin_call():
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, StreamingPitchTracker
    fs, hop, T = 44100.0, 256, 16384
    x = np.stack([LC.voice(T, s, 140.0 + 23.0 * s, 8) for s in range(2)])
    st = StftRoundTrip(2, T, F, hop)
    d_in = _dev(x, np.float32)
    out, parts = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    period, ratio = st.autotune(d_in, out, fs, locked=True, subbin=True)
    p2, r2 = st.track_pitch(d_in, fs)
    st.pitch_shift_locked(d_in, parts, d_ratio=r2, subbin=True)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        st.autotune(d_in, out, fs, subbin=True)
    st.close()
    assert torch.equal(period, p2) and torch.equal(ratio, r2) and np.array_equal(out.cpu().numpy(), parts.cpu().numpy())
    assert np.all(np.isfinite(out.cpu().numpy()))
    N, nb = 512, 32
    a, ta = PhaseVocoderStream(2, N, hop=hop), StreamingPitchTracker(2, N, fs)
    b, tb = PhaseVocoderStream(2, N, hop=hop), StreamingPitchTracker(2, N, fs)
    blk = _blocks(x, N)
    oa, ob = torch.full_like(blk, float("nan")), torch.full_like(blk, float("nan"))
    for b0 in range(0, nb, 8):
        pa, ra = a.autotune_device(ta, blk[b0:b0 + 8], oa[b0:b0 + 8], n_blocks=8, locked=True, subbin=True)
        pb, rb = tb.process_device(blk[b0:b0 + 8], n_blocks=8)
        b.process_device(blk[b0:b0 + 8], ob[b0:b0 + 8], n_blocks=8, d_ratio=rb, locked=True, subbin=True)
        assert torch.equal(ra, rb) and torch.equal(pa, pb)
    torch.cuda.synchronize()
    assert np.array_equal(oa.cpu().numpy(), ob.cpu().numpy()) and np.all(np.isfinite(oa.cpu().numpy()))
    for p in (a, b, ta, tb):
        p.close()


def test_the_cpp_entry_gives_the_raw_call_s_bits(tmp_path):
    """vp::StreamingPitchShifter::processBlocksLockedSubbin on one handle, vp_pv_process_blocks_locked_subbin_device on another, the same
    blocks and table: the same bytes, and not the integer call's."""
    import shutil
    import subprocess
    from vocoderproject_amd import build
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no g++ / HIP headers")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = build.build()
    src = tmp_path / "t.cpp"
    src.write_text(r"""
#include <hip/hip_runtime_api.h>
#include "vp_amd.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#define HIPOK(x) do { if ((x) != hipSuccess) { std::printf("HIP error at %d\n", __LINE__); return 9; } } while (0)
int main() {
    const int S = 3, N = 256, B = 12;
    std::vector<float> x((size_t)B * S * N);
    std::vector<double> tab((size_t)B * S);
    for (int b = 0; b < B; b++) for (int s = 0; s < S; s++) {
        tab[(size_t)b * S + s] = std::pow(2.0, (double)((b * 5 + s * 3) % 25 - 12) / 12.0);
        for (int i = 0; i < N; i++) {
            const double t = (double)(b * N + i) / 44100.0, f0 = 131.0 + 29.0 * s;
            double v = 0.0;
            for (int h = 1; h <= 6; h++) v += std::sin(2.0 * M_PI * h * f0 * t) / h;
            x[((size_t)b * S + s) * N + i] = (float)(0.25 * v);
        }
    }
    try {
        float *dIn, *dOut;
        double *dTab;
        HIPOK(hipSetDevice(0));
        HIPOK(hipMalloc((void **)&dIn, x.size() * sizeof(float)));
        HIPOK(hipMalloc((void **)&dOut, x.size() * sizeof(float)));
        HIPOK(hipMalloc((void **)&dTab, tab.size() * sizeof(double)));
        HIPOK(hipMemcpy(dIn, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(dTab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
        std::vector<float> viaCpp(x.size()), viaC(x.size()), integer(x.size());
        {
            vp::StreamingPitchShifter p(0, S, N);
            p.processBlocksLockedSubbin(dIn, dOut, dTab, 5);
            p.processBlocksLockedSubbin(dIn + (size_t)5 * S * N, dOut + (size_t)5 * S * N, dTab + 5 * S, B - 5);
            HIPOK(hipDeviceSynchronize());
            HIPOK(hipMemcpy(viaCpp.data(), dOut, x.size() * sizeof(float), hipMemcpyDeviceToHost));
            try { p.processBlocksLockedSubbin(dIn, dOut, nullptr, 1); return 3; } catch (const vp::Error &e) { if (e.code != VP_ERR_INVALID_ARG) return 4; }
        }
        {
            vp_pv *q = nullptr;
            if (vp_pv_create(0, S, N, 1024, 256, &q) != VP_OK) return 2;
            if (vp_pv_process_blocks_locked_subbin_device(q, dIn, dOut, dTab, B, nullptr) != VP_OK) return 2;
            HIPOK(hipDeviceSynchronize());
            HIPOK(hipMemcpy(viaC.data(), dOut, x.size() * sizeof(float), hipMemcpyDeviceToHost));
            vp_pv_destroy(q);
        }
        {
            vp::StreamingPitchShifter p(0, S, N);
            p.processBlocksLocked(dIn, dOut, dTab, B);
            HIPOK(hipDeviceSynchronize());
            HIPOK(hipMemcpy(integer.data(), dOut, x.size() * sizeof(float), hipMemcpyDeviceToHost));
        }
        HIPOK(hipFree(dIn)); HIPOK(hipFree(dOut)); HIPOK(hipFree(dTab));
        double e = 0.0;
        for (float v : viaC) { if (!std::isfinite(v)) return 7; e += (double)v * v; }
        if (!(e > 0.0)) return 6;
        if (std::memcmp(viaCpp.data(), viaC.data(), viaC.size() * sizeof(float)) != 0) return 5;
        if (std::memcmp(integer.data(), viaC.data(), viaC.size() * sizeof(float)) == 0) return 8;
        std::printf("processBlocksLockedSubbin == vp_pv_process_blocks_locked_subbin_device\n");
        return 0;
    } catch (const vp::Error &e) {
        std::printf("vp::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
""")
    exe = tmp_path / "t"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(root, "include"),
                           str(src), "-o", str(exe), lib, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.dirname(lib) + ":/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
