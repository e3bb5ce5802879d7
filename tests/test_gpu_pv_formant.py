"""The formant-preserving phase-vocoder pitch shift on the GPU (include/vp_amd.h vp_stft_pitch_shift_formant,
vp_pv_process_blocks_formant_device and the two autotune entries; kernels vp_k_stft_pv_formant and vp_k_pv_stream_formant of
csrc/vp_stft_formant.inc): against the NumPy definition on every case of tests/pv_formant_cases.py (whose conditioning
tests/test_pv_formant_reference_cpu.py gates), the curve kernels' bits where the formant ratio equals the pitch ratio, the streaming call
bit-identical to the one-shot, call grouping, formant / curve / plain calls mixed on one handle, silence and DC, the clamps, argument
errors, the neighbours on the handle, no allocation, more workgroups than compute units, and autotune against its two parts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_formant_cases as FC  # noqa: E402

pytestmark = pytest.mark.gpu

S, F = FC.N_STREAMS, FC.F
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4              # include/vp_amd.h


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _formant(st, x, ratio, phi=None, nc=32):
    """One vp_stft_pitch_shift_formant call on x [S][T] with ratio tables (phi None: the NULL table); the output starts as NaN, so every
    sample must have been written."""
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    d_ratio = _dev(ratio, np.float64)
    d_phi = _dev(phi, np.float64) if phi is not None else None
    rc = st.L.vp_stft_pitch_shift_formant(st.h, d_in.data_ptr(), d_out.data_ptr(), d_ratio.data_ptr(), d_phi.data_ptr() if d_phi is not None else None,
                                          int(nc), _cur())
    torch.cuda.synchronize()
    assert rc == 0, (rc, st.L.vp_stft_last_error(st.h))
    return d_out.cpu().numpy()


def _curve(st, x, ratio):
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    st.pitch_shift_curve(d_in, d_out, d_ratio=_dev(ratio, np.float64))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _blocks(x, N):
    n, T = x.shape
    return _dev(x.reshape(n, T // N, N).transpose(1, 0, 2), np.float32)


def _rows(d):
    nb, n, N = d.shape
    return d.cpu().numpy().transpose(1, 0, 2).reshape(n, nb * N)


# ---- 1. one-shot against NumPy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.ALL_CASES, ids=FC.case_id)
def test_one_shot_formant_matches_numpy(c):
    from vocoderproject_amd import StftRoundTrip
    x, ref = FC.case_input(c), FC.reference(c)
    T = FC.length(c)
    st = StftRoundTrip(S, T, F, c.hop)
    assert st.n_frames == c.nF
    y = _formant(st, x, FC.ratios_of(c), FC.FORMANT_RATIOS, c.nc)
    st.close()
    assert np.all(np.isfinite(y))
    for s in range(S):
        err, bnd = np.abs(y[s] - ref[s]).max(), FC.bound(c, ref[s])
        print(f"FORMANT {FC.case_id(c)} stream {s}: err {err:.3g} bound {bnd:.3g}")
        assert err <= bnd, (s, err, bnd)
    covered = (c.nF - 1) * c.hop + F
    assert np.all(y[:, covered:] == 0) and y[:, covered:].shape[1] == c.extra        # samples no frame covers


def test_the_python_entry_builds_the_same_tables():
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios
    c = FC.FormantCase(256, 19, 3, "glide", 32)
    x = FC.case_input(c)
    st = StftRoundTrip(S, FC.length(c), F, c.hop)
    d_in = _dev(x, np.float32)
    semis = np.array([3.0, -7.0, 12.0, -12.0, 0.5])
    fsemi = np.array([0.0, 0.0, -5.0, 12.0, -12.0])
    nF = st.n_frames
    want = _formant(st, x, np.repeat(semitones_to_ratios(semis)[:, None], nF, axis=1), semitones_to_ratios(fsemi), 16)
    d_out = torch.full_like(d_in, float("nan"))
    st.pitch_shift_formant(d_in, d_out, semitones=semis, formant_semitones=fsemi, lifter=16)          # one interval per stream: a constant table
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)
    # a scalar interval, the default formant interval (0: preservation) and lifter (32); the NULL table is ratio 1
    want = _formant(st, x, np.full((S, nF), semitones_to_ratios(np.array(7.0))), None, 32)
    st.pitch_shift_formant(d_in, d_out, semitones=7.0)
    torch.cuda.synchronize()
    st.close()
    assert np.array_equal(d_out.cpu().numpy(), want)


# ---- 2. a formant ratio equal to the pitch ratio is the plain pitch shift, bit for bit ----------------------------------------------------
@pytest.mark.parametrize("hop", [256, 512])
def test_formant_following_the_pitch_is_bit_identical_to_pitch_shift(hop):
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios
    nF = 19
    T = F + (nF - 1) * hop + 3
    x = pv_cases.mixed_streams(T, seed=hop + 5)
    st = StftRoundTrip(S, T, F, hop)
    r = semitones_to_ratios(np.array(pv_cases.SEMITONES))
    y = _formant(st, x, np.repeat(r[:, None], nF, axis=1), r, 32)
    kept = _formant(st, x, np.repeat(r[:, None], nF, axis=1), None, 32)
    d_in = _dev(x, np.float32)
    d_out = torch.empty_like(d_in)
    for s, v in enumerate(pv_cases.SEMITONES):
        st.pitch_shift(d_in, d_out, v)
        torch.cuda.synchronize()
        o = d_out.cpu().numpy()
        assert np.array_equal(y[s], o[s]), (s, v, np.abs(y[s] - o[s]).max())
        assert not np.array_equal(kept[s], o[s]), s                                  # (preservation is another signal)
    st.close()


@pytest.mark.parametrize("N,hop", [(256, 256), (100, 512)])
def test_streaming_formant_following_the_pitch_is_the_curve_call(N, hop):
    from vocoderproject_amd import PhaseVocoderStream, semitones_to_ratios
    nb = 24 if N == 256 else 60
    x = pv_cases.mixed_streams(N * nb, seed=hop + N)
    r = semitones_to_ratios(np.array(pv_cases.SEMITONES))
    tab = _dev(np.tile(r, (nb, 1)), np.float64)
    d_in = _blocks(x, N)
    a, b = PhaseVocoderStream(S, N, hop=hop), PhaseVocoderStream(S, N, hop=hop)
    ya, yb = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    b0 = 0
    for k in pv_cases.call_spans(nb, FC.STREAM_CALLS):
        a.process_device(d_in[b0:b0 + k], ya[b0:b0 + k], n_blocks=k, d_ratio=tab[b0:b0 + k], d_formant=_dev(r, np.float64), lifter=64)
        b.process_device(d_in[b0:b0 + k], yb[b0:b0 + k], n_blocks=k, d_ratio=tab[b0:b0 + k])
        b0 += k
    torch.cuda.synchronize()
    a.close()
    b.close()
    ya, yb = _rows(ya), _rows(yb)
    assert np.all(np.isfinite(ya)) and np.abs(ya).max() > 0.05
    assert np.array_equal(ya, yb), np.abs(ya - yb).max()


# ---- 3. streaming equals one-shot; grouping -------------------------------------------------------------------------------------------------
def _stream_formant(c, x, tab, phi, spans):
    from vocoderproject_amd import PhaseVocoderStream
    ps = PhaseVocoderStream(S, c.N, hop=c.hop)
    d_in = _blocks(x, c.N)
    d_out = torch.full_like(d_in, float("nan"))
    d_tab, d_phi = _dev(tab, np.float64), _dev(phi, np.float64)
    n0 = ps.debug_alloc_count()
    b0 = 0
    for k in spans:
        rc = ps.L.vp_pv_process_blocks_formant_device(ps.h, d_in[b0:b0 + k].data_ptr(), d_out[b0:b0 + k].data_ptr(), d_tab[b0:b0 + k].data_ptr(),
                                                      d_phi.data_ptr(), c.nc, k, _cur())
        assert rc == 0
        b0 += k
    torch.cuda.synchronize()
    assert ps.debug_alloc_count() == n0 and n0 > 0                                    # streaming formant calls allocate nothing
    L = ps.latency
    ps.close()
    return _rows(d_out), L


# the call shapes FC.STREAM_CASES leave out: a first call in which no frame completes (N = 64), and single blocks of 256 at hop 256 (a
# call whose first frame is not wavefront 0's)
MORE_STREAM_CASES = [FC.StreamFormantCase(64, 256, 128, 32), FC.StreamFormantCase(256, 256, 32, 32)]


@pytest.mark.parametrize("c", FC.STREAM_CASES + MORE_STREAM_CASES, ids=FC.stream_id)
def test_streaming_formant_is_bit_identical_to_the_one_shot_and_grouping_changes_no_bit(c):
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios
    T = c.N * c.n_blocks
    x = FC.stream_input(c)
    tab = semitones_to_ratios(FC.stream_semitones(c))                                # [n_blocks][S]
    per_frame = FC.per_frame(tab, c.N, c.hop, T)
    nF = per_frame.shape[1]
    assert len(np.unique(per_frame[0])) > 3
    st = StftRoundTrip(S, T, F, c.hop)
    y1 = _formant(st, x, per_frame, FC.FORMANT_RATIOS, c.nc)
    st.close()
    y2, L = _stream_formant(c, x, tab, FC.FORMANT_RATIOS, pv_cases.call_spans(c.n_blocks, FC.STREAM_CALLS))
    n = min(nF * c.hop, T - L)                                                       # finished one-shot samples that the stream has emitted
    assert n > 2 * F and np.all(y2[:, :L] == 0)
    for s in range(S):
        assert np.array_equal(y2[s, L:L + n], y1[s, :n]), (s, np.abs(y2[s, L:L + n] - y1[s, :n]).max())
    y3, _ = _stream_formant(c, x, tab, FC.FORMANT_RATIOS, [c.n_blocks])              # one call
    y4, _ = _stream_formant(c, x, tab, FC.FORMANT_RATIOS, [1] * c.n_blocks)          # block by block
    assert np.array_equal(y2, y3) and np.array_equal(y2, y4)
    assert np.all(np.isfinite(y2))


def test_streaming_formant_matches_numpy():
    """The streaming kernel against the NumPy definition driven block by block (N = 100 at hop 128: blocks that end inside a round)."""
    import pv_formant_reference as FR
    c = FC.STREAM_CASES[1]
    x, semis = FC.stream_input(c), FC.stream_semitones(c)
    y, _ = _stream_formant(c, x, pv_cases.ratio_of(semis), FC.FORMANT_RATIOS, pv_cases.call_spans(c.n_blocks, FC.STREAM_CALLS))
    for s in range(S):
        ref = FR.by_block(x[s], c.N, c.hop, pv_cases.ratio_of(semis[:, s]), FC.FORMANT_RATIOS[s], c.nc)
        err, bnd = np.abs(y[s] - ref).max(), pv_cases.bound(c.hop, ref)
        print(f"FORMANT stream {FC.stream_id(c)} stream {s}: err {err:.3g} bound {bnd:.3g}")
        assert err <= bnd, (s, err, bnd)


# ---- 4. formant, curve and plain calls mixed on one handle ----------------------------------------------------------------------------------
def test_formant_curve_and_plain_calls_mix_on_one_handle():
    from vocoderproject_amd import PhaseVocoderStream, semitones_to_ratios
    N, hop, nc = 100, 128, 32
    spans = [3, 16, 5, 2, 7, 4]                                                      # formant, curve, plain (pending set_semitones), formant (pending reset), plain, formant
    kinds = ["formant", "curve", "plain", "formant", "plain", "formant"]
    nb = sum(spans)
    x = pv_cases.mixed_streams(N * nb, seed=hop + N + 2)
    tab = semitones_to_ratios(np.random.default_rng([N, hop, 12]).uniform(-12.0, 12.0, (nb, S)))
    d_in, d_tab, d_phi = _blocks(x, N), _dev(tab, np.float64), _dev(FC.FORMANT_RATIOS, np.float64)
    held0 = list(pv_cases.SEMITONES)

    def drive(single):
        ps = PhaseVocoderStream(S, N, hop=hop)
        for s, v in enumerate(held0):
            ps.set_semitones(v, stream=s)                                            # pending at the first formant call: stored, not used
        d_out = torch.full_like(d_in, float("nan"))
        b0 = 0
        for i, (k, kind) in enumerate(zip(spans, kinds)):
            if i == 2:
                ps.set_semitones(-3.0, stream=1)                                     # pending at a plain call
            if i == 3:
                ps.reset(2)                                                          # pending at a formant call
                ps.set_semitones(5.0, stream=4)                                      # ... stored by it, used by the plain call behind it
            for b in ([(b0, k)] if not single else [(b0 + j, 1) for j in range(k)]):
                lo, n = b
                kw = {}
                if kind != "plain":
                    kw["d_ratio"] = d_tab[lo:lo + n]
                if kind == "formant":
                    kw.update(d_formant=d_phi, lifter=nc)
                ps.process_device(d_in[lo:lo + n], d_out[lo:lo + n], n_blocks=n, **kw)
            b0 += k
        torch.cuda.synchronize()
        held = [ps.semitones(s) for s in range(S)]
        ps.close()
        return _rows(d_out), held

    ya, ha = drive(False)
    yb, hb = drive(True)
    assert np.all(np.isfinite(ya))
    b0 = 0
    for k, kind in zip(spans, kinds):
        assert np.array_equal(ya[:, b0 * N:(b0 + k) * N], yb[:, b0 * N:(b0 + k) * N]), (kind, b0)
        b0 += k
    assert ha == hb == [7.0, -3.0, 12.0, 0.37, 5.0]                                   # the held intervals: set_semitones' alone


def test_formant_calls_without_a_table_take_the_held_intervals():
    """process_device / run with formant_semitones and no ratio table: a constant table of the intervals set_semitones holds."""
    from vocoderproject_amd import PhaseVocoderStream, semitones_to_ratios
    N, hop, nb = 256, 256, 12
    x = pv_cases.mixed_streams(N * nb, seed=hop + N + 3)
    held, fsemi = np.array(pv_cases.SEMITONES), np.array([0.0, 0.0, -5.0, 12.0, -12.0])
    d_in = _blocks(x, N)
    a, b = PhaseVocoderStream(S, N, hop=hop), PhaseVocoderStream(S, N, hop=hop)
    for ps in (a, b):
        for s_, v in enumerate(held):
            ps.set_semitones(v, stream=s_)
    ya, yb = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    d_tab, d_phi = _dev(np.tile(semitones_to_ratios(held), (nb, 1)), np.float64), _dev(semitones_to_ratios(fsemi), np.float64)
    b0 = 0
    for k in (1, 3, 8):
        a.process_device(d_in[b0:b0 + k], ya[b0:b0 + k], n_blocks=k, formant_semitones=fsemi, lifter=24)
        b.process_device(d_in[b0:b0 + k], yb[b0:b0 + k], n_blocks=k, d_ratio=d_tab[b0:b0 + k], d_formant=d_phi, lifter=24)
        b0 += k
    torch.cuda.synchronize()
    ya, yb = _rows(ya), _rows(yb)
    assert np.all(np.isfinite(ya)) and np.abs(ya).max() > 0.05 and np.array_equal(ya, yb)
    assert [a.semitones(s_) for s_ in range(S)] == list(held)
    # run(): whole signals, with and without a curve of its own
    a.reset()
    b.reset()
    za = a.run(x, blocks_per_call=5, formant_semitones=fsemi, lifter=24)
    zb = b.run(x, blocks_per_call=5, curve=held[None, :], formant_semitones=fsemi, lifter=24)
    a.close()
    b.close()
    assert za.shape == x.shape and np.array_equal(za, zb) and np.abs(za).max() > 0.05
    L = 1024 - 256
    assert np.array_equal(za[:, :nb * N - L], ya[:, L:])                              # ... and they are the calls above, the latency taken off


# ---- 5. silence, DC, clamps -------------------------------------------------------------------------------------------------------------------
def test_silence_and_dc_stay_finite_and_silence_stays_zero():
    from vocoderproject_amd import StftRoundTrip
    c = FC.FormantCase(256, 19, 3, "glide", 32)
    T = FC.length(c)
    x = FC.case_input(c).copy()
    x[1] = 0.0
    x[3] = pv_cases.degenerate("dc", T)
    x[4] = 0.0
    st = StftRoundTrip(S, T, F, c.hop)
    y = _formant(st, x, FC.ratios_of(c), FC.FORMANT_RATIOS, c.nc)
    st.close()
    assert np.all(np.isfinite(y))
    assert np.all(y[1] == 0) and np.all(y[4] == 0)
    assert np.abs(y[3]).max() > 0.01 and np.abs(y[0]).max() > 0.01


def test_pitch_and_formant_ratios_are_clamped_and_a_nan_becomes_one_half():
    from vocoderproject_amd import StftRoundTrip
    c = FC.FormantCase(256, 19, 3, "steps", 32)
    x, clean = FC.case_input(c), FC.ratios_of(c)
    st = StftRoundTrip(S, FC.length(c), F, c.hop)
    y0 = _formant(st, x, clean, FC.FORMANT_RATIOS, c.nc)
    dirty, clamped = clean.copy(), clean.copy()
    for f, v, w in ((2, 0.1, 0.5), (5, 7.0, 2.0), (6, float("nan"), 0.5), (11, -1.0, 0.5), (18, float("inf"), 2.0)):
        dirty[2, f], clamped[2, f] = v, w
    yd = _formant(st, x, dirty, FC.FORMANT_RATIOS, c.nc)                             # (returns VP_OK: _formant asserts it)
    yc = _formant(st, x, clamped, FC.FORMANT_RATIOS, c.nc)
    assert np.all(np.isfinite(yd))
    assert np.array_equal(yd[2], yc[2]) and not np.array_equal(yd[2], y0[2])
    for s in (0, 1, 3, 4):
        assert np.array_equal(yd[s], y0[s]), s
    for v, w in ((0.1, 0.5), (float("nan"), 0.5), (9.0, 2.0)):
        pd, pc = FC.FORMANT_RATIOS.copy(), FC.FORMANT_RATIOS.copy()
        pd[0], pc[0] = v, w
        yd, yc = _formant(st, x, clean, pd, c.nc), _formant(st, x, clean, pc, c.nc)
        assert np.all(np.isfinite(yd))
        assert np.array_equal(yd[0], yc[0]) and not np.array_equal(yd[0], y0[0]), v
        for s in (1, 2, 3, 4):
            assert np.array_equal(yd[s], y0[s]), (v, s)
    st.close()


# ---- 6. errors before the device is touched ---------------------------------------------------------------------------------------------------
def test_argument_errors_are_reported_before_the_device_is_touched():
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, StreamingPitchTracker
    T = 4096
    st, st2k = StftRoundTrip(2, T, 1024, 256), StftRoundTrip(2, T, 2048, 512)
    d_in = _dev(np.zeros((2, T)), np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    d_r = _dev(np.ones((2, st.n_frames)), np.float64)
    d_phi = _dev(np.ones(2), np.float64)
    i, o, r, p = d_in.data_ptr(), d_out.data_ptr(), d_r.data_ptr(), d_phi.data_ptr()
    call = st.L.vp_stft_pitch_shift_formant
    for args in ((None, o, r, p, 32), (i, None, r, p, 32), (i, o, None, p, 32), (i, o, r, p, 3), (i, o, r, p, 65), (i, o, r, None, 0), (i, o, r, p, -1)):
        assert call(st.h, *args, _cur()) == VP_ERR_INVALID_ARG, args
        assert st.L.vp_stft_last_error(st.h).startswith(b"formant:")
    assert call(None, i, o, r, p, 32, _cur()) == VP_ERR_INVALID_ARG
    assert call(st2k.h, i, o, r, p, 32, _cur()) == VP_ERR_GEOMETRY
    assert b"2048" in st.L.vp_stft_last_error(st2k.h)
    d_p = torch.zeros((2, st2k.n_frames), dtype=torch.int32, device="cuda")
    tune = st.L.vp_stft_autotune_formant
    assert tune(st2k.h, i, o, 44100.0, None, d_p.data_ptr(), r, p, 32, _cur()) == VP_ERR_GEOMETRY
    assert tune(st.h, i, o, 44100.0, None, d_p.data_ptr(), r, p, 65, _cur()) == VP_ERR_INVALID_ARG
    assert tune(st.h, i, o, 44100.0, None, d_p.data_ptr(), None, p, 32, _cur()) == VP_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert torch.all(torch.isnan(d_out))                                             # nothing ran
    with pytest.raises(Exception):
        st2k.pitch_shift_formant(d_in, d_out, semitones=0.0)
    st.close()
    st2k.close()
    N = 256
    ps, trk = PhaseVocoderStream(2, N), StreamingPitchTracker(2, N, 44100.0)
    b_in = _dev(np.zeros((1, 2, N)), np.float32)
    b_out = torch.full_like(b_in, float("nan"))
    b_r = _dev(np.ones((1, 2)), np.float64)
    bi, bo, br = b_in.data_ptr(), b_out.data_ptr(), b_r.data_ptr()
    call = ps.L.vp_pv_process_blocks_formant_device
    for args in ((None, bo, br, p, 32, 1), (bi, None, br, p, 32, 1), (bi, bo, None, p, 32, 1), (bi, bo, br, p, 3, 1), (bi, bo, br, p, 65, 1), (bi, bo, br, p, 32, 0)):
        assert call(ps.h, *args, _cur()) == VP_ERR_INVALID_ARG, args
    assert call(None, bi, bo, br, p, 32, 1, _cur()) == VP_ERR_INVALID_ARG
    tune = ps.L.vp_pv_autotune_blocks_formant_device
    assert tune(ps.h, trk.h, bi, bo, None, None, br, p, 3, 1, _cur()) == VP_ERR_INVALID_ARG
    assert tune(ps.h, trk.h, bi, bo, None, None, None, p, 32, 1, _cur()) == VP_ERR_INVALID_ARG
    assert tune(ps.h, None, bi, bo, None, None, br, p, 32, 1, _cur()) == VP_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert torch.all(torch.isnan(b_out))
    ps.close()
    trk.close()


# ---- 7. the neighbours ----------------------------------------------------------------------------------------------------------------------
def test_round_trip_pitch_shift_and_curve_keep_their_bits_around_a_formant_call():
    from vocoderproject_amd import StftRoundTrip
    c = FC.FormantCase(512, 19, 3, "steps", 32)
    x, ratio = FC.case_input(c), FC.ratios_of(c)
    st = StftRoundTrip(S, FC.length(c), F, c.hop)
    d_in = _dev(x, np.float32)

    def three():
        o1, o2 = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
        st(d_in, o1)
        st.pitch_shift(d_in, o2, -5.0)
        torch.cuda.synchronize()
        return o1.cpu().numpy(), o2.cpu().numpy(), _curve(st, x, ratio)
    before = three()
    y = _formant(st, x, ratio, FC.FORMANT_RATIOS, c.nc)
    after = three()
    st.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert not np.array_equal(y, before[2])


# ---- 8. more workgroups than compute units ----------------------------------------------------------------------------------------------------
def test_three_hundred_streams():
    from vocoderproject_amd import StftRoundTrip
    x, ref = FC.big_input(), FC.big_reference()
    st = StftRoundTrip(FC.BIG_S, FC.BIG_T, F, FC.BIG_HOP)
    y = _formant(st, x, FC.big_ratios(), FC.big_formants(), FC.BIG_NC)
    st.close()
    assert np.all(np.isfinite(y))
    for s in FC.BIG_CHECKED:
        err, bnd = np.abs(y[s] - ref[s]).max(), pv_cases.bound(FC.BIG_HOP, ref[s])
        print(f"FORMANT big stream {s}: err {err:.3g} bound {bnd:.3g}")
        assert err <= bnd, (s, err, bnd)


# ---- 9. autotune against its two parts --------------------------------------------------------------------------------------------------------
def test_one_shot_autotune_formant_is_the_tracker_then_the_formant_call():
    import pv_track_cases as TC
    import pv_track_reference as R
    from vocoderproject_amd import StftRoundTrip
    hop, fs, nF = 256, 44100.0, 19
    T = F + (nF - 1) * hop + R.tau_max(fs) + 3
    x, keys = TC.make_input(("sine_off", "glide", "gap", "saw", "noise"), T, fs, F + hop), (12, 0, 7, 12, 3)
    st = StftRoundTrip(S, T, F, hop)
    d_in = _dev(x, np.float32)
    p, r = st.track_pitch(d_in, fs, keys=list(keys))
    torch.cuda.synchronize()
    assert len(np.unique(r.cpu().numpy())) > 4
    phi = FC.FORMANT_RATIOS
    want = _formant(st, x, r.cpu().numpy(), phi, 24)
    d_out = torch.full_like(d_in, float("nan"))
    d_p = torch.full((S, st.n_frames), -77, dtype=torch.int32, device="cuda")
    d_r = torch.full((S, st.n_frames), float("nan"), dtype=torch.float64, device="cuda")
    d_key, d_phi = _dev(keys, np.int32), _dev(phi, np.float64)
    rc = st.L.vp_stft_autotune_formant(st.h, d_in.data_ptr(), d_out.data_ptr(), fs, d_key.data_ptr(), d_p.data_ptr(), d_r.data_ptr(), d_phi.data_ptr(), 24, _cur())
    torch.cuda.synchronize()
    assert rc == 0
    y = d_out.cpu().numpy()
    assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.1
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(d_p.cpu().numpy(), p.cpu().numpy()) and np.array_equal(d_r.cpu().numpy().view(np.uint64), r.cpu().numpy().view(np.uint64))
    # the adapter: formant_semitones = None is today's autotune, a value the formant one
    plain = torch.full_like(d_in, float("nan"))
    st.pitch_shift_curve(d_in, plain, d_ratio=r)
    o_none, o_zero = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    st.autotune(d_in, o_none, fs, keys=list(keys))
    st.autotune(d_in, o_zero, fs, keys=list(keys), formant_semitones=0.0)
    torch.cuda.synchronize()
    kept = _formant(st, x, r.cpu().numpy(), None, 32)
    st.close()
    assert np.array_equal(o_none.cpu().numpy().view(np.uint32), plain.cpu().numpy().view(np.uint32))
    assert np.array_equal(o_zero.cpu().numpy().view(np.uint32), kept.view(np.uint32))
    assert not np.array_equal(kept, plain.cpu().numpy())


def test_streaming_autotune_formant_is_the_tracker_then_the_formant_call():
    import pv_track_stream_cases as SC
    from vocoderproject_amd import PhaseVocoderStream, StreamingPitchTracker
    c = SC.BY_NAME["n256-glide"]
    n, hop = len(c.signals), 256
    d_in = _dev(SC.case_input(c), np.float32)
    groups = SC.groupings(c)["mixed"]
    phi = FC.FORMANT_RATIOS[np.arange(n) % S]
    d_phi, keys = _dev(phi, np.float64), list(c.keys)

    def tracker():
        return StreamingPitchTracker(n, c.N, c.fs, c.F, hold_blocks=c.hold, glide=c.glide)
    outs = {}
    for variant in ("parts", "c", "python", "python-none", "curve-parts"):
        trk, pv = tracker(), PhaseVocoderStream(n, c.N, hop)
        d_out = torch.full_like(d_in, float("nan"))
        rs, b = [], 0
        for k in groups:
            i, o = d_in[b:b + k], d_out[b:b + k]
            if variant in ("parts", "curve-parts"):
                _, d_r = trk.process_device(i, n_blocks=k, keys=keys)
                pv.process_device(i, o, n_blocks=k, d_ratio=d_r, **({"d_formant": d_phi, "lifter": 24} if variant == "parts" else {}))
            elif variant == "c":
                d_r = torch.full((k, n), float("nan"), dtype=torch.float64, device="cuda")
                rc = pv.L.vp_pv_autotune_blocks_formant_device(pv.h, trk.h, i.data_ptr(), o.data_ptr(), _dev(keys, np.int32).data_ptr(), None, d_r.data_ptr(),
                                                               d_phi.data_ptr(), 24, k, _cur())
                assert rc == 0
            elif variant == "python":
                _, d_r = pv.autotune_device(trk, i, o, n_blocks=k, keys=keys, formant_semitones=12.0 * np.log2(phi), lifter=24)
            else:
                _, d_r = pv.autotune_device(trk, i, o, n_blocks=k, keys=keys)
            rs.append(d_r)
            b += k
        torch.cuda.synchronize()
        trk.close()
        pv.close()
        outs[variant] = (d_out.cpu().numpy(), torch.cat(rs).cpu().numpy())
    y, r = outs["parts"]
    assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.1 and len(np.unique(r)) > 4
    for v in ("c", "python"):
        assert np.array_equal(outs[v][1].view(np.uint64), r.view(np.uint64)), v
        assert np.array_equal(outs[v][0].view(np.uint32), y.view(np.uint32)), v
    assert np.array_equal(outs["python-none"][0].view(np.uint32), outs["curve-parts"][0].view(np.uint32))      # None: today's autotune
    assert not np.array_equal(outs["python-none"][0], y)
