"""The phase-vocoder harmonizer on the GPU (include/vp_amd.h vp_stft_harmonize, vp_hz_process_blocks_device; kernels vp_k_stft_harm and
vp_k_hz_stream of csrc/vp_stft_harm.inc): against the NumPy definition tests/pv_harm_reference.py on the cases of
tests/pv_harm_cases.py (whose teeth tests/test_pv_harm_reference_cpu.py shows), bit ties to the locked call and to the round trip it is
made of, voices that keep their own angles, the streaming call bit-identical to the one-shot under every grouping, resets, 300 streams,
degenerate inputs, argument errors, what the call is for (a chord), and the Python adapters.  The PVHARM lines (-s) are what
profiles/pv_harm_errors.txt is made of.

Figures of the one-shot comparison on an MI355X: worst err / bound over the 96 cases x 6 streams is recorded in
profiles/pv_harm_errors.txt."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_harm_cases as HC  # noqa: E402
import pv_harm_reference as HR  # noqa: E402
import pv_lock_cases as LC  # noqa: E402
import stft_reference  # noqa: E402

pytestmark = pytest.mark.gpu

S, F = HC.S, HC.F
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4              # include/vp_amd.h


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _harm(st, x, ratio, gain=None, dry=None):
    """One vp_stft_harmonize call on x [S][T] with ratio [S][V][nF], gain [S][V] or None, dry [S] or None; the output starts as NaN, so
    every sample must have been written."""
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    ratio = np.asarray(ratio)
    assert ratio.shape == (x.shape[0], ratio.shape[1], st.n_frames), ratio.shape
    d_ratio = _dev(ratio, np.float64)
    d_gain = None if gain is None else _dev(gain, np.float64)
    d_dry = None if dry is None else _dev(dry, np.float64)
    rc = st.L.vp_stft_harmonize(st.h, d_in.data_ptr(), d_out.data_ptr(), ratio.shape[1], d_ratio.data_ptr(), _ptr(d_gain), _ptr(d_dry), _cur())
    torch.cuda.synchronize()
    assert rc == 0, (rc, st.L.vp_stft_last_error(st.h))
    return d_out.cpu().numpy()


def _one_shot(x, ratio, hop, gain=None, dry=None):
    from vocoderproject_amd import StftRoundTrip
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    y = _harm(st, x, ratio, gain, dry)
    st.close()
    return y


def _blocks(x, N):
    n, T = x.shape
    return _dev(x.reshape(n, T // N, N).transpose(1, 0, 2), np.float32)


def _rows(d):
    nb, n, N = d.shape
    return d.cpu().numpy().transpose(1, 0, 2).reshape(n, nb * N)


def _stream(hz, d_in, d_tab, spans, d_gain=None, d_dry=None, b0=0, d_out=None):
    """Streaming calls of `spans` blocks each from block b0 on; returns the device output [n_blocks][S][N] (NaN where no call wrote)."""
    if d_out is None:
        d_out = torch.full_like(d_in, float("nan"))
    for k in spans:
        rc = hz.L.vp_hz_process_blocks_device(hz.h, d_in[b0:b0 + k].data_ptr(), d_out[b0:b0 + k].data_ptr(), d_tab[b0:b0 + k].data_ptr(), _ptr(d_gain),
                                              _ptr(d_dry), k, _cur())
        assert rc == 0, rc
        b0 += k
    return d_out


# ---- 1. one-shot against NumPy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nF", HC.NFS)
@pytest.mark.parametrize("hop", HC.HOPS)
def test_one_shot_matches_numpy(hop, nF):
    """Mixed content, every residue mod 4 of the last round, a tail of hop - 1 samples no frame covers; every voice set with gains that
    differ between streams (a 0, a negative, a 4.0, a NaN) and dry 0, 1 and 0.5."""
    from vocoderproject_amd import StftRoundTrip
    x = LC.gpu_input(hop, nF)
    T = x.shape[1]
    st = StftRoundTrip(S, T, F, hop)
    assert st.n_frames == nF
    for V in HC.VOICE_SETS:
        ref, bnd = HC.reference(V, hop, nF)
        y = _harm(st, x, HC.ratios(V, hop, nF), HC.gains(V), HC.DRY)
        assert np.all(np.isfinite(y))
        for s in range(S):
            err = np.abs(y[s] - ref[s]).max()
            print(f"PVHARM one-shot hop{hop}-nF{nF}-V{V} stream {s} ({LC.GPU_STREAMS[s]}): err {err:.3g} bound {bnd[s]:.3g} err/bound {err / bnd[s]:.3f}")
            assert err <= bnd[s], (V, s, err, bnd[s])
        covered = (nF - 1) * hop + F
        assert np.all(y[:, covered:] == 0) and y[:, covered:].shape[1] == hop - 1       # samples no frame covers
    st.close()


# ---- 2. bit ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", HC.HOPS)
def test_one_voice_with_gain_one_and_no_dry_part_has_the_locked_call_s_bits(hop):
    from vocoderproject_amd import StftRoundTrip
    nF = 7
    x = LC.gpu_input(hop, nF)
    st = StftRoundTrip(S, x.shape[1], F, hop)
    d_in = _dev(x, np.float32)
    for name in LC.GPU_CURVES:
        r = LC.gpu_ratios(name, hop, nF)
        d_lk = torch.full_like(d_in, float("nan"))
        st.pitch_shift_locked(d_in, d_lk, d_ratio=_dev(r, np.float64))
        torch.cuda.synchronize()
        lk = d_lk.cpu().numpy()
        y = _harm(st, x, r[:, None, :], np.ones((S, 1)), None)
        assert np.all(np.isfinite(lk)) and np.abs(lk).max() > 0.05
        assert np.array_equal(y, lk), (name, np.abs(y - lk).max())
        assert np.array_equal(_harm(st, x, r[:, None, :], None, None), lk), name      # a null gain table: every gain 1
        assert np.array_equal(_harm(st, x, r[:, None, :], None, np.zeros(S)), lk), name
    st.close()


@pytest.mark.parametrize("hop", HC.HOPS)
def test_all_gains_zero_with_dry_one_has_the_double_round_trip_s_bits(hop):
    from vocoderproject_amd import StftRoundTrip
    nF = 7
    x = LC.gpu_input(hop, nF)
    st = StftRoundTrip(S, x.shape[1], F, hop)
    d_in = _dev(x, np.float32)
    d_rt = torch.full_like(d_in, float("nan"))
    st(d_in, d_rt)
    torch.cuda.synchronize()
    rt = d_rt.cpu().numpy()
    for V in (1, 3):
        y = _harm(st, x, HC.ratios(V, hop, nF), np.zeros((S, V)), np.ones(S))
        assert np.array_equal(y, rt), (V, np.abs(y - rt).max())
    st.close()
    assert np.abs(rt).max() > 0.05


def test_a_null_gain_table_is_a_table_of_ones_and_rows_are_independent_and_homogeneous():
    hop, nF, V = 128, 7, 3
    x = LC.gpu_input(hop, nF)
    r, dry = HC.ratios(V, hop, nF), HC.DRY
    y = _one_shot(x, r, hop, None, dry)
    assert np.array_equal(_one_shot(x, r, hop, np.ones((S, V)), dry), y)
    g = HC.gains(V)
    y = _one_shot(x, r, hop, g, dry)
    perm = np.array([3, 0, 5, 1, 4, 2])
    assert np.array_equal(_one_shot(x[perm], r[perm], hop, g[perm], dry[perm]), y[perm])
    for e in (-6, 3):
        assert np.array_equal(_one_shot(x * np.float32(2.0 ** e), r, hop, g, dry), y * np.float32(2.0 ** e)), e
    x0 = x.copy()
    x0[2] = 0.0
    y0 = _one_shot(x0, r, hop, g, dry)
    assert np.all(y0[2] == 0) and np.array_equal(np.delete(y0, 2, 0), np.delete(y, 2, 0))


# ---- 3. voices keep their own angles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", HC.HOPS)
def test_a_voice_with_gain_zero_leaves_the_other_voice_s_bits(hop):
    """(each one-voice output is multiplied by gain 1 in double and the sum adds a +-0 term: np.array_equal takes -0 as 0)"""
    nF, V = 8, 2
    x = LC.gpu_input(hop, nF)
    r = HC.ratios(V, hop, nF)
    a = _one_shot(x, r[:, :1], hop, np.ones((S, 1)), None)
    b = _one_shot(x, r[:, 1:], hop, np.ones((S, 1)), None)
    assert not np.array_equal(a, b) and np.abs(a).max() > 0.05 and np.abs(b).max() > 0.05
    ya = _one_shot(x, r, hop, np.tile([1.0, 0.0], (S, 1)), None)
    yb = _one_shot(x, r, hop, np.tile([0.0, 1.0], (S, 1)), None)
    assert np.array_equal(ya, a), np.abs(ya - a).max()
    assert np.array_equal(yb, b), np.abs(yb - b).max()


# ---- 4. streaming -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", HC.STREAM_BLOCKS)
@pytest.mark.parametrize("hop", HC.HOPS)
def test_streaming_is_bit_identical_to_the_one_shot(hop, N):
    from vocoderproject_amd import HarmonizerStream
    V = HC.STREAM_V
    x, tab = LC.stream_input(hop, N), HC.stream_ratios(hop, N)
    nb, T = tab.shape[0], x.shape[1]
    per_frame = HC.per_frame(tab, N, hop, T)
    g, dry = HC.gains(V), np.full(S, HC.STREAM_DRY)
    y1 = _one_shot(x, per_frame, hop, g, dry)
    hz = HarmonizerStream(S, N, V, hop=hop)
    n0 = hz.debug_alloc_count()
    d_out = _stream(hz, _blocks(x, N), _dev(tab, np.float64), pv_cases.call_spans(nb, HC.STREAM_CALLS), _dev(g, np.float64), _dev(dry, np.float64))
    torch.cuda.synchronize()
    assert hz.debug_alloc_count() == n0 and n0 > 0
    L = hz.latency
    hz.close()
    assert L == F - np.gcd(N, hop)
    y2 = _rows(d_out)
    n = min(per_frame.shape[2] * hop, T - L)                                         # finished one-shot samples that the stream has emitted
    assert n > 2 * F and np.all(y2[:, :L] == 0) and np.all(np.isfinite(y2))
    for s in range(S):
        assert np.array_equal(y2[s, L:L + n], y1[s, :n]), (s, np.abs(y2[s, L:L + n] - y1[s, :n]).max())


@pytest.mark.parametrize("hop,N", [(64, 17), (128, 1000), (256, 256), (512, 64), (256, 4096)])
def test_grouping_of_the_calls_changes_no_bit(hop, N):
    from vocoderproject_amd import HarmonizerStream
    V = HC.STREAM_V
    x, tab = LC.stream_input(hop, N), HC.stream_ratios(hop, N)
    nb = tab.shape[0]
    d_in, d_tab, d_g, d_d = _blocks(x, N), _dev(tab, np.float64), _dev(HC.gains(V), np.float64), _dev(np.full(S, HC.STREAM_DRY), np.float64)
    outs = []
    for grp in (1, 3, 16):
        hz = HarmonizerStream(S, N, V, hop=hop)
        outs.append(_rows(_stream(hz, d_in, d_tab, pv_cases.call_spans(nb, (grp,)), d_g, d_d)))
        hz.close()
    assert np.all(np.isfinite(outs[0])) and np.abs(outs[0]).max() > 0.05
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_streaming_matches_numpy_block_by_block():
    """N = 100 at hop 128: blocks that end inside a round; the reference is driven block by block, the dry part delayed by the latency."""
    from vocoderproject_amd import HarmonizerStream
    hop, N, V = 128, 100, 3
    nb = 62
    x = np.stack([LC.SIGNALS[s](N * nb, seed=hop + N) for s in LC.GPU_STREAMS])
    tab = LC.ratio_of(np.random.default_rng([hop, N, 52]).uniform(-13.0, 13.0, (nb, S, V)))
    g, dry = HC.gains(V), HC.DRY
    hz = HarmonizerStream(S, N, V, hop=hop)
    y = _rows(_stream(hz, _blocks(x, N), _dev(tab, np.float64), pv_cases.call_spans(nb, HC.STREAM_CALLS), _dev(g, np.float64), _dev(dry, np.float64)))
    L = hz.latency
    hz.close()
    for s in range(S):
        ref = HR.by_block(x[s], N, hop, tab[:, s, :], g[s], dry[s])
        refs = [LC.LR.by_block(x[s], N, hop, tab[:, s, v]) for v in range(V)]
        rt = np.concatenate((np.zeros(L), stft_reference.stft_roundtrip(x[s], F, hop)[:N * nb - L]))
        bnd = HR.gpu_bound(hop, dry[s], rt, g[s], refs)
        err = np.abs(y[s] - ref).max()
        print(f"PVHARM stream N{N}-hop{hop} stream {s} ({LC.GPU_STREAMS[s]}): err {err:.3g} bound {bnd:.3g} err/bound {err / bnd:.3f}")
        assert err <= bnd, (s, err, bnd)


def _schedule_input(N, nb, hop, V, n=S):
    x = np.stack([LC.SIGNALS[LC.GPU_STREAMS[s % S]](N * nb, seed=hop + 11 + s // S) for s in range(n)])
    tab = LC.ratio_of(np.random.default_rng([hop, N, 53]).uniform(-12.0, 12.0, (nb, n, V)))
    return x, tab


def test_forty_single_block_calls_allocate_nothing():
    from vocoderproject_amd import HarmonizerStream
    N, hop, nb, V = 64, 128, 40, 4
    x, tab = _schedule_input(N, nb, hop, V)
    hz = HarmonizerStream(S, N, V, hop=hop)
    n0 = hz.debug_alloc_count()
    y = _rows(_stream(hz, _blocks(x, N), _dev(tab, np.float64), [1] * nb, None, _dev(np.ones(S), np.float64)))
    assert hz.debug_alloc_count() == n0 and n0 > 0 and np.all(np.isfinite(y))
    hz.close()


@pytest.mark.parametrize("hop", [64, 256])
def test_a_reset_in_the_middle_of_a_round_restarts_that_stream_alone(hop):
    from vocoderproject_amd import HarmonizerStream
    N, nb, cut, V = 100, 60, 27, 3                                                   # the reset lands before block 27: sample 2700
    x, tab = _schedule_input(N, nb, hop, V)
    assert ((cut * N - F) // hop + 1) % 4 != 0                                       # frames so far: not at a round's end
    d_in, d_tab, d_d = _blocks(x, N), _dev(tab, np.float64), _dev(np.full(S, 0.5), np.float64)
    a = HarmonizerStream(S, N, V, hop=hop)
    d_a = _stream(a, d_in, d_tab, [cut], None, d_d)
    a.reset(2)
    _stream(a, d_in, d_tab, [nb - cut], None, d_d, cut, d_a)
    ya = _rows(d_a)
    a.close()
    b = HarmonizerStream(S, N, V, hop=hop)                                           # never reset
    yb = _rows(_stream(b, d_in, d_tab, [nb], None, d_d))
    b.close()
    f = HarmonizerStream(S, N, V, hop=hop)                                           # a fresh handle from the cut on
    yf = _rows(_stream(f, d_in[cut:].contiguous(), d_tab[cut:].contiguous(), [nb - cut], None, d_d))
    f.close()
    assert np.all(np.isfinite(yb)) and np.abs(yb).max() > 0.05
    for s in range(S):
        if s == 2:
            assert np.array_equal(ya[s, :cut * N], yb[s, :cut * N]) and np.array_equal(ya[s, cut * N:], yf[s])
            assert not np.array_equal(ya[s, cut * N:], yb[s, cut * N:])
        else:
            assert np.array_equal(ya[s], yb[s]), s


def test_forty_pending_resets_are_all_applied():
    """More pending resets than a call's arguments carry (16): update launches in front of the call."""
    from vocoderproject_amd import HarmonizerStream
    S2, N, hop, nb, cut, V = 40, 256, 256, 12, 5, 2
    x, tab = _schedule_input(N, nb, hop, V, S2)
    d_in, d_tab = _blocks(x, N), _dev(tab, np.float64)
    a = HarmonizerStream(S2, N, V, hop=hop)
    d_a = _stream(a, d_in, d_tab, [cut])
    for s in range(S2):
        a.reset(s)
    _stream(a, d_in, d_tab, [nb - cut], None, None, cut, d_a)
    ya = _rows(d_a)
    a.close()
    f = HarmonizerStream(S2, N, V, hop=hop)
    yf = _rows(_stream(f, d_in[cut:].contiguous(), d_tab[cut:].contiguous(), [nb - cut]))
    f.close()
    assert np.abs(yf).max() > 0.05 and np.all(np.isfinite(ya))
    for s in range(S2):
        assert np.array_equal(ya[s, cut * N:], yf[s]), s


# ---- 5. more workgroups than compute units ------------------------------------------------------------------------------------------------------
def test_three_hundred_streams():
    from vocoderproject_amd import HarmonizerStream
    BIG, hop, N, nb, V = 300, 256, 256, 12, 3
    T = N * nb
    x = pv_cases.harmonic_streams(BIG, T, seed=hop + 3)
    curves = ("steps", "+7", "vibrato")
    tab = np.stack([np.stack([LC.curve(c, nb, hop, s) for c in curves], axis=1) for s in range(BIG)], axis=1)     # [nb][BIG][V]
    assert tab.shape == (nb, BIG, V)
    per_frame = HC.per_frame(tab, N, hop, T)
    g = np.tile([1.0, 0.5, -0.75], (BIG, 1))
    dry = np.full(BIG, 0.5)
    y1 = _one_shot(x, per_frame, hop, g, dry)
    for s in (0, 1, 149, 255, 256, 299):
        refs = [LC.LR.locked_roundtrip(x[s], per_frame[s, v], F, hop) for v in range(V)]
        rt = stft_reference.stft_roundtrip(x[s], F, hop)
        ref, bnd = HR.from_parts(rt, refs, g[s], dry[s]), HR.gpu_bound(hop, dry[s], rt, g[s], refs)
        err = np.abs(y1[s] - ref).max()
        print(f"PVHARM big stream {s}: err {err:.3g} bound {bnd:.3g} err/bound {err / bnd:.3f}")
        assert err <= bnd, (s, err, bnd)
    hz = HarmonizerStream(BIG, N, V, hop=hop)
    y2 = _rows(_stream(hz, _blocks(x, N), _dev(tab, np.float64), [5, 7], _dev(g, np.float64), _dev(dry, np.float64)))
    L = hz.latency
    hz.close()
    n = min(per_frame.shape[2] * hop, T - L)
    assert np.array_equal(y2[:, L:L + n], y1[:, :n])


# ---- 6. degenerate inputs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [64, 512])
def test_degenerate_inputs_stay_finite_and_bounded(hop):
    from vocoderproject_amd import HarmonizerStream
    nF, V = 9, 4
    T = LC.length(nF, hop, 5)
    x = np.stack([pv_cases.degenerate(n, T) for n in LC.DEGENERATE])
    n = len(x)
    r = np.stack([np.stack([LC.curve("outside", nF, hop, s + v) for v in range(V)]) for s in range(n)])
    g = np.array([[1.0, -0.5, 4.0, 0.25]] * n)
    dry = np.array([1.0, 0.5, -1.0, 1.0])
    y = _one_shot(x, r, hop, g, dry)
    assert np.all(np.isfinite(y)) and np.all(y[0] == 0)
    for s in range(n):                                                               # every voice is a translation and a rotation of the bins: no frame gains magnitude
        assert np.abs(y[s]).max() <= (abs(dry[s]) + np.abs(g[s]).sum()) * pv_cases.magnitude_ceiling(x[s], hop) + 1e-6, s
    N, nb = 100, 30
    xs = np.stack([pv_cases.degenerate(nm, N * nb) for nm in LC.DEGENERATE])
    tab = np.stack([np.stack([LC.curve("outside", nb, hop, s + v) for v in range(V)], axis=1) for s in range(n)], axis=1)
    hz = HarmonizerStream(n, N, V, hop=hop)
    ys = _rows(_stream(hz, _blocks(xs, N), _dev(tab, np.float64), pv_cases.call_spans(nb, HC.STREAM_CALLS), _dev(g, np.float64), _dev(dry, np.float64)))
    hz.close()
    assert np.all(np.isfinite(ys)) and np.all(ys[0] == 0)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_reported_before_the_device_is_touched():
    from vocoderproject_amd import HarmonizerStream, StftRoundTrip, VpError
    st2 = StftRoundTrip(2, 8192, 2048, 512)
    d = torch.zeros((2, 8192), dtype=torch.float32, device="cuda")
    o = torch.full_like(d, 7.0)
    r = torch.ones((2, 2, st2.n_frames), dtype=torch.float64, device="cuda")
    rc = st2.L.vp_stft_harmonize(st2.h, d.data_ptr(), o.data_ptr(), 2, r.data_ptr(), None, None, _cur())
    msg = st2.L.vp_stft_last_error(st2.h)
    assert rc == VP_ERR_GEOMETRY and msg.startswith(b"harmonize: ") and b"2048-point frames are not built" in msg, msg
    with pytest.raises(VpError) as e:
        st2.harmonize(d, o, d_ratio=r)
    assert "2048-point" in str(e.value)
    st2.close()
    st = StftRoundTrip(2, 8192, 1024, 256)
    L = st.L
    r = torch.ones((2, 4, st.n_frames), dtype=torch.float64, device="cuda")
    i_, o_, r_ = d.data_ptr(), o.data_ptr(), r.data_ptr()
    assert L.vp_stft_harmonize(None, i_, o_, 2, r_, None, None, _cur()) == VP_ERR_INVALID_ARG
    for args in ((None, o_, 2, r_), (i_, None, 2, r_), (i_, o_, 2, None)):
        assert L.vp_stft_harmonize(st.h, *args, None, None, _cur()) == VP_ERR_INVALID_ARG
        assert b"harmonize: null" in L.vp_stft_last_error(st.h)
    for V in (0, 5, -1):
        assert L.vp_stft_harmonize(st.h, i_, o_, V, r_, None, None, _cur()) == VP_ERR_INVALID_ARG
        assert b"harmonize: the number of voices" in L.vp_stft_last_error(st.h)
    st.close()
    hz = HarmonizerStream(2, 256, 2)
    x = torch.zeros((2, 256), dtype=torch.float32, device="cuda")
    bo = torch.full_like(x, 7.0)
    br = torch.ones((1, 2, 2), dtype=torch.float64, device="cuda")
    i_, o2, r_ = x.data_ptr(), bo.data_ptr(), br.data_ptr()
    assert L.vp_hz_process_blocks_device(None, i_, o2, r_, None, None, 1, _cur()) == VP_ERR_INVALID_ARG
    for args in ((None, o2, r_, 1), (i_, None, r_, 1), (i_, o2, None, 1), (i_, o2, r_, 0), (i_, o2, r_, -3)):
        assert L.vp_hz_process_blocks_device(hz.h, *args[:3], None, None, args[3], _cur()) == VP_ERR_INVALID_ARG
    assert L.vp_hz_reset(hz.h, 2) == VP_ERR_INVALID_ARG and L.vp_hz_reset(hz.h, -2) == VP_ERR_INVALID_ARG
    hz.close()
    h = C.c_void_p()
    for V in (0, 5):
        assert L.vp_hz_create(0, 2, 256, 1024, 256, V, C.byref(h)) == VP_ERR_INVALID_ARG and not h.value
    assert L.vp_hz_create(0, 2, 256, 2048, 512, 2, C.byref(h)) == VP_ERR_GEOMETRY and not h.value
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((bo == 7.0).all())                       # the prefilled outputs are untouched


# ---- 8. behaviour -----------------------------------------------------------------------------------------------------------------------------------
def test_a_tone_becomes_a_chord_whose_notes_follow_their_gains():
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios
    fs, hop, T = 44100.0, 256, 32768
    x = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(T) / fs)).astype(np.float32)[None].repeat(2, 0)
    st = StftRoundTrip(2, T, F, hop)
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    st.harmonize(d_in, d_out, semitones=[4.0, 7.0], gains=[1.0, 0.5], dry=1.0)
    torch.cuda.synchronize()
    st.close()
    y = d_out.cpu().numpy()[0]
    assert np.all(np.isfinite(y))
    seg = y[4096:4096 + 16384] * np.hanning(16384)
    spec = np.abs(np.fft.rfft(seg))
    loc = [k for k in range(2, len(spec) - 2) if spec[k] > spec[k - 1] and spec[k] >= spec[k + 1]]
    top = sorted(sorted(loc, key=lambda k: -spec[k])[:3])
    r4, r7 = (float(v) for v in semitones_to_ratios(np.array([4.0, 7.0])))
    got = []
    for k in top:
        a, b, c = np.log(spec[k - 1:k + 2])
        got.append(((k + 0.5 * (a - c) / (a - 2 * b + c)) * fs / 16384, spec[k]))
    print("PVHARM chord: peaks " + ", ".join(f"{f:.2f} Hz ({m:.1f})" for f, m in got) + f"; wanted 440.00, {440.0 * r4:.2f}, {440.0 * r7:.2f}")
    for (f, _), want in zip(got, (440.0, 440.0 * r4, 440.0 * r7)):
        assert abs(f - want) < 3.0, (f, want)
    assert got[2][1] < got[1][1], got                                                # the fifth at gain 0.5 is lower than the third at gain 1


# ---- 9. the Python adapters ---------------------------------------------------------------------------------------------------------------------------
def test_the_python_entries_build_the_same_tables():
    from vocoderproject_amd import HarmonizerStream, StftRoundTrip, semitones_to_ratios
    hop, nF, V = 256, 7, 3
    x = LC.gpu_input(hop, nF)
    st = StftRoundTrip(S, x.shape[1], F, hop)
    semis = np.random.default_rng(5).uniform(-12.0, 12.0, (S, V, nF))
    g, dry = HC.gains(V), HC.DRY
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))

    def py(**kw):
        d_out.fill_(float("nan"))
        st.harmonize(d_in, d_out, **kw)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()
    want = _harm(st, x, semitones_to_ratios(semis), g, dry)
    assert np.array_equal(py(semitones=semis, gains=g, dry=dry), want)                # [S][V][nF]
    assert np.array_equal(py(d_ratio=_dev(semitones_to_ratios(semis), np.float64), gains=_dev(g, np.float64), dry=_dev(dry, np.float64)), want)
    want = _harm(st, x, semitones_to_ratios(np.broadcast_to(semis[0], (S, V, nF))), np.tile(g[0], (S, 1)), np.full(S, 0.5))
    assert np.array_equal(py(semitones=semis[0], gains=g[0], dry=0.5), want)          # [V][nF]: the same curves for every stream
    fixed = np.array([4.0, 7.0, -5.0])
    want = _harm(st, x, semitones_to_ratios(np.broadcast_to(fixed[None, :, None], (S, V, nF))), None, None)
    assert np.array_equal(py(semitones=fixed), want)                                  # [V]: fixed intervals, every gain 1, no dry part
    st.close()
    # the stream: run() against the device call on the same blocks
    N, nb = 256, 12
    xs = np.stack([LC.SIGNALS[s](N * nb, seed=3) for s in LC.GPU_STREAMS])
    hz = HarmonizerStream(S, N, V, hop=hop)
    L = hz.latency
    nbt = -(-(N * nb + L) // N)
    y = hz.run(xs, fixed, blocks_per_call=5, gains=g, dry=dry)
    hz.close()
    xp = np.concatenate((xs, np.zeros((S, nbt * N - N * nb), np.float32)), axis=1)
    tab = np.broadcast_to(semitones_to_ratios(fixed), (nbt, S, V))
    hz = HarmonizerStream(S, N, V, hop=hop)
    want = _rows(_stream(hz, _blocks(xp, N), _dev(tab, np.float64), [nbt], _dev(g, np.float64), _dev(dry, np.float64)))
    hz.close()
    assert y.shape == xs.shape and np.array_equal(y, want[:, L:L + N * nb]) and np.abs(y).max() > 0.05
