"""The key-aware voices on the GPU (include/vp_amd.h vp_stft_track_harmony, vp_stft_harmonize_key,
vp_pv_tracker_process_blocks_voices_device, vp_hz_autoharm_blocks_device; kernels vp_k_yin_track_voices, vp_k_yin_track_voices_stream and
vp_k_track_follow_voices of csrc/vp_track.hip), through the C ABI and the Python mirror.  Everything compares bit for bit with
tests/pv_harmkey_reference.py and tests/pv_harmkey_stream_reference.py on the cases of tests/pv_harmkey_cases.py (whose conditioning
tests/test_pv_harmkey_reference_cpu.py gates); the one tolerance, the chord's, comes from the definitions
(profiles/pv_harmkey_quality.txt)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_harm_cases as HC  # noqa: E402
import pv_harmkey_cases as K  # noqa: E402
import pv_harmkey_reference as HR  # noqa: E402
import pv_harmkey_stream_reference as HSR  # noqa: E402

pytestmark = pytest.mark.gpu

S = K.S
GUARD, GUARD_F, GUARD_I = 16, 7.25, -777                     # guard words before and after every output table
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(p, r, want_p, want_r):
    assert p.shape == want_p.shape and r.shape == want_r.shape, (p.shape, want_p.shape, r.shape, want_r.shape)
    bad = np.argwhere(p != want_p)
    assert bad.size == 0, ("period", len(bad), bad[:4].tolist(), p[tuple(bad[0])], want_p[tuple(bad[0])])
    bad = np.argwhere(_bits(r) != _bits(want_r))
    assert bad.size == 0, ("ratio", len(bad), bad[:4].tolist(), r[tuple(bad[0])], want_r[tuple(bad[0])])


class _Guarded:
    """An output table between guard words: the table starts as NaN (or the int sentinel), the guards must come back untouched."""

    def __init__(self, shape, dtype):
        self.n, self.shape, self.f = int(np.prod(shape)), shape, dtype == torch.float64
        self.buf = torch.full((self.n + 2 * GUARD,), GUARD_F if self.f else GUARD_I, dtype=dtype, device="cuda")
        self.tab = self.buf[GUARD:GUARD + self.n]
        self.tab.fill_(float("nan") if self.f else GUARD_I)

    def get(self):
        """The table as NumPy, every slot written and finite, the guards untouched (after a synchronise)."""
        b = self.buf.cpu().numpy()
        g = np.concatenate([b[:GUARD], b[GUARD + self.n:]])
        assert np.all(g == (GUARD_F if self.f else GUARD_I)), "a guard word was written"
        t = b[GUARD:GUARD + self.n].reshape(self.shape)
        assert np.all(np.isfinite(t)) if self.f else not np.any(t == GUARD_I)
        return t


def _harmony(st, d_in, fs, keys, degrees, unvoiced):
    """vp_stft_track_harmony through the C ABI -> (period [S][nF], ratio [S][V][nF]) as NumPy."""
    V = degrees.shape[1]
    d_key, d_deg = None if keys is None else _dev(keys, np.int32), _dev(degrees, np.int32)
    d_unv = None if unvoiced is None else _dev(unvoiced, np.float64)
    gp, gr = _Guarded((st.S, st.n_frames), torch.int32), _Guarded((st.S, V, st.n_frames), torch.float64)
    rc = st.L.vp_stft_track_harmony(st.h, d_in.data_ptr(), fs, _ptr(d_key), V, d_deg.data_ptr(), _ptr(d_unv), gp.tab.data_ptr(), gr.tab.data_ptr(), _cur())
    torch.cuda.synchronize()
    assert rc == 0, (rc, st.L.vp_stft_last_error(st.h))
    return gp.get(), gr.get()


# ---- 1. the batch call against the definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_period_and_ratio_equal_the_definition(c):
    from vocoderproject_amd import StftRoundTrip
    want_p, want_r = K.reference(c)
    st = StftRoundTrip(S, c.T, c.F, c.hop)
    p, r = _harmony(st, _dev(K.batch_input(c), np.float32), c.fs, c.keys, K.degrees_of(c), K.unvoiced_of(c))
    st.close()
    _same(p, r, want_p, want_r)


def test_one_output_may_be_null_and_keys_may_be_null():
    from vocoderproject_amd import StftRoundTrip
    c = K.BY_NAME["steady-v3"]
    x, deg = K.batch_input(c), K.degrees_of(c)
    want_p, want_r = HR.track_harmony(x, c.fs, c.F, c.hop, deg, None, None)          # no key table: chromatic everywhere
    st = StftRoundTrip(S, c.T, c.F, c.hop)
    d_in, d_deg = _dev(x, np.float32), _dev(deg, np.int32)
    gp, gr = _Guarded(want_p.shape, torch.int32), _Guarded(want_r.shape, torch.float64)
    assert st.L.vp_stft_track_harmony(st.h, d_in.data_ptr(), c.fs, None, 3, d_deg.data_ptr(), None, gp.tab.data_ptr(), None, _cur()) == 0
    assert st.L.vp_stft_track_harmony(st.h, d_in.data_ptr(), c.fs, None, 3, d_deg.data_ptr(), None, None, gr.tab.data_ptr(), _cur()) == 0
    torch.cuda.synchronize()
    st.close()
    _same(gp.get(), gr.get(), want_p, want_r)


def test_out_of_range_degrees_are_clamped_on_the_device():
    from vocoderproject_amd import StftRoundTrip
    c = K.BY_NAME["steady-v3"]
    x = K.batch_input(c)
    wild = np.array([[13, -13, 2 ** 31 - 1], [-2 ** 31, 100, -100], [12, -12, 0]], np.int32)
    want_p, want_r = HR.track_harmony(x, c.fs, c.F, c.hop, np.clip(wild, -12, 12), c.keys, None)
    st = StftRoundTrip(S, c.T, c.F, c.hop)
    p, r = _harmony(st, _dev(x, np.float32), c.fs, c.keys, wild, None)
    st.close()
    _same(p, r, want_p, want_r)


@pytest.mark.parametrize("name", ["steady-v4", "glide-v4", "popped", "f2048"])
def test_every_voice_at_degree_zero_has_track_pitch_s_rows(name):
    from vocoderproject_amd import StftRoundTrip
    c = K.BY_NAME[name]
    V = len(c.degrees[0])
    st = StftRoundTrip(S, c.T, c.F, c.hop)
    d_in = _dev(K.batch_input(c), np.float32)
    p, r = _harmony(st, d_in, c.fs, c.keys, np.zeros((S, V), np.int32), None)
    tp, tr = st.track_pitch(d_in, c.fs, keys=list(c.keys))
    torch.cuda.synchronize()
    st.close()
    tp, tr = tp.cpu().numpy(), tr.cpu().numpy()
    assert np.any(tp > 0)
    for v in range(V):
        _same(p, r[:, v], tp, tr)


def test_the_python_mirror_builds_the_same_tables():
    from vocoderproject_amd import StftRoundTrip
    c = K.BY_NAME["unvoiced-u"]
    x = K.batch_input(c)
    st = StftRoundTrip(S, c.T, c.F, c.hop)
    d_in = _dev(x, np.float32)
    p, r = st.track_harmony(d_in, c.fs, K.degrees_of(c), keys=list(c.keys), unvoiced=K.unvoiced_of(c))
    p1, r1 = st.track_harmony(d_in, c.fs, [0, 2, -3], keys=list(c.keys))           # one row of degrees for all streams, the nominal intervals
    torch.cuda.synchronize()
    st.close()
    _same(p.cpu().numpy(), r.cpu().numpy(), *K.reference(c))
    nominal = HR.nominal_unvoiced([0, 2, -3], c.keys, S)
    assert nominal[0].tolist() == [1.0, 2.0 ** (3 / 12), 2.0 ** (-5 / 12)] and nominal[2].tolist() == [1.0, 2.0 ** (2 / 12), 2.0 ** (-3 / 12)]
    _same(p1.cpu().numpy(), r1.cpu().numpy(), *HR.track_harmony(x, c.fs, c.F, c.hop, np.array([0, 2, -3]), c.keys, nominal))


# ---- 2. vp_stft_harmonize_key --------------------------------------------------------------------------------------------------------------------
def test_harmonize_key_has_the_bits_of_its_two_calls():
    from vocoderproject_amd import StftRoundTrip
    c = K.BY_NAME["glide-v4"]
    V = 4
    st = StftRoundTrip(S, c.T, c.F, c.hop)
    d_in = _dev(K.batch_input(c), np.float32)
    d_key, d_deg, d_unv = _dev(c.keys, np.int32), _dev(K.degrees_of(c), np.int32), _dev(K.unvoiced_of(c), np.float64)
    d_gain, d_dry = _dev(np.linspace(0.4, 1.2, S * V).reshape(S, V), np.float64), _dev([0.5, 0.0, 1.0], np.float64)
    gp, gr = _Guarded((S, st.n_frames), torch.int32), _Guarded((S, V, st.n_frames), torch.float64)
    out = torch.full_like(d_in, float("nan"))
    rc = st.L.vp_stft_harmonize_key(st.h, d_in.data_ptr(), out.data_ptr(), c.fs, d_key.data_ptr(), V, d_deg.data_ptr(), d_unv.data_ptr(),
                                    d_gain.data_ptr(), d_dry.data_ptr(), gp.tab.data_ptr(), gr.tab.data_ptr(), _cur())
    assert rc == 0, (rc, st.L.vp_stft_last_error(st.h))
    p2, r2 = _harmony(st, d_in, c.fs, c.keys, K.degrees_of(c), K.unvoiced_of(c))
    out2 = torch.full_like(d_in, float("nan"))
    d_r2 = _dev(r2, np.float64)
    assert st.L.vp_stft_harmonize(st.h, d_in.data_ptr(), out2.data_ptr(), V, d_r2.data_ptr(), d_gain.data_ptr(), d_dry.data_ptr(), _cur()) == 0
    torch.cuda.synchronize()
    st.close()
    _same(gp.get(), gr.get(), p2, r2)                                               # its d_ratio holds the table
    _same(p2, r2, *K.reference(c))
    y, y2 = out.cpu().numpy(), out2.cpu().numpy()
    assert np.all(np.isfinite(y)) and np.array_equal(y.view(np.uint32), y2.view(np.uint32))


def test_harmonize_key_refuses_2048_point_frames_and_bad_arguments_with_nothing_written():
    from vocoderproject_amd import StftRoundTrip
    T = 4096
    d_in = torch.zeros((S, T), dtype=torch.float32, device="cuda")
    out = torch.full_like(d_in, 7.0)
    d_deg = _dev(np.zeros((S, 2)), np.int32)
    for F, hop in ((2048, 512), (1024, 256)):
        st = StftRoundTrip(S, T, F, hop)
        gp, gr = _Guarded((S, st.n_frames), torch.int32), _Guarded((S, 2, st.n_frames), torch.float64)
        key = lambda o=out, r=gr.tab, V=2, deg=d_deg: st.L.vp_stft_harmonize_key(  # noqa: E731
            st.h, d_in.data_ptr(), _ptr(o), 44100.0, None, V, _ptr(deg), None, None, None, gp.tab.data_ptr(), _ptr(r), _cur())
        if F == 2048:
            assert key() == VP_ERR_GEOMETRY and st.L.vp_stft_last_error(st.h).decode().startswith("harmonize: 2048-point frames are not built")
        else:
            assert key(o=None) == VP_ERR_INVALID_ARG and key(r=None) == VP_ERR_INVALID_ARG
            assert st.L.vp_stft_last_error(st.h).decode().startswith("harmonize key: null output or ratio table")
            for V in (0, 5):
                assert key(V=V) == VP_ERR_INVALID_ARG and "outside 1 .. 4" in st.L.vp_stft_last_error(st.h).decode()
            assert key(deg=None) == VP_ERR_INVALID_ARG and "null degree table" in st.L.vp_stft_last_error(st.h).decode()
            harm = lambda p, r: st.L.vp_stft_track_harmony(st.h, d_in.data_ptr(), 44100.0, None, 2, d_deg.data_ptr(), None, p, r, _cur())  # noqa: E731
            assert harm(None, None) == VP_ERR_INVALID_ARG and "both null" in st.L.vp_stft_last_error(st.h).decode()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool(torch.isnan(gr.tab).all()) and bool((gp.tab == GUARD_I).all())
        st.close()


# ---- 3. streaming ---------------------------------------------------------------------------------------------------------------------------------
def _tracker(hold=0, glide=1.0):
    from vocoderproject_amd import StreamingPitchTracker
    return StreamingPitchTracker(S, K.STREAM_N, K.STREAM_FS, K.STREAM_F, hold_blocks=hold, glide=glide)


def _voices(trk, d_blocks, d_key, d_deg, d_unv, V):
    """vp_pv_tracker_process_blocks_voices_device through the C ABI, guarded outputs -> (period, ratio) device-side holders."""
    n = d_blocks.shape[0]
    gp, gr = _Guarded((n, S), torch.int32), _Guarded((n, S, V), torch.float64)
    rc = trk.L.vp_pv_tracker_process_blocks_voices_device(trk.h, d_blocks.data_ptr(), _ptr(d_key), V, d_deg.data_ptr(), _ptr(d_unv), gp.tab.data_ptr(),
                                                          gr.tab.data_ptr(), n, _cur())
    assert rc == 0, rc
    return gp, gr


def _feed(trk, d_in, groups, d_key, d_deg, d_unv, V, first=0):
    outs, b = [], first
    for k in groups:
        outs.append(_voices(trk, d_in[b:b + k], d_key, d_deg, d_unv, V))
        b += k
    torch.cuda.synchronize()
    return np.concatenate([gp.get() for gp, _ in outs]), np.concatenate([gr.get() for _, gr in outs])


def _stream_tables(degrees=K.STREAM_DEGREES, unvoiced=K.STREAM_UNVOICED):
    return (_dev(K.stream_input(), np.float32), _dev(K.STREAM_KEYS, np.int32), _dev(degrees, np.int32),
            None if unvoiced is None else _dev(unvoiced, np.float64))


@pytest.mark.parametrize("hold,glide", K.STREAM_FOLLOW)
def test_streaming_equals_the_definition_in_every_grouping(hold, glide):
    want_p, want_r = K.stream_reference(hold, glide)
    assert np.all(want_p[:K.FIRST_DECISION] == 0) and np.all(want_p[K.FIRST_DECISION, [0, 2]] > 0)     # the first blocks (n_b < W) are unvoiced
    d_in, d_key, d_deg, d_unv = _stream_tables()
    for name, groups in K.STREAM_GROUPINGS.items():
        trk = _tracker(hold, glide)
        n0 = trk.debug_alloc_count()
        p, r = _feed(trk, d_in, groups, d_key, d_deg, d_unv, 3)
        assert trk.debug_alloc_count() == n0 and n0 > 0
        trk.close()
        try:
            _same(p, r, want_p, want_r)
        except AssertionError as e:
            raise AssertionError(f"grouping {name}: {e}") from None


def test_a_reset_of_one_stream_makes_it_a_fresh_stream_and_leaves_the_others():
    hold, glide, cut = 3, 0.5, 11
    want_p, want_r = K.stream_reference(hold, glide)
    x = K.stream_input()
    fresh_p, fresh_r = HSR.run(x[cut:], K.STREAM_FS, K.STREAM_F, np.asarray(K.STREAM_DEGREES, np.int32), K.STREAM_KEYS,
                               np.asarray(K.STREAM_UNVOICED), hold, glide)
    d_in, d_key, d_deg, d_unv = _stream_tables()
    trk = _tracker(hold, glide)
    p0, r0 = _feed(trk, d_in, [4, cut - 4], d_key, d_deg, d_unv, 3)
    trk.reset(1)
    p1, r1 = _feed(trk, d_in, [6, K.STREAM_BLOCKS - cut - 6], d_key, d_deg, d_unv, 3, first=cut)
    trk.close()
    p, r = np.concatenate([p0, p1]), np.concatenate([r0, r1])
    for s in (0, 2):
        _same(p[:, s], r[:, s], want_p[:, s], want_r[:, s])
    _same(p[:cut, 1], r[:cut, 1], want_p[:cut, 1], want_r[:cut, 1])
    _same(p[cut:, 1], r[cut:, 1], fresh_p[:, 1], fresh_r[:, 1])
    assert np.any(_bits(fresh_r[:, 1]) != _bits(want_r[cut:, 1]))                    # the reset shows


@pytest.mark.parametrize("hold,glide", K.STREAM_FOLLOW)
def test_degree_zero_and_unvoiced_one_equal_the_mono_call_on_a_twin_handle(hold, glide):
    d_in, d_key, d_deg, _ = _stream_tables(degrees=np.zeros((S, 3)), unvoiced=None)
    a, b = _tracker(hold, glide), _tracker(hold, glide)
    p, r = _feed(a, d_in, [5, 19], d_key, d_deg, _dev(np.ones((S, 3)), np.float64), 3)
    mp, mr = b.process_device(d_in, n_blocks=K.STREAM_BLOCKS, keys=list(K.STREAM_KEYS))
    torch.cuda.synchronize()
    a.close()
    b.close()
    for v in range(3):
        _same(p, r[:, :, v], mp.cpu().numpy(), mr.cpu().numpy())


def test_mono_and_voice_calls_alternate_on_one_handle_each_with_its_own_follow_state():
    """Blocks 0 .. 23 in spans that alternate between the two calls.  Ring and counter advance once per block, so every raw decision is the
    definition's; each call's follow state sees only its own spans: the voices' table equals the definition's follow stage run over the
    voices' spans alone (the state carried across the mono spans), and likewise the mono table."""
    import pv_track_stream_reference as SR
    hold, glide = 3, 0.5
    spans = [(0, 7, "v"), (7, 10, "m"), (10, 16, "v"), (16, 19, "m"), (19, 24, "v")]
    x = K.stream_input()
    deg, unv = np.asarray(K.STREAM_DEGREES, np.int32), np.asarray(K.STREAM_UNVOICED)
    # the definitions, fed every block (the raw decision needs all of them) but following only their own spans
    voices, mono = HSR.StreamVoices(S, K.STREAM_N, K.STREAM_FS, K.STREAM_F, hold, glide), SR.StreamTracker(S, K.STREAM_N, K.STREAM_FS, K.STREAM_F, hold, glide)
    want = []
    for b0, b1, kind in spans:
        if kind == "v":
            want.append(voices.process(x[b0:b1], deg, K.STREAM_KEYS, unv))
            keep = list(mono.state)
            mono.process(x[b0:b1], K.STREAM_KEYS)
            mono.state = keep
        else:
            want.append(mono.process(x[b0:b1], K.STREAM_KEYS))
            keep = [[t.copy(), c.copy(), a] for t, c, a in voices.state]
            voices.process(x[b0:b1], deg, K.STREAM_KEYS, unv)
            voices.state = keep
    d_in, d_key, d_deg, d_unv = _stream_tables()
    trk = _tracker(hold, glide)
    n0 = trk.debug_alloc_count()
    for (b0, b1, kind), (wp, wr) in zip(spans, want):
        if kind == "v":
            p, r = _feed(trk, d_in, [b1 - b0], d_key, d_deg, d_unv, 3, first=b0)
        else:
            mp, mr = trk.process_device(d_in[b0:b1], n_blocks=b1 - b0, keys=d_key)
            torch.cuda.synchronize()
            p, r = mp.cpu().numpy(), mr.cpu().numpy()
        try:
            _same(p, r, wp, wr)
        except AssertionError as e:
            raise AssertionError(f"span {b0}:{b1} {kind}: {e}") from None
    assert trk.debug_alloc_count() == n0
    trk.close()


def test_the_voice_count_may_change_from_call_to_call_and_unnamed_voices_keep_their_state():
    hold, glide = 3, 0.5
    x = K.stream_input()
    deg, unv = np.asarray(K.STREAM_DEGREES, np.int32), np.asarray(K.STREAM_UNVOICED)
    ref = HSR.StreamVoices(S, K.STREAM_N, K.STREAM_FS, K.STREAM_F, hold, glide)
    calls = [(0, 9, 3), (9, 15, 1), (15, 24, 3)]
    want = [ref.process(x[a:b], deg[:, :V], K.STREAM_KEYS, unv[:, :V]) for a, b, V in calls]
    d_in, d_key = _dev(x, np.float32), _dev(K.STREAM_KEYS, np.int32)
    trk = _tracker(hold, glide)
    for (a, b, V), (wp, wr) in zip(calls, want):
        p, r = _feed(trk, d_in, [b - a], d_key, _dev(deg[:, :V], np.int32), _dev(unv[:, :V], np.float64), V, first=a)
        _same(p, r, wp, wr)
    trk.close()


def test_null_outputs_advance_the_state_through_the_handle_s_scratch():
    hold, glide = 3, 0.5
    want_p, want_r = K.stream_reference(hold, glide)
    d_in, d_key, d_deg, d_unv = _stream_tables()
    trk = _tracker(hold, glide)
    gp = _Guarded((18, S), torch.int32)
    rc = trk.L.vp_pv_tracker_process_blocks_voices_device(trk.h, d_in.data_ptr(), d_key.data_ptr(), 3, d_deg.data_ptr(), d_unv.data_ptr(), gp.tab.data_ptr(),
                                                          None, 18, _cur())                 # 18 blocks: more than one scratch chunk at V = 3
    assert rc == 0
    p, r = _feed(trk, d_in, [6], d_key, d_deg, d_unv, 3, first=18)
    trk.close()
    assert np.array_equal(gp.get(), want_p[:18])
    _same(p, r, want_p[18:], want_r[18:])


def test_streaming_argument_errors_are_reported_before_the_device_is_touched():
    from vocoderproject_amd import HarmonizerStream, StreamingPitchTracker
    trk = _tracker()
    d_in, d_key, d_deg, d_unv = _stream_tables()
    gp, gr = _Guarded((2, S), torch.int32), _Guarded((2, S, 3), torch.float64)
    f = trk.L.vp_pv_tracker_process_blocks_voices_device
    ok = [trk.h, d_in.data_ptr(), None, 3, d_deg.data_ptr(), None, gp.tab.data_ptr(), gr.tab.data_ptr(), 2, _cur()]
    for i, v in ((0, None), (1, None), (3, 0), (3, 5), (4, None), (8, 0)):
        bad = list(ok)
        bad[i] = v
        assert f(*bad) == VP_ERR_INVALID_ARG, i
    bad = list(ok)
    bad[6] = bad[7] = None
    assert f(*bad) == VP_ERR_INVALID_ARG
    hz = HarmonizerStream(S, K.STREAM_N, 3)
    other = StreamingPitchTracker(S + 1, K.STREAM_N, K.STREAM_FS)
    out = torch.full((2, S, K.STREAM_N), 7.0, dtype=torch.float32, device="cuda")
    g = hz.L.vp_hz_autoharm_blocks_device
    ok = [hz.h, trk.h, d_in.data_ptr(), out.data_ptr(), None, d_deg.data_ptr(), None, None, None, gp.tab.data_ptr(), gr.tab.data_ptr(), 2, _cur()]
    for i in (0, 1, 2, 3, 5, 10):
        bad = list(ok)
        bad[i] = None
        assert g(*bad) == VP_ERR_INVALID_ARG, i
    bad = list(ok)
    bad[1] = other.h
    assert g(*bad) == VP_ERR_GEOMETRY
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool(torch.isnan(gr.tab).all()) and bool((gp.tab == GUARD_I).all())
    for h in (hz, other, trk):
        h.close()


# ---- 4. vp_hz_autoharm_blocks_device ----------------------------------------------------------------------------------------------------------------
def test_autoharm_has_the_bits_of_its_two_calls_and_of_the_one_shot_along_its_table():
    """The streaming pair against (a) the tracker call followed by vp_hz_process_blocks_device on twin handles, bit for bit, and (b)
    vp_stft_harmonize_key's harmonizer half: the one-shot vp_stft_harmonize along the STREAMING table (a frame takes the block in which its
    last sample arrives), delayed by L = F - gcd(N, hop), over every sample emitted.
    Where the two trackers agree: the streaming decision of block b reads the W = 1465 samples that end at (b + 1) N, the batch decision
    of frame f the W samples that start at f hop.  With N = hop = 256 the two windows would coincide where f hop + W = (b + 1) N, and W is
    no multiple of 256: no frame's window is a block's.  So vp_stft_harmonize_key's own table differs from the streaming one wherever the
    pitch moves (stream 2's glide) or stops (stream 1), and equality with vp_stft_harmonize_key's output is asserted on the harmonizer
    half alone; on stream 0 (a steady period) both trackers return 199 on every voiced decision, which is asserted too."""
    from vocoderproject_amd import HarmonizerStream, StftRoundTrip
    N, hop, F, V, nb = K.STREAM_N, 256, K.STREAM_F, 3, K.STREAM_BLOCKS
    x = K.stream_input()
    d_in, d_key, d_deg, d_unv = _stream_tables()
    d_gain, d_dry = _dev(np.linspace(0.5, 1.0, S * V).reshape(S, V), np.float64), _dev([0.5, 0.0, 1.0], np.float64)
    hz, trk, hz2, trk2 = HarmonizerStream(S, N, V, hop=hop), _tracker(3, 0.5), HarmonizerStream(S, N, V, hop=hop), _tracker(3, 0.5)
    out, out2 = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    tabs, b = [], 0
    for k in (1, 7, 16):
        gp, gr = _Guarded((k, S), torch.int32), _Guarded((k, S, V), torch.float64)
        rc = hz.L.vp_hz_autoharm_blocks_device(hz.h, trk.h, d_in[b:b + k].data_ptr(), out[b:b + k].data_ptr(), d_key.data_ptr(), d_deg.data_ptr(),
                                               d_unv.data_ptr(), d_gain.data_ptr(), d_dry.data_ptr(), gp.tab.data_ptr(), gr.tab.data_ptr(), k, _cur())
        assert rc == 0, rc
        gp2, gr2 = _voices(trk2, d_in[b:b + k], d_key, d_deg, d_unv, V)
        assert hz2.L.vp_hz_process_blocks_device(hz2.h, d_in[b:b + k].data_ptr(), out2[b:b + k].data_ptr(), gr2.tab.data_ptr(), d_gain.data_ptr(),
                                                 d_dry.data_ptr(), k, _cur()) == 0
        tabs.append((gp, gr, gp2, gr2))
        b += k
    torch.cuda.synchronize()
    L = hz.latency
    for h in (hz, trk, hz2, trk2):
        h.close()
    p, r = np.concatenate([t[0].get() for t in tabs]), np.concatenate([t[1].get() for t in tabs])
    _same(p, r, np.concatenate([t[2].get() for t in tabs]), np.concatenate([t[3].get() for t in tabs]))
    _same(p, r, *K.stream_reference(3, 0.5))
    y, y2 = out.cpu().numpy(), out2.cpu().numpy()
    assert np.all(np.isfinite(y)) and np.array_equal(y.view(np.uint32), y2.view(np.uint32))
    # (b) the one-shot call along the streaming table
    rows = x.transpose(1, 0, 2).reshape(S, nb * N)
    T = rows.shape[1]
    per_frame = HC.per_frame(r, N, hop, T)
    st = StftRoundTrip(S, T, F, hop)
    d_rows, one = _dev(rows, np.float32), torch.full((S, T), float("nan"), dtype=torch.float32, device="cuda")
    d_tab = _dev(per_frame, np.float64)
    assert st.L.vp_stft_harmonize(st.h, d_rows.data_ptr(), one.data_ptr(), V, d_tab.data_ptr(), d_gain.data_ptr(), d_dry.data_ptr(), _cur()) == 0
    bp, _ = st.track_harmony(d_rows, K.STREAM_FS, np.asarray(K.STREAM_DEGREES, np.int32), keys=list(K.STREAM_KEYS), unvoiced=np.asarray(K.STREAM_UNVOICED))
    torch.cuda.synchronize()
    st.close()
    y1, ys = one.cpu().numpy(), y.transpose(1, 0, 2).reshape(S, T)
    assert L == F - N
    n = min(per_frame.shape[2] * hop, T - L)                                        # finished one-shot samples that the stream has emitted
    assert n > 2 * F and np.all(ys[:, :L] == 0)
    for s in range(S):
        assert np.array_equal(ys[s, L:L + n], y1[s, :n]), (s, np.abs(ys[s, L:L + n] - y1[s, :n]).max())
    bp = bp.cpu().numpy()
    assert np.all(bp[0] == K.P_A3) and np.all(p[K.FIRST_DECISION:, 0] == K.P_A3)


# ---- 5. behaviour -----------------------------------------------------------------------------------------------------------------------------------
def test_a_sharp_a3_in_c_major_gets_its_third_and_fifth_from_the_key():
    """Tolerance: twice the distance the NumPy harmonizer leaves along the definition's table (0.0807 Hz, profiles/pv_harmkey_quality.txt)
    or one bin of this check's own transform (5.38 Hz), whichever is larger."""
    from vocoderproject_amd import StftRoundTrip
    st = StftRoundTrip(1, K.CHORD_T, 1024, 256)
    d_in = _dev(K.chord_input(), np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    period, ratio = st.harmonize(d_in, d_out, degrees=list(K.CHORD_DEGREES), sample_rate=K.CHORD_FS, keys=K.CHORD_KEY, gains=[1.0, 1.0], dry=0.0)
    torch.cuda.synchronize()
    st.close()
    y = d_out.cpu().numpy()[0]
    assert np.all(np.isfinite(y)) and np.all(period.cpu().numpy() == K.P_A3)
    got, want, tol = K.chord_peaks(y), K.chord_notes(), K.chord_tolerance()
    print(f"PVHARMKEY chord: maxima {got[0]:.3f}, {got[1]:.3f} Hz; the table's notes {want[0]:.3f}, {want[1]:.3f} Hz; tolerance {tol:.3f} Hz")
    assert abs(want[0] - 277.18) < 0.01 and abs(want[1] - 329.63) < 0.01
    for g, w in zip(got, want):
        assert abs(g - w) <= tol, (got, want, tol)
