"""The fine pitch trackers on the GPU (include/vp_amd.h VP_TRACK_FINE, vp_stft_track_pitch_fine, vp_pv_tracker_process_blocks_fine_device;
kernels vp_k_yin_track_fine, vp_k_yin_track_stream_fine, vp_k_yin_track_voices_fine, vp_k_yin_track_voices_stream_fine of
csrc/vp_track_fine_kernels.inc): period, refined period and ratio bit-equal to tests/pv_track_fine_reference.py on every frame of every
case of tests/pv_track_fine_cases.py (whose branch coverage tests/test_pv_track_fine_reference_cpu.py gates); the mode switch on one
handle; the composed calls under VP_TRACK_FINE against their two parts; the streaming tracker against
tests/pv_track_fine_stream_reference.py in three groupings, with a reset, a mode change, hold and glide, mono and voices; degenerate rows;
argument errors; allocations; and one end-to-end figure."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_harmkey_reference as HR  # noqa: E402
import pv_track_fine_cases as FC  # noqa: E402
import pv_track_fine_reference as FR  # noqa: E402
import pv_track_fine_stream_reference as FSR  # noqa: E402
import pv_track_reference as R  # noqa: E402
import pv_track_stream_reference as SR  # noqa: E402

pytestmark = pytest.mark.gpu

PERIOD_SENTINEL = -777
VP_ERR_INVALID_ARG = -1
INTEGER, FINE = 0, 1


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, names=("period", "period_fine", "ratio")):
    """Integer tables equal, double tables bit-equal; the first difference is what the assertion shows."""
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.argwhere(g != w) if g.dtype.kind == "i" else np.argwhere(_bits(g) != _bits(w))
        assert bad.size == 0, (name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _tables(shape, period=True, fine=True, ratio=True):
    return (torch.full(shape, PERIOD_SENTINEL, dtype=torch.int32, device="cuda") if period else None,
            torch.full(shape, float("nan"), dtype=torch.float64, device="cuda") if fine else None,
            torch.full(shape, float("nan"), dtype=torch.float64, device="cuda") if ratio else None)


def _track_fine(st, d_in, fs, d_key=None, period=True, fine=True, ratio=True):
    """vp_stft_track_pitch_fine through the C ABI with sentinel-filled outputs -> (rc, period, period_fine, ratio), NumPy or None."""
    d_p, d_f, d_r = _tables((st.S, st.n_frames), period, fine, ratio)
    rc = st.L.vp_stft_track_pitch_fine(st.h, d_in.data_ptr(), float(fs), _ptr(d_key), _ptr(d_p), _ptr(d_f), _ptr(d_r), _cur())
    torch.cuda.synchronize()
    return (rc,) + tuple(None if t is None else t.cpu().numpy() for t in (d_p, d_f, d_r))


def _track(st, d_in, fs, d_key=None):
    """vp_stft_track_pitch (whatever the handle's mode) -> (period, ratio)."""
    d_p, _, d_r = _tables((st.S, st.n_frames), fine=False)
    assert st.L.vp_stft_track_pitch(st.h, d_in.data_ptr(), float(fs), _ptr(d_key), d_p.data_ptr(), d_r.data_ptr(), _cur()) == 0
    torch.cuda.synchronize()
    return d_p.cpu().numpy(), d_r.cpu().numpy()


def _set_mode(st, mode):
    assert st.L.vp_stft_set_track_mode(st.h, mode) == 0 and st.L.vp_stft_get_track_mode(st.h) == mode


# ---- 1. bit equality with the definition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.CASES, ids=FC.case_id)
def test_period_fine_period_and_ratio_equal_the_definition_bit_for_bit(c):
    from vocoderproject_amd import StftRoundTrip
    want = FC.reference(c)[:3]
    st = StftRoundTrip(FC.N_STREAMS, FC.length(c), c.F, c.hop)
    rc, p, pf, r = _track_fine(st, _dev(FC.batch_input(c), np.float32), c.fs, d_key=None if c.keys is None else _dev(c.keys, np.int32))
    st.close()
    assert rc == 0
    assert not np.any(p == PERIOD_SENTINEL) and not np.any(np.isnan(pf)) and not np.any(np.isnan(r))       # every slot was written
    _same((p, pf, r), want)


def test_any_output_may_be_null_but_not_all_three_and_python_returns_the_third_table():
    from vocoderproject_amd import StftRoundTrip
    c = FC.THREE_BY_THREE
    want = FC.reference(c)[:3]
    st = StftRoundTrip(FC.N_STREAMS, FC.length(c), c.F, c.hop)
    d_in, d_key = _dev(FC.batch_input(c), np.float32), _dev(c.keys, np.int32)
    for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)):
        rc, *got = _track_fine(st, d_in, c.fs, d_key, *map(bool, keep))
        assert rc == 0
        _same([g for g in got if g is not None], [w for w, k in zip(want, keep) if k], [n for n, k in zip(("period", "period_fine", "ratio"), keep) if k])
    rc, *_ = _track_fine(st, d_in, c.fs, d_key, False, False, False)
    assert rc == VP_ERR_INVALID_ARG and "null" in st.L.vp_stft_last_error(st.h).decode()
    p, r, pf = st.track_pitch(d_in, c.fs, keys=list(c.keys), with_fine_period=True)
    torch.cuda.synchronize()
    assert not st.track_fine                                                        # the fine entry does not change the mode
    st.close()
    _same((p.cpu().numpy(), pf.cpu().numpy(), r.cpu().numpy()), want)


# ---- 2. the mode switch on one handle -------------------------------------------------------------------------------------------------------
def _mode_input():
    c = FC.BY_NAME["near-fs44100-F1024-clamp-3"]
    x = np.concatenate([FC.batch_input(c), FC.batch_input(FC.BY_NAME["left-fs44100-F1024-clamp"])[:1], FC.batch_input(FC.NULL_KEYS)[:2]])
    return x, (12, 0, 7, 12, 0, 7), c


def test_the_mode_selects_the_tracker_of_every_batch_entry_and_switches_back():
    from vocoderproject_amd import StftRoundTrip
    x, keys, c = _mode_input()
    fs, S = c.fs, x.shape[0]
    deg = np.asarray([0, 2, -3], np.int32)
    unv = HR.nominal_unvoiced(deg, keys, S)
    int_p, int_r = R.track(x, fs, c.F, c.hop, keys)
    fine_p, fine_f, fine_r = FR.track_fine(x, fs, c.F, c.hop, keys)
    int_h, fine_h = HR.track_harmony(x, fs, c.F, c.hop, deg, keys, unv)[1], FR.track_harmony_fine(x, fs, c.F, c.hop, deg, keys, unv)[1]
    assert not np.array_equal(_bits(int_r), _bits(fine_r)) and not np.array_equal(_bits(int_h), _bits(fine_h))
    st = StftRoundTrip(S, x.shape[1], c.F, c.hop)
    d_in, d_key = _dev(x, np.float32), _dev(keys, np.int32)
    assert st.L.vp_stft_get_track_mode(st.h) == INTEGER
    for mode, (wp, wr, wh) in ((INTEGER, (int_p, int_r, int_h)), (FINE, (fine_p, fine_r, fine_h)), (INTEGER, (int_p, int_r, int_h))):
        _set_mode(st, mode)
        _same(_track(st, d_in, fs, d_key), (wp, wr), ("period", "ratio"))
        hp, hr = st.track_harmony(d_in, fs, deg, keys=list(keys))
        out, out_f, out_h = (torch.full_like(d_in, float("nan")) for _ in range(3))
        ap, ar = st.autotune(d_in, out, fs, keys=list(keys))
        fp, fr = st.autotune(d_in, out_f, fs, keys=list(keys), formant_semitones=0.0)
        kp, kr = st.harmonize(d_in, out_h, degrees=deg, keys=list(keys), sample_rate=fs)
        # the parts along this mode's tables: the curve, formant and harmonizer calls do not track
        d_wr, d_wh = _dev(wr, np.float64), _dev(wh, np.float64)
        parts, parts_f, parts_h = (torch.full_like(d_in, float("nan")) for _ in range(3))
        st.pitch_shift_curve(d_in, parts, d_ratio=d_wr)
        st.pitch_shift_formant(d_in, parts_f, d_ratio=d_wr, formant_semitones=0.0)
        st.harmonize(d_in, parts_h, d_ratio=d_wh)
        torch.cuda.synchronize()
        _same((hp.cpu().numpy(), hr.cpu().numpy()), (wp, wh), ("period", "harmony"))
        _same((ap.cpu().numpy(), ar.cpu().numpy()), (wp, wr), ("period", "autotune ratio"))
        _same((fp.cpu().numpy(), fr.cpu().numpy()), (wp, wr), ("period", "autotune formant ratio"))
        _same((kp.cpu().numpy(), kr.cpu().numpy()), (wp, wh), ("period", "harmonize key ratio"))
        for name, a, b in (("autotune", out, parts), ("autotune formant", out_f, parts_f), ("harmonize key", out_h, parts_h)):
            ya, yb = a.cpu().numpy(), b.cpu().numpy()
            assert np.all(np.isfinite(ya)) and np.abs(ya).max() > 0.1 and np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), (mode, name)
        assert np.array_equal(_bits(hr.cpu().numpy()[:, 0]), _bits(wr))             # a voice at degree 0 has the mono ratio's bits
        # the fine entry refines whatever the mode, and under VP_TRACK_FINE vp_stft_track_pitch equals it
        rc, p, pf, r = _track_fine(st, d_in, fs, d_key)
        assert rc == 0
        _same((p, pf, r), (fine_p, fine_f, fine_r))
    for bad in (2, -1, 77):
        assert st.L.vp_stft_set_track_mode(st.h, bad) == VP_ERR_INVALID_ARG and st.L.vp_stft_get_track_mode(st.h) == INTEGER
    st.set_track_mode(True)
    assert st.track_fine
    st.set_track_mode(False)
    assert not st.track_fine
    st.close()


# ---- 3. composed calls under VP_TRACK_FINE have the bits of their two parts ------------------------------------------------------------------
def test_composed_batch_calls_have_the_bits_of_their_two_parts():
    from vocoderproject_amd import StftRoundTrip
    x, keys, c = _mode_input()
    fs, S = c.fs, x.shape[0]
    st = StftRoundTrip(S, x.shape[1], c.F, c.hop)
    d_in = _dev(x, np.float32)
    _set_mode(st, FINE)
    p, r = st.track_pitch(d_in, fs, keys=list(keys))
    want = FR.track_fine(x, fs, c.F, c.hop, keys)
    _same((p.cpu().numpy(), r.cpu().numpy()), (want[0], want[2]), ("period", "ratio"))
    # autotune = fine track + curve; autotune_formant = fine track + formant call
    parts, out = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    st.pitch_shift_curve(d_in, parts, d_ratio=r)
    ap, ar = st.autotune(d_in, out, fs, keys=list(keys))
    parts_f, out_f = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    st.pitch_shift_formant(d_in, parts_f, d_ratio=r, formant_semitones=0.0)
    fp, fr = st.autotune(d_in, out_f, fs, keys=list(keys), formant_semitones=0.0)
    # harmonize_key = fine track_harmony + harmonize
    deg = np.asarray([0, 2, 4], np.int32)
    hp, hr = st.track_harmony(d_in, fs, deg, keys=list(keys))
    parts_h, out_h = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    st.harmonize(d_in, parts_h, d_ratio=hr)
    st.harmonize(d_in, out_h, degrees=deg, keys=list(keys), sample_rate=fs)
    torch.cuda.synchronize()
    st.close()
    for a, b in ((ar, r), (fr, r)):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    assert np.array_equal(_bits(hr.cpu().numpy()[:, 0]), _bits(r.cpu().numpy()))
    _same((hp.cpu().numpy(), hr.cpu().numpy()), FR.track_harmony_fine(x, fs, c.F, c.hop, deg, keys, HR.nominal_unvoiced(deg, keys, S)), ("period", "harmony"))
    for a, b in ((out, parts), (out_f, parts_f), (out_h, parts_h)):
        ya, yb = a.cpu().numpy(), b.cpu().numpy()
        assert np.all(np.isfinite(ya)) and np.abs(ya).max() > 0.1 and np.array_equal(ya.view(np.uint32), yb.view(np.uint32))


# ---- 4. streaming ---------------------------------------------------------------------------------------------------------------------------
def _tracker(c, hold=None, glide=None):
    from vocoderproject_amd import StreamingPitchTracker
    return StreamingPitchTracker(len(c.signals), c.N, c.fs, c.F, hold_blocks=c.hold if hold is None else hold, glide=c.glide if glide is None else glide)


def _stream_fine(trk, d_blocks, d_key, fine=True):
    n = d_blocks.shape[0]
    d_p, d_f, d_r = _tables((n, trk.S), fine=fine)
    rc = trk.L.vp_pv_tracker_process_blocks_fine_device(trk.h, d_blocks.data_ptr(), _ptr(d_key), d_p.data_ptr(), _ptr(d_f), d_r.data_ptr(), n, _cur())
    assert rc == 0
    return d_p, d_f, d_r


def _stream_mono(trk, d_blocks, d_key):
    n = d_blocks.shape[0]
    d_p, _, d_r = _tables((n, trk.S), fine=False)
    assert trk.L.vp_pv_tracker_process_blocks_device(trk.h, d_blocks.data_ptr(), _ptr(d_key), d_p.data_ptr(), d_r.data_ptr(), n, _cur()) == 0
    return d_p, d_r


def _cat(outs):
    torch.cuda.synchronize()
    got = tuple(torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(len(outs[0])))
    assert not np.any(got[0] == PERIOD_SENTINEL) and not any(np.any(np.isnan(g)) for g in got[1:])
    return got


def _feed(call, d_in, groups):
    outs, b = [], 0
    for k in groups:
        outs.append(call(d_in[b:b + k]))
        b += k
    return _cat(outs)


@pytest.mark.parametrize("c", FC.STREAM_CASES, ids=lambda c: c.name)
def test_streaming_equals_the_definition_in_three_groupings(c):
    want = FC.stream_reference(c)
    fd = -(-SR.window_len(c.fs, c.F) // c.N) - 1
    assert 0 < fd < c.n_blocks - 5 and np.all(want[0][:fd] == 0) and np.all(want[1][:fd] == 0.0) and np.any(want[0][fd] > 0)   # the ring fills inside the run
    d_in, d_key = _dev(FC.stream_input(c), np.float32), _dev(c.keys, np.int32)
    for name, groups in FC.stream_groupings(c).items():
        trk = _tracker(c)
        n0 = trk.debug_alloc_count()
        got = _feed(lambda blk: _stream_fine(trk, blk, d_key), d_in, groups)
        assert trk.debug_alloc_count() == n0 and not trk.fine                       # the fine entry does not change the mode
        trk.close()
        try:
            _same(got, want)
        except AssertionError as e:
            raise AssertionError(f"{c.name} grouping {name}: {e}") from None
    # under VP_TRACK_FINE the plain call gives the same period and ratio; without a fine table too
    trk = _tracker(c)
    trk.set_fine(True)
    got = _feed(lambda blk: _stream_mono(trk, blk, d_key), d_in, FC.stream_groupings(c)["mixed"])
    trk.close()
    _same(got, (want[0], want[2]), ("period", "ratio"))
    trk = _tracker(c)
    got = _feed(lambda blk: tuple(t for t in _stream_fine(trk, blk, d_key, fine=False) if t is not None), d_in, [c.n_blocks])
    trk.close()
    _same(got, (want[0], want[2]), ("period", "ratio"))


def test_a_reset_of_one_stream_leaves_its_neighbours_bits():
    c = FC.STREAM_CASES[1]
    x = FC.stream_input(c)
    d_in, d_key = _dev(x, np.float32), _dev(c.keys, np.int32)
    cut, s = 13, 2
    trk = _tracker(c)
    a = _stream_fine(trk, d_in[:cut], d_key)
    assert trk.L.vp_pv_tracker_reset(trk.h, s) == 0
    b = _stream_fine(trk, d_in[cut:], d_key)
    got = _cat([a, b])
    trk.close()
    want = FC.stream_reference(c)
    ref = FSR.FineStreamTracker(x.shape[1], c.N, c.fs, c.F, c.hold, c.glide)
    p1, r1 = ref.process(x[:cut], c.keys)
    f1 = ref.period_fine
    ref.reset(s)
    p2, r2 = ref.process(x[cut:], c.keys)
    mine = (np.concatenate([p1, p2]), np.concatenate([f1, ref.period_fine]), np.concatenate([r1, r2]))
    others = [k for k in range(x.shape[1]) if k != s]
    _same([g[:, others] for g in got], [w[:, others] for w in want])
    _same(got, mine)
    assert np.all(mine[0][cut:cut + 5, s] == 0) and np.any(want[0][cut:cut + 5, s] > 0)   # the reset stream fills its ring again


@pytest.mark.parametrize("hold,glide", [(0, 1.0), (8, 0.5)])
def test_a_mode_change_between_two_calls_changes_only_what_follows(hold, glide):
    c = FC.STREAM_CASES[2]
    x = FC.stream_input(c)
    d_in, d_key = _dev(x, np.float32), _dev(c.keys, np.int32)
    groups, modes = [4, 3, 3], [False, True, False]
    trk = _tracker(c, hold, glide)
    outs, b = [], 0
    for k, m in zip(groups, modes):
        trk.set_fine(m)
        assert trk.fine == m
        outs.append(_stream_mono(trk, d_in[b:b + k], d_key))
        b += k
    got = _cat(outs)
    for bad in (2, -1):
        assert trk.L.vp_pv_tracker_set_mode(trk.h, bad) == VP_ERR_INVALID_ARG and not trk.fine
    trk.close()
    wp, _, wr = FSR.run(x, c.fs, c.F, c.keys, hold, glide, groups=groups, fine=modes)
    _same(got, (wp, wr), ("period", "ratio"))
    ip, ir = SR.run(x, c.fs, c.F, c.keys, hold, glide)
    assert np.array_equal(_bits(got[1][:4]), _bits(ir[:4])) and not np.array_equal(_bits(got[1][4:7]), _bits(ir[4:7]))


def _voice_tables(c, V):
    S = len(c.signals)
    deg = np.asarray([[0, 2, -3][:V]] * S, np.int32)
    return deg, HR.nominal_unvoiced(deg, c.keys, S)


def _stream_voices(trk, d_blocks, d_key, d_deg, d_unv, V):
    """vp_pv_tracker_process_blocks_voices_device through the C ABI with sentinel-filled outputs -> (period, ratio), device tensors."""
    n = d_blocks.shape[0]
    d_p = torch.full((n, trk.S), PERIOD_SENTINEL, dtype=torch.int32, device="cuda")
    d_r = torch.full((n, trk.S, V), float("nan"), dtype=torch.float64, device="cuda")
    assert trk.L.vp_pv_tracker_process_blocks_voices_device(trk.h, d_blocks.data_ptr(), d_key.data_ptr(), V, d_deg.data_ptr(), d_unv.data_ptr(),
                                                            d_p.data_ptr(), d_r.data_ptr(), n, _cur()) == 0
    return d_p, d_r


_VREF = {}


def _voices_reference(c, V):
    """(period [n][S], followed ratio [n][S][V]) of the case's voices under the fine mode in one call, computed once."""
    if (c.name, V) not in _VREF:
        deg, unv = _voice_tables(c, V)
        out = FSR.FineStreamVoices(len(c.signals), c.N, c.fs, c.F, c.hold, c.glide).process(FC.stream_input(c), deg, c.keys, unv)
        for a in out:
            a.setflags(write=False)
        _VREF[c.name, V] = out
    return _VREF[c.name, V]


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("c", FC.STREAM_CASES, ids=lambda c: c.name)
def test_streaming_voices_equal_the_definition_in_three_groupings(c, V):
    """N = 64, 256 and 1000 (the gather's three step patterns), hold 0 / 8 and glide 1 / 0.5 as the cases carry them, V = 1 and 3."""
    want = _voices_reference(c, V)
    deg, unv = _voice_tables(c, V)
    d_in, d_key, d_deg, d_unv = _dev(FC.stream_input(c), np.float32), _dev(c.keys, np.int32), _dev(deg, np.int32), _dev(unv, np.float64)
    fd = -(-SR.window_len(c.fs, c.F) // c.N) - 1
    assert np.all(want[0][:fd] == 0) and np.any(want[0][fd] > 0)                    # the ring fills inside the run
    for name, groups in FC.stream_groupings(c).items():
        trk = _tracker(c)
        trk.set_fine(True)
        n0 = trk.debug_alloc_count()
        got = _feed(lambda blk: _stream_voices(trk, blk, d_key, d_deg, d_unv, V), d_in, groups)
        assert trk.debug_alloc_count() == n0
        trk.close()
        try:
            _same(got, want, ("period", "voices"))
        except AssertionError as e:
            raise AssertionError(f"{c.name} V {V} grouping {name}: {e}") from None
    mono = FC.stream_reference(c)
    assert np.array_equal(want[0], mono[0]) and np.array_equal(_bits(want[1][:, :, 0]), _bits(mono[2]))   # degree 0: the mono fine table


@pytest.mark.parametrize("V", [1, 3])
def test_a_reset_of_one_stream_leaves_its_neighbours_voices(V):
    c = FC.STREAM_CASES[1]
    x = FC.stream_input(c)
    S = x.shape[1]
    deg, unv = _voice_tables(c, V)
    d_in, d_key, d_deg, d_unv = _dev(x, np.float32), _dev(c.keys, np.int32), _dev(deg, np.int32), _dev(unv, np.float64)
    cut, s = 13, 2
    trk = _tracker(c)
    trk.set_fine(True)
    a = _stream_voices(trk, d_in[:cut], d_key, d_deg, d_unv, V)
    assert trk.L.vp_pv_tracker_reset(trk.h, s) == 0
    b = _stream_voices(trk, d_in[cut:], d_key, d_deg, d_unv, V)
    got = _cat([a, b])
    trk.close()
    ref = FSR.FineStreamVoices(S, c.N, c.fs, c.F, c.hold, c.glide)
    p1, r1 = ref.process(x[:cut], deg, c.keys, unv)
    ref.reset(s)
    p2, r2 = ref.process(x[cut:], deg, c.keys, unv)
    mine = (np.concatenate([p1, p2]), np.concatenate([r1, r2]))
    want = _voices_reference(c, V)
    others = [k for k in range(S) if k != s]
    _same([g[:, others] for g in got], [w[:, others] for w in want], ("period", "voices"))   # the neighbours' bits
    _same(got, mine, ("period", "voices"))
    assert np.all(mine[0][cut:cut + 5, s] == 0) and np.any(want[0][cut:cut + 5, s] > 0)      # the reset stream fills its ring again


@pytest.mark.parametrize("V", [1, 3])
def test_a_mode_change_between_two_voices_calls_changes_only_what_follows(V):
    c = FC.STREAM_CASES[1]
    x = FC.stream_input(c)
    S = x.shape[1]
    deg, unv = _voice_tables(c, V)
    d_in, d_key, d_deg, d_unv = _dev(x, np.float32), _dev(c.keys, np.int32), _dev(deg, np.int32), _dev(unv, np.float64)
    groups = FC.stream_groupings(c)["mixed"]
    ref = FSR.FineStreamVoices(S, c.N, c.fs, c.F, c.hold, c.glide)
    trk = _tracker(c)
    outs, wants, b = [], [], 0
    for i, k in enumerate(groups):
        trk.set_fine(i != 4)                                                        # one call in the integer mode in the middle
        ref.fine = trk.fine
        outs.append(_stream_voices(trk, d_in[b:b + k], d_key, d_deg, d_unv, V))
        wants.append(ref.process(x[b:b + k], deg, c.keys, unv))
        b += k
    got = _cat(outs)
    trk.close()
    _same(got, (np.concatenate([w[0] for w in wants]), np.concatenate([w[1] for w in wants])), ("period", "voices"))
    first, whole = sum(groups[:4]), _voices_reference(c, V)
    assert np.array_equal(_bits(got[1][:first]), _bits(whole[1][:first])) and not np.array_equal(_bits(got[1][first:]), _bits(whole[1][first:]))


def test_streaming_compositions_have_the_bits_of_their_two_parts():
    from vocoderproject_amd import HarmonizerStream, PhaseVocoderStream
    c = FC.STREAM_CASES[1]
    x = FC.stream_input(c)
    S, n = x.shape[1], x.shape[0]
    d_in = _dev(x, np.float32)
    keys = list(c.keys)
    deg = np.asarray([0, 2, 4], np.int32)
    groups, modes = (7, 5, n - 12), (False, True, False)                            # integer, fine, integer: the ring is full from block 5 on
    want = FSR.run(x, c.fs, c.F, c.keys, c.hold, c.glide, groups=list(groups), fine=list(modes))
    whole_int, whole_fine = SR.run(x, c.fs, c.F, c.keys, c.hold, c.glide), FC.stream_reference(c)
    assert not np.array_equal(_bits(want[2]), _bits(whole_int[1])) and not np.array_equal(_bits(want[2]), _bits(whole_fine[2]))
    for kind in ("curve", "formant", "harm"):
        outs = []
        for composed in (True, False):
            trk = _tracker(c)
            sh = HarmonizerStream(S, c.N, 3, hop=256) if kind == "harm" else PhaseVocoderStream(S, c.N, 256)
            out = torch.full_like(d_in, float("nan"))
            tabs, b = [], 0
            for k, m in zip(groups, modes):
                trk.set_fine(m)
                i, o = d_in[b:b + k], out[b:b + k]
                if kind == "harm":
                    if composed:
                        p, r = sh.autoharm_device(trk, i, o, deg, n_blocks=k, keys=keys)
                    else:
                        p, r = trk.process_voices_device(i, deg, n_blocks=k, keys=keys)
                        sh.process_device(i, o, n_blocks=k, d_ratio=r)
                else:
                    fm = {"formant_semitones": 0.0} if kind == "formant" else {}
                    if composed:
                        p, r = sh.autotune_device(trk, i, o, n_blocks=k, keys=keys, **fm)
                    else:
                        p, r = trk.process_device(i, n_blocks=k, keys=keys)
                        sh.process_device(i, o, n_blocks=k, d_ratio=r, **fm)
                tabs.append((p, r))
                b += k
            torch.cuda.synchronize()
            trk.close()
            sh.close()
            outs.append((out.cpu().numpy(), torch.cat([t[0] for t in tabs]).cpu().numpy(), torch.cat([t[1] for t in tabs]).cpu().numpy()))
        (ya, pa, ra), (yb, pb, rb) = outs
        assert np.all(np.isfinite(ya)) and np.abs(ya).max() > 0.05, kind
        assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)) and np.array_equal(pa, pb) and np.array_equal(_bits(ra), _bits(rb)), kind
        assert np.array_equal(pa, want[0]) and np.array_equal(_bits(ra[:, :, 0] if kind == "harm" else ra), _bits(want[2])), kind


# ---- 5. degenerate rows, argument errors, allocations -----------------------------------------------------------------------------------------
def test_degenerate_rows_stay_finite_and_unvoiced():
    from vocoderproject_amd import StftRoundTrip
    fs, F, hop = 44100.0, 1024, 256
    T = F + R.tau_max(fs) + 3 * hop + 17
    x = np.zeros((5, T), np.float32)
    x[1] = 0.5
    x[2], x[3] = 1e30, -1e30
    x[4, 900] = 1.0
    st = StftRoundTrip(5, T, F, hop)
    rc, p, pf, r = _track_fine(st, _dev(x, np.float32), fs)
    st.close()
    assert rc == 0 and np.all(p == 0) and np.all(pf == 0.0) and np.all(r == 1.0)
    _same((p, pf, r), FR.track_fine(x, fs, F, hop))


def test_argument_errors_return_before_the_device_is_touched():
    from vocoderproject_amd import StftRoundTrip, StreamingPitchTracker
    F, hop = 1024, 256
    T = F + 441
    st = StftRoundTrip(2, T, F, hop)
    d_in = _dev(np.zeros((2, T)), np.float32)
    d_p, d_f, d_r = _tables((2, st.n_frames))
    L = st.L
    assert L.vp_stft_track_pitch_fine(None, d_in.data_ptr(), 44100.0, None, d_p.data_ptr(), d_f.data_ptr(), d_r.data_ptr(), _cur()) == VP_ERR_INVALID_ARG
    assert L.vp_stft_track_pitch_fine(st.h, d_in.data_ptr(), 44100.0, None, None, None, None, _cur()) == VP_ERR_INVALID_ARG
    assert L.vp_stft_track_pitch_fine(st.h, None, 44100.0, None, d_p.data_ptr(), d_f.data_ptr(), d_r.data_ptr(), _cur()) == VP_ERR_INVALID_ARG
    assert L.vp_stft_track_pitch_fine(st.h, d_in.data_ptr(), 7999.0, None, d_p.data_ptr(), d_f.data_ptr(), d_r.data_ptr(), _cur()) == VP_ERR_INVALID_ARG
    assert L.vp_stft_set_track_mode(None, FINE) == VP_ERR_INVALID_ARG and L.vp_stft_set_track_mode(st.h, 2) == VP_ERR_INVALID_ARG
    assert L.vp_stft_get_track_mode(None) == VP_ERR_INVALID_ARG
    trk = StreamingPitchTracker(2, 256, 44100.0)
    d_blk = _dev(np.zeros((1, 2, 256)), np.float32)
    s_p, s_f, s_r = _tables((1, 2))
    fine = L.vp_pv_tracker_process_blocks_fine_device
    assert fine(None, d_blk.data_ptr(), None, s_p.data_ptr(), s_f.data_ptr(), s_r.data_ptr(), 1, _cur()) == VP_ERR_INVALID_ARG
    assert fine(trk.h, None, None, s_p.data_ptr(), s_f.data_ptr(), s_r.data_ptr(), 1, _cur()) == VP_ERR_INVALID_ARG
    assert fine(trk.h, d_blk.data_ptr(), None, None, s_f.data_ptr(), None, 1, _cur()) == VP_ERR_INVALID_ARG
    assert fine(trk.h, d_blk.data_ptr(), None, s_p.data_ptr(), s_f.data_ptr(), s_r.data_ptr(), 0, _cur()) == VP_ERR_INVALID_ARG
    assert L.vp_pv_tracker_set_mode(None, FINE) == VP_ERR_INVALID_ARG and L.vp_pv_tracker_set_mode(trk.h, 2) == VP_ERR_INVALID_ARG
    assert L.vp_pv_tracker_get_mode(None) == VP_ERR_INVALID_ARG and L.vp_pv_tracker_get_mode(trk.h) == INTEGER
    torch.cuda.synchronize()
    for t in (d_p, s_p):
        assert bool((t == PERIOD_SENTINEL).all())
    for t in (d_f, d_r, s_f, s_r):
        assert bool(torch.isnan(t).all())                                           # nothing ran
    trk.close()
    st.close()


def test_forty_single_block_calls_allocate_nothing():
    c = FC.STREAM_CASES[1]
    d_in, d_key = _dev(FC.stream_input(c), np.float32), _dev(c.keys, np.int32)
    trk = _tracker(c)
    n0 = trk.debug_alloc_count()
    d_p, d_f, d_r = _tables((1, trk.S))
    for i in range(40):
        blk = d_in[i % c.n_blocks:i % c.n_blocks + 1]
        if i % 2:
            assert trk.L.vp_pv_tracker_process_blocks_fine_device(trk.h, blk.data_ptr(), d_key.data_ptr(), d_p.data_ptr(), d_f.data_ptr(), d_r.data_ptr(), 1, _cur()) == 0
        else:
            trk.set_fine(i % 4 == 0)
            assert trk.L.vp_pv_tracker_process_blocks_device(trk.h, blk.data_ptr(), d_key.data_ptr(), d_p.data_ptr(), d_r.data_ptr(), 1, _cur()) == 0
    torch.cuda.synchronize()
    assert trk.debug_alloc_count() == n0 and n0 > 0
    trk.close()


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------------
def _peak_hz(y, fs):
    """The spectral maximum of y, refined by a parabola through the log magnitudes of a zero-padded, Hann-windowed transform."""
    n = 1 << 18
    m = np.abs(np.fft.rfft(y * np.hanning(len(y)), n))
    k = int(np.argmax(m))
    a, b, c = np.log(m[k - 1:k + 2])
    return (k + 0.5 * (a - c) / (a - 2 * b + c)) * fs / n


def test_the_corrected_voice_lies_nearer_its_note_in_the_fine_mode():
    """A 0.5-amplitude 12-harmonic voice at 587.0 Hz, chromatic key: the note is D5, 587.33 Hz.  The integer tracker hears period 75
    (588.0 Hz), so its table asks for 586.331 Hz, 2.9 cents below the note; the fine one hears 75.13 samples and asks for 587.253 Hz,
    0.23 cents below.  Measured on the device through autotune(locked=True): 586.331 Hz and 587.251 Hz.  Asserted loosely, against the
    definition's own figures and no fixed number: the fine output lies nearer the note than the integer one, and within half the
    integer table's error plus the fine table's own."""
    from vocoderproject_amd import StftRoundTrip
    fs, F, hop, f0, note = 44100.0, 1024, 256, 587.0, 587.3295358348151
    T = F + 63 * hop + R.tau_max(fs)
    t = np.arange(T) / fs
    y = sum(np.sin(2 * np.pi * h * f0 * t + 0.37 * h) / h for h in range(1, 13))
    x = (0.5 * y / np.abs(y).max()).astype(np.float32)[None, :]
    p, pf, r = FR.track_fine(x[:, :F + R.tau_max(fs)], fs, F, F, 12)
    assert O_closest(fs / pf[0, 0]) == pytest.approx(note, abs=1e-6)
    want_fine, want_int = f0 * r[0, 0], f0 * R.track(x[:, :F + R.tau_max(fs)], fs, F, F, 12)[1][0, 0]
    st = StftRoundTrip(1, T, F, hop)
    d_in = _dev(x, np.float32)
    peaks = {}
    for mode in (False, True):
        st.set_track_mode(mode)
        out = torch.full_like(d_in, float("nan"))
        st.autotune(d_in, out, fs, keys=12, locked=True)
        torch.cuda.synchronize()
        peaks[mode] = _peak_hz(out.cpu().numpy()[0, 4 * F:T - 4 * F].astype(np.float64), fs)
    st.close()
    print(f"PV TRACK FINE end to end: note {note:.3f} Hz, integer mode {peaks[False]:.3f} Hz (its table asks for {want_int:.3f}), "
          f"fine mode {peaks[True]:.3f} Hz (its table asks for {want_fine:.3f})")
    assert abs(peaks[True] - note) < abs(peaks[False] - note)
    assert abs(peaks[True] - note) <= 0.5 * abs(want_int - note) + abs(want_fine - note)


def O_closest(pitch):
    from oracle import oracle_py as O
    return O.notes_closest(pitch, 12)
