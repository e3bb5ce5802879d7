"""The pitch tracker and the automatic correction on the GPU (include/vp_amd.h vp_stft_track_pitch, vp_stft_autotune; kernel
vp_k_yin_track of csrc/vp_track.hip): period and ratio bit-equal to tests/pv_track_reference.py on every frame of every case of
tests/pv_track_cases.py (whose conditioning tests/test_pv_track_reference_cpu.py gates), the nullable outputs and keys, autotune against
its two parts, the closed loop tracker -> shift -> tracker, batch independence, argument errors, and the neighbours on the same handle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_track_cases as TC  # noqa: E402
import pv_track_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

PERIOD_SENTINEL = -777
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _raw_track(st, d_in, fs, d_key=None, period=True, ratio=True):
    """vp_stft_track_pitch through the C ABI with sentinel-filled outputs: -> (rc, period or None, ratio or None) as NumPy arrays."""
    d_p = torch.full((st.S, st.n_frames), PERIOD_SENTINEL, dtype=torch.int32, device="cuda") if period else None
    d_r = torch.full((st.S, st.n_frames), float("nan"), dtype=torch.float64, device="cuda") if ratio else None
    rc = st.L.vp_stft_track_pitch(st.h, d_in.data_ptr(), float(fs), d_key.data_ptr() if d_key is not None else None,
                                  d_p.data_ptr() if period else None, d_r.data_ptr() if ratio else None,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, (d_p.cpu().numpy() if period else None), (d_r.cpu().numpy() if ratio else None)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. bit equality with the definition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TC.CASES, ids=TC.case_id)
def test_period_and_ratio_equal_the_reference_bit_for_bit(c):
    from vocoderproject_amd import StftRoundTrip
    x = TC.case_input(c)
    ref_p, ref_r = TC.reference(c)
    st = StftRoundTrip(TC.N_STREAMS, TC.length(c), c.F, c.hop)
    rc, p, r = _raw_track(st, _dev(x, np.float32), c.fs, d_key=_dev(c.keys, np.int32))
    st.close()
    assert rc == 0
    assert p.shape == ref_p.shape and not np.any(p == PERIOD_SENTINEL) and not np.any(np.isnan(r))     # every slot was written
    bad = np.argwhere(p != ref_p)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), p[tuple(bad[0])], ref_p[tuple(bad[0])])
    bad = np.argwhere(_bits(r) != _bits(ref_r))
    assert bad.size == 0, (len(bad), bad[:4].tolist(), r[tuple(bad[0])], ref_r[tuple(bad[0])])


def test_python_entry_takes_keys_in_three_forms():
    from vocoderproject_amd import StftRoundTrip
    c = next(c for c in TC.CASES if c.keys == (0, 7, 12) and c.length == "clamp")
    ref_p, ref_r = TC.reference(c)
    st = StftRoundTrip(TC.N_STREAMS, TC.length(c), c.F, c.hop)
    d_in = _dev(TC.case_input(c), np.float32)
    for keys in (list(c.keys), _dev(c.keys, np.int32)):
        p, r = st.track_pitch(d_in, c.fs, keys=keys)
        torch.cuda.synchronize()
        assert np.array_equal(p.cpu().numpy(), ref_p) and np.array_equal(_bits(r.cpu().numpy()), _bits(ref_r))
    table = st._key_table
    p7, r7 = st.track_pitch(d_in, c.fs, keys=7)
    assert st._key_table is table                                                   # one key table per handle
    torch.cuda.synchronize()
    want_p, want_r = R.track(TC.case_input(c), c.fs, c.F, c.hop, 7)
    st.close()
    assert np.array_equal(p7.cpu().numpy(), want_p) and np.array_equal(_bits(r7.cpu().numpy()), _bits(want_r))


# ---- 2. nullable outputs and keys -----------------------------------------------------------------------------------------------------------
def test_nullable_outputs_and_keys():
    from vocoderproject_amd import StftRoundTrip
    c = next(c for c in TC.CASES if c.keys == (-1, 13, 12) and c.length == "long" and c.hop == 256)
    st = StftRoundTrip(TC.N_STREAMS, TC.length(c), c.F, c.hop)
    d_in = _dev(TC.case_input(c), np.float32)
    rc, p, r = _raw_track(st, d_in, c.fs, d_key=_dev(c.keys, np.int32))
    assert rc == 0 and np.array_equal(p, TC.reference(c)[0])
    rc1, p1, _ = _raw_track(st, d_in, c.fs, d_key=_dev(c.keys, np.int32), ratio=False)
    rc2, _, r2 = _raw_track(st, d_in, c.fs, d_key=_dev(c.keys, np.int32), period=False)
    assert rc1 == 0 and rc2 == 0 and np.array_equal(p1, p) and np.array_equal(_bits(r2), _bits(r))
    for keys in (None, (12, 12, 12)):                                               # NULL = chromatic = what -1 and 13 count as
        rc3, p3, r3 = _raw_track(st, d_in, c.fs, d_key=None if keys is None else _dev(keys, np.int32))
        assert rc3 == 0 and np.array_equal(p3, p) and np.array_equal(_bits(r3), _bits(r))
    rc4, _, r4 = _raw_track(st, d_in, c.fs, d_key=_dev((0, 0, 0), np.int32))
    st.close()
    assert rc4 == 0 and not np.array_equal(_bits(r4), _bits(r))                     # (the key is read)


# ---- 3. autotune against its parts ------------------------------------------------------------------------------------------------------------
def _tune_input(F, hop, fs, n_frames=19):
    T = F + (n_frames - 1) * hop + R.tau_max(fs) + 3
    return TC.make_input(("sine_off", "glide", "gap", "saw", "noise"), T, fs, F + hop), (12, 0, 7, 12, 3)


@pytest.mark.parametrize("F,hop", [(1024, 256), (2048, 512)])
def test_autotune_is_the_tracker_then_the_curve_call(F, hop):
    from vocoderproject_amd import StftRoundTrip
    fs = 44100.0
    x, keys = _tune_input(F, hop, fs)
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    d_in, d_key = _dev(x, np.float32), _dev(keys, np.int32)
    rc, p, r = _raw_track(st, d_in, fs, d_key=d_key)
    assert rc == 0 and np.any(p > 0) and np.any(p == 0) and len(np.unique(r)) > 4
    d_parts = torch.full_like(d_in, float("nan"))
    st.pitch_shift_curve(d_in, d_parts, d_ratio=_dev(r, np.float64))
    d_out = torch.full_like(d_in, float("nan"))
    d_p = torch.full((st.S, st.n_frames), PERIOD_SENTINEL, dtype=torch.int32, device="cuda")
    d_r = torch.full((st.S, st.n_frames), float("nan"), dtype=torch.float64, device="cuda")
    rc = st.L.vp_stft_autotune(st.h, d_in.data_ptr(), d_out.data_ptr(), fs, d_key.data_ptr(), d_p.data_ptr(), d_r.data_ptr(),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    y, y_parts = d_out.cpu().numpy(), d_parts.cpu().numpy()
    assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.1
    assert np.array_equal(y.view(np.uint32), y_parts.view(np.uint32))
    assert np.array_equal(d_p.cpu().numpy(), p) and np.array_equal(_bits(d_r.cpu().numpy()), _bits(r))
    # the Python entry, and the C call without a period table
    d_out2 = torch.full_like(d_in, float("nan"))
    p2, r2 = st.autotune(d_in, d_out2, fs, keys=list(keys))
    d_out3 = torch.full_like(d_in, float("nan"))
    rc = st.L.vp_stft_autotune(st.h, d_in.data_ptr(), d_out3.data_ptr(), fs, d_key.data_ptr(), None, d_r.data_ptr(),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    st.close()
    assert rc == 0 and np.array_equal(p2.cpu().numpy(), p) and np.array_equal(_bits(r2.cpu().numpy()), _bits(r))
    assert np.array_equal(d_out2.cpu().numpy().view(np.uint32), y.view(np.uint32))
    assert np.array_equal(d_out3.cpu().numpy().view(np.uint32), y.view(np.uint32))


def test_autotune_of_an_unvoiced_batch_is_the_zero_shift():
    from vocoderproject_amd import StftRoundTrip
    F, hop, fs = 1024, 256, 44100.0
    T = F + 18 * hop + R.tau_max(fs)
    x = TC.make_input(("noise", "silence", "noise", "noise"), T, fs, 5)
    x[2] = x[2, ::-1] * np.float32(0.01)
    x[3] *= np.float32(0.1)
    st = StftRoundTrip(4, T, F, hop)
    d_in = _dev(x, np.float32)
    d_out, d_zero = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    p, r = st.autotune(d_in, d_out, fs)
    st.pitch_shift(d_in, d_zero, 0.0)
    torch.cuda.synchronize()
    st.close()
    assert np.all(p.cpu().numpy() == 0) and np.all(r.cpu().numpy() == 1.0)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), d_zero.cpu().numpy().view(np.uint32))


# ---- 4. closed loop on the device ---------------------------------------------------------------------------------------------------------------
def test_closed_loop_tracker_shift_tracker():
    """The condition tests/test_pv_track_reference_cpu.py establishes for the reference: the corrected signal's period lies within one
    sample of fs / closestFreq on every frame of its fully overlapped part."""
    from vocoderproject_amd import StftRoundTrip
    x, keys = TC.steady_input()
    fs, F, hop = TC.STEADY_FS, TC.STEADY_F, TC.STEADY_HOP
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    p, r = st.autotune(d_in, d_out, fs, keys=keys)
    torch.cuda.synchronize()
    st.close()
    y = d_out.cpu().numpy()
    yc = np.stack([TC.covered_part(y[s], F, hop) for s in range(len(keys))])
    st2 = StftRoundTrip(yc.shape[0], yc.shape[1], F, hop)
    p2, _ = st2.track_pitch(_dev(yc, np.float32), fs, keys=keys)
    torch.cuda.synchronize()
    st2.close()
    p2 = p2.cpu().numpy()
    for s, target in enumerate(TC.steady_targets()):
        print(f"PV TRACK closed loop (device) {TC.STEADY[s]}: period {p.cpu().numpy()[s, 0]} -> {sorted(set(p2[s].tolist()))} target {target:.2f}")
        assert p2.shape[1] >= 8 and np.all(np.abs(p2[s] - target) <= 1.0), (s, p2[s], target)


# ---- 5. batch independence ----------------------------------------------------------------------------------------------------------------------
def test_streams_do_not_see_their_neighbours():
    from vocoderproject_amd import StftRoundTrip
    fs, F, hop = 44100.0, 1024, 256
    T = F + 9 * hop + R.tau_max(fs) + 7
    voiced = TC.make_input(("sine_off", "glide", "saw"), T, fs, 11)
    noise = TC.make_input(("noise",), T, fs, 12)[0]
    assert np.all(np.isfinite(noise))
    silent = np.zeros(T, np.float32)
    keys = (0, 7, 12)

    def run(rows, ks):
        st = StftRoundTrip(len(rows), T, F, hop)
        rc, p, r = _raw_track(st, _dev(np.stack(rows), np.float32), fs, d_key=_dev(ks, np.int32))
        st.close()
        assert rc == 0
        return p, r

    p_a, r_a = run([voiced[0], noise, voiced[1], silent, voiced[2]], (keys[0], 12, keys[1], 12, keys[2]))
    p_b, r_b = run([voiced[0], silent, voiced[1], noise, voiced[2]], (keys[0], 12, keys[1], 12, keys[2]))
    p_c, r_c = run([voiced[0], voiced[1], voiced[2]], keys)
    assert np.any(p_c > 0)
    for i, j in enumerate((0, 2, 4)):
        assert np.array_equal(p_a[j], p_c[i]) and np.array_equal(p_b[j], p_c[i])
        assert np.array_equal(_bits(r_a[j]), _bits(r_c[i])) and np.array_equal(_bits(r_b[j]), _bits(r_c[i]))
    assert np.all(p_a[3] == 0) and np.all(p_b[1] == 0) and np.array_equal(p_a[1], p_b[3])


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_statuses_with_a_message_and_launch_nothing():
    from vocoderproject_amd import StftRoundTrip, VpError
    F, hop = 1024, 256
    st = StftRoundTrip(2, F + 441, F, hop)
    d_in = _dev(np.zeros((2, F + 441)), np.float32)
    msg = lambda: st.L.vp_stft_last_error(st.h).decode()                             # noqa: E731
    for fs in (7999.0, 51201.0, float("nan")):
        rc, p, r = _raw_track(st, d_in, fs)
        assert rc == VP_ERR_INVALID_ARG and "sample rate" in msg()
        assert np.all(p == PERIOD_SENTINEL) and np.all(np.isnan(r))                 # nothing ran
    rc, p, r = _raw_track(st, d_in, 44100.0, period=False, ratio=False)
    assert rc == VP_ERR_INVALID_ARG and "both null" in msg()
    rc, p, r = _raw_track(st, d_in, 44101.0)                                        # tauMax 442: the rows are one sample short
    assert rc == VP_ERR_GEOMETRY and "shorter" in msg() and np.all(p == PERIOD_SENTINEL) and np.all(np.isnan(r))
    d_out = torch.full_like(d_in, float("nan"))
    with pytest.raises(VpError) as e:
        st.autotune(d_in, d_out, 44101.0)
    assert e.value.code == VP_ERR_GEOMETRY and "shorter" in str(e.value)
    torch.cuda.synchronize()
    assert np.all(np.isnan(d_out.cpu().numpy()))
    rc = st.L.vp_stft_autotune(st.h, d_in.data_ptr(), d_out.data_ptr(), 44100.0, None, None, None, None)   # the ratio table is required
    assert rc == VP_ERR_INVALID_ARG and "ratio" in msg()
    rc, p, r = _raw_track(st, d_in, 44100.0)                                        # and the handle still serves a good call
    st.close()
    assert rc == 0 and np.all(p == 0) and np.all(r == 1.0)


# ---- 7. neighbours on the same handle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,hop", [(1024, 256), (2048, 512)])
def test_neighbours_on_the_handle_keep_their_bits(F, hop):
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios, stretch_positions
    fs = 44100.0
    x, keys = _tune_input(F, hop, fs, n_frames=9)
    S, T = x.shape
    st = StftRoundTrip(S, T, F, hop)
    d_in = _dev(x, np.float32)
    ratio = _dev(np.repeat(semitones_to_ratios(np.linspace(-5.0, 5.0, S))[:, None], st.n_frames, axis=1), np.float64)
    pos = np.tile(stretch_positions(st.n_frames, hop, 1.25, T, F), (S, 1))

    def neighbours():
        outs = []
        for call in (lambda o: st.pitch_shift(d_in, o, 3.0), lambda o: st.pitch_shift_curve(d_in, o, d_ratio=ratio),
                     lambda o: st.time_stretch(d_in, o, positions=pos, semitones=-2.0), lambda o: st(d_in, o)):
            o = torch.full_like(d_in, float("nan"))
            call(o)
            outs.append(o)
        torch.cuda.synchronize()
        return [o.cpu().numpy().view(np.uint32) for o in outs]

    before = neighbours()
    p, r = st.track_pitch(d_in, fs, keys=list(keys))
    after = neighbours()
    p2, r2 = st.track_pitch(d_in, fs, keys=list(keys))
    torch.cuda.synchronize()
    st.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(p.cpu().numpy(), p2.cpu().numpy()) and np.array_equal(_bits(r.cpu().numpy()), _bits(r2.cpu().numpy()))
    want_p, want_r = R.track(x, fs, F, hop, keys)
    assert np.array_equal(p.cpu().numpy(), want_p) and np.array_equal(_bits(r.cpu().numpy()), _bits(want_r))
