"""The locked time stretch with a phase reset on the GPU (include/vp_amd.h vp_stft_time_stretch_locked_reset; kernel
vp_k_stft_pv_stretch_lock_reset of csrc/vp_stft_stretch_reset.inc): an all-zero table is vp_stft_time_stretch_locked bit for bit, on that
call's own test tables -- the test of the copy --; against the NumPy definition tests/pv_transient_reference.py on the items of
tests/pv_transient_cases.py (whose gate and conditioning tests/test_pv_transient_reference_cpu.py asserts), with flags on frame 0, the last
frame, every frame, a silent frame and the frame behind a silent one, within pv_stretch_lock_cases.bound unchanged; behind a reset at
ratio 1 and frames hop apart the output is vp_stft_roundtrip's, and with the flag cleared it is not; rows are independent and any non-zero
byte is a set flag; argument errors; no allocation; transients= equals the explicit four steps.  The outputs start as NaN, so every sample
must have been written.  The TRANSIENT lines (-s) are the measured errors."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_lock_cases as LC  # noqa: E402
import pv_stretch_cases as SC  # noqa: E402
import pv_transient_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu

F = TC.F
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _nan_out(st):
    return torch.full((st.S, st.T), float("nan"), dtype=torch.float32, device="cuda")


def _reset(st, x, pos, ratio, reset):
    """One vp_stft_time_stretch_locked_reset call on x [S][n_in] with the tables pos, ratio and reset [S][nF]."""
    d_in, d_out = _dev(x, np.float32), _nan_out(st)
    st.time_stretch_locked(d_in, d_out, d_pos=_dev(np.clip(pos, SC.INT_MIN, SC.INT_MAX), np.int32), d_ratio=_dev(ratio, np.float64), d_reset=_dev(reset, np.uint8))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _launch(items):
    from vocoderproject_amd import StftRoundTrip
    it = items[0]
    assert all(len(i.x) == len(it.x) and i.T == it.T and i.hop == it.hop for i in items)
    st = StftRoundTrip(len(items), it.T, F, it.hop)
    assert st.n_frames == len(it.pos)
    y = _reset(st, np.stack([i.x for i in items]), np.stack([i.pos for i in items]), np.stack([i.ratio for i in items]), np.stack([i.reset for i in items]))
    st.close()
    return y


def _check(y, items, tag):
    assert y.shape == (len(items), items[0].T) and np.all(np.isfinite(y)), tag
    for s, it in enumerate(items):
        ref = TC.reference(it)
        if not TC.pointwise(it):                                                         # (misses the conditioning probe: properties only)
            print(f"TRANSIENT {tag} {it.name}: properties only, max |y| {np.abs(y[s]).max():.3g}")
            assert np.abs(y[s]).max() <= TC.ceiling(it) + 1e-6, it.name
            continue
        err, bnd = np.abs(y[s] - ref).max(), TC.bound(it.hop, ref)
        print(f"TRANSIENT {tag} {it.name}: err {err:.3g} bound {bnd:.3g}, {int(np.count_nonzero(it.reset))} flags")
        assert err <= bnd, (it.name, err, bnd)
    covered = (len(items[0].pos) - 1) * items[0].hop + F
    assert np.all(y[:, covered:] == 0)                                                   # samples no frame covers


# ---- 1. an all-zero table is vp_stft_time_stretch_locked, bit for bit: the test of the copy ------------------------------------------------------
@pytest.mark.parametrize("hop", TC.HOPS)
def test_an_all_zero_table_is_bit_identical_to_time_stretch_locked(hop):
    """On the tables of test_gpu_pv_stretch_lock.py's own test of the copy: pv_lock_cases curves, nF 19, 6 and 1, positions f hop."""
    from vocoderproject_amd import StftRoundTrip
    S = len(LC.GPU_STREAMS)
    for nF in (19, 6, 1):
        x = LC.gpu_input(hop, nF)
        T = x.shape[1]
        st = StftRoundTrip(S, T, F, hop)
        d_in = _dev(x, np.float32)
        d_pos = _dev(np.tile(np.arange(nF) * hop, (S, 1)), np.int32)
        d_zero = torch.zeros((S, nF), dtype=torch.uint8, device="cuda")
        for name in LC.GPU_CURVES:
            d_ratio = _dev(LC.gpu_ratios(name, hop, nF), np.float64)
            o1, o2 = _nan_out(st), _nan_out(st)
            st.time_stretch_locked(d_in, o1, d_pos=d_pos, d_ratio=d_ratio, d_reset=d_zero)
            st.time_stretch_locked(d_in, o2, d_pos=d_pos, d_ratio=d_ratio)
            torch.cuda.synchronize()
            y, o = o1.cpu().numpy(), o2.cpu().numpy()
            assert np.all(np.isfinite(y)) and np.abs(y).max() > 0
            for s in range(S):
                assert np.array_equal(y[s], o[s]), (nF, name, s, np.abs(y[s] - o[s]).max())
        st.close()


@pytest.mark.parametrize("c", [c for c in TC.GPU_CASES if c.nF == 19], ids=TC.gpu_id)
def test_an_all_zero_table_is_bit_identical_on_stretched_tables(c):
    """... and off the grid: the locked stretch's own items (four factors and a seeded table, an odd n_in)."""
    from vocoderproject_amd import StftRoundTrip
    import pv_stretch_lock_cases as K
    items = K.gpu_items(c)
    x, pos, r = np.stack([i.x for i in items]), np.stack([i.pos for i in items]), np.stack([i.ratio for i in items])
    st = StftRoundTrip(len(items), items[0].T, F, c.hop)
    y = _reset(st, x, pos, r, np.zeros(pos.shape, np.uint8))
    o = _nan_out(st)
    st.time_stretch_locked(_dev(x, np.float32), o, d_pos=_dev(pos, np.int32), d_ratio=_dev(r, np.float64))
    torch.cuda.synchronize()
    st.close()
    assert np.all(np.isfinite(y)) and np.array_equal(y, o.cpu().numpy())


# ---- 2. against NumPy ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TC.GPU_CASES, ids=TC.gpu_id)
def test_reset_stretch_matches_numpy(c):
    """Streams: a flag on frame 0, on the last frame, on every frame, on scattered frames, garbage bytes."""
    items = TC.gpu_items(c)
    assert items[0].reset[0] and items[1].reset[-1] and items[2].reset.all() and items[4].reset.max() > 1
    _check(_launch(items), items, "case")


def test_flags_on_a_silent_frame_and_behind_one_match_numpy():
    items = TC.silent_items()
    assert all(TC.pointwise(it) for it in items)
    y = _launch(items)
    _check(y, items, "silent")
    assert np.abs(y[:, 2048 + F:4608 - F]).max() == 0                                    # (frames without a peak give zeros)


# ---- 3. behind a reset the stage is the identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", TC.HOPS)
def test_behind_a_reset_the_output_is_the_plain_round_trips(hop):
    """Ratio +7 semitones and positions off the grid up to frame r, a flag on frame r, then ratio 1 and frames hop apart: every output
    sample covered only by frames >= r has vp_stft_roundtrip's double-precision bits for the input those frames read -- the input moved
    so that frame f stands at f hop.  The same call with the flag cleared does not."""
    from vocoderproject_amd import StftRoundTrip
    S, nF, r = 4, TC.IDENTITY_NF, TC.IDENTITY_R
    pos, ratio, reset, n_in = TC.identity_tables(hop, S)
    x = np.stack([LC.SIGNALS[s](n_in, seed=hop + 9) for s in ("voice", "noise", "tone-tone", "voice+noise")])
    T = LC.length(nF, hop, hop - 1)
    st = StftRoundTrip(S, T, F, hop)
    y = _reset(st, x, pos, ratio, reset)
    y0 = _reset(st, x, pos, ratio, np.zeros_like(reset))
    # the plain round trip of the input as the frames >= r read it: x'[t] = x[t - r hop + pos[r]]
    xr = np.zeros((S, T), np.float32)
    for s in range(S):
        shift = int(pos[s, r]) - r * hop
        lo = max(0, -shift)
        hi = min(T, n_in - shift)
        xr[s, lo:hi] = x[s, lo + shift:hi + shift]
    d_out = _nan_out(st)
    st(_dev(xr, np.float32), d_out)
    torch.cuda.synchronize()
    yr = d_out.cpu().numpy()
    st.close()
    first, last = (r - 1) * hop + F, (nF - 1) * hop + F                                  # covered by frames r .. nF - 1 only
    assert last - first >= 4 * hop and np.abs(yr[:, first:last]).max() > 1e-3
    for s in range(S):
        assert np.array_equal(y[s, first:last], yr[s, first:last]), (s, np.abs(y[s, first:last] - yr[s, first:last]).max())
        assert not np.array_equal(y0[s, first:last], yr[s, first:last]), s
        print(f"TRANSIENT identity hop {hop} stream {s}: {last - first} samples equal the round trip's; without the flag max difference "
              f"{np.abs(y0[s, first:last] - yr[s, first:last]).max():.3g}")


# ---- 4. rows, flag bytes ------------------------------------------------------------------------------------------------------------------------------
def test_rows_are_independent_and_any_non_zero_byte_is_a_flag():
    from vocoderproject_amd import StftRoundTrip
    c = next(g for g in TC.GPU_CASES if g.hop == 256 and g.nF == 19)
    items = TC.gpu_items(c)
    x, pos, r = np.stack([i.x for i in items]), np.stack([i.pos for i in items]), np.stack([i.ratio for i in items])
    reset = np.stack([i.reset for i in items])
    ones = (reset != 0).astype(np.uint8)
    garbage = np.where(reset != 0, np.random.default_rng(76).integers(1, 256, reset.shape), 0).astype(np.uint8)
    assert garbage.max() > 1 and not np.array_equal(garbage, ones)
    st = StftRoundTrip(TC.N_STREAMS, items[0].T, F, c.hop)
    y, y1, yg = _reset(st, x, pos, r, reset), _reset(st, x, pos, r, ones), _reset(st, x, pos, r, garbage)
    assert np.array_equal(y, y1) and np.array_equal(y, yg)
    other = reset.copy()
    other[2] = 0
    other[2, 5] = 1
    yo = _reset(st, x, pos, r, other)
    xs = x.copy()
    xs[2] = np.nan
    yn = _reset(st, xs, pos, r, reset)
    st.close()
    assert not np.array_equal(yo[2], y[2])
    for s in (0, 1, 3, 4):
        assert np.array_equal(yo[s], y[s]) and np.array_equal(yn[s], y[s]), s
    for s, it in enumerate(items):                                                       # ... and a row alone has the row's bits
        st1 = StftRoundTrip(1, it.T, F, it.hop)
        assert np.array_equal(_reset(st1, it.x[None], it.pos[None], it.ratio[None], it.reset[None])[0], y[s]), s
        st1.close()


# ---- 5. errors, allocation, the convenience ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing_and_calls_allocate_nothing():
    from vocoderproject_amd import StftRoundTrip, VpError
    c = next(g for g in TC.GPU_CASES if g.hop == 256 and g.nF == 6)
    items = TC.gpu_items(c)
    x, pos, r = np.stack([i.x for i in items]), np.stack([i.pos for i in items]), np.stack([i.ratio for i in items])
    reset = np.stack([i.reset for i in items])
    st = StftRoundTrip(TC.N_STREAMS, items[0].T, F, c.hop)
    want = _reset(st, x, pos, r, reset)
    d_in, d_pos, d_ratio, d_reset, d_out = _dev(x, np.float32), _dev(pos, np.int32), _dev(r, np.float64), _dev(reset, np.uint8), _nan_out(st)
    stream = torch.cuda.current_stream().cuda_stream
    call = st.L.vp_stft_time_stretch_locked_reset
    good = dict(p=st.h, d_in=d_in.data_ptr(), n_in=x.shape[1], d_pos=d_pos.data_ptr(), d_out=d_out.data_ptr(), d_ratio=d_ratio.data_ptr(), d_reset=d_reset.data_ptr())
    order = ("p", "d_in", "n_in", "d_pos", "d_out", "d_ratio", "d_reset")
    for change in (dict(n_in=F - 1), dict(n_in=0), dict(d_in=None), dict(d_pos=None), dict(d_out=None), dict(d_ratio=None), dict(d_reset=None)):
        a = dict(good, **change)
        assert call(*[a[k] for k in order], stream) == VP_ERR_INVALID_ARG, change
        assert b"stretch locked reset" in st.L.vp_stft_last_error(st.h)
    assert call(*[dict(good, p=None)[k] for k in order], stream) == VP_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_out).all())                                                # nothing was launched
    n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    for _ in range(20):
        assert call(*[good[k] for k in order], stream) == 0
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0                   # no allocation in the call
    st.close()
    assert np.array_equal(d_out.cpu().numpy(), want)
    T2 = 2048 + 5 * 512
    st2 = StftRoundTrip(2, T2, 2048, 512)
    i2, o2 = torch.zeros((2, T2), dtype=torch.float32, device="cuda"), torch.full((2, T2), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(VpError) as e:
        st2.time_stretch_locked(i2, o2, stretch=1.0, d_reset=torch.zeros((2, st2.n_frames), dtype=torch.uint8, device="cuda"))
    assert e.value.code == VP_ERR_GEOMETRY and "2048-point frames are not built" in str(e.value)
    torch.cuda.synchronize()
    st2.close()
    assert bool((o2 == 7.0).all())


@pytest.mark.parametrize("hop", [128, 512])
def test_transients_equals_the_four_explicit_steps(hop):
    """time_stretch_locked(stretch=, transients=thr, span=K) is onset_flux -> copy -> pick_onsets and stretch_positions_transient per
    stream -> upload -> the reset call, bit for bit; each stream is planned with its own stretch against the input's length."""
    from vocoderproject_amd import StftRoundTrip, pick_onsets, stretch_positions_transient
    c = next(p for p in TC.PICK_CASES if p.hop == hop)
    x = TC.pick_input(c)
    S, n_in = x.shape
    factors = np.array([0.5, 0.75, 1.5, 2.0])
    T = int(n_in * 1.25)
    st = StftRoundTrip(S, T, F, hop)
    d_in = _dev(x, np.float32)
    semis = np.array([0.0, 0.0, 7.0, -3.0])[:, None] * np.ones((S, st.n_frames))
    o1 = _nan_out(st)
    st.time_stretch_locked(d_in, o1, stretch=factors, semitones=semis, transients=TC.THR, span=2)
    torch.cuda.synchronize()
    d_flux, d_mass = st.onset_flux(d_in)
    flux, mass = d_flux.cpu().numpy(), d_mass.cpu().numpy()
    pos, reset = np.zeros((S, st.n_frames), np.int32), np.zeros((S, st.n_frames), np.uint8)
    for s in range(S):
        pos[s], reset[s] = stretch_positions_transient(pick_onsets(flux[s], mass[s], TC.THR), st.n_frames, hop, factors[s], n_in, F, 2)
    assert reset.any(axis=1).all()                                                       # every stream has a span
    o2 = _nan_out(st)
    st.time_stretch_locked(d_in, o2, d_pos=_dev(pos, np.int32), semitones=semis, d_reset=_dev(reset, np.uint8))
    o3 = _nan_out(st)
    st.time_stretch_locked(d_in, o3, stretch=factors, semitones=semis, transients=True, span=2)   # (True: the default threshold)
    torch.cuda.synchronize()
    st.close()
    y1, y2 = o1.cpu().numpy(), o2.cpu().numpy()
    assert np.all(np.isfinite(y1)) and np.abs(y1).max() > 0 and np.array_equal(y1, y2) and np.array_equal(y1, o3.cpu().numpy())
