"""The peak-locked time stretch on the GPU (include/vp_amd.h vp_stft_time_stretch_locked; kernel vp_k_stft_pv_stretch_lock of
csrc/vp_stft_stretch_lock.inc): against the NumPy definition tests/pv_stretch_lock_reference.py on the items of
tests/pv_stretch_lock_cases.py (whose gate and conditioning tests/test_pv_stretch_lock_reference_cpu.py asserts; the items it demotes are
held to finite and bounded here too), bit-identical to vp_stft_pitch_shift_locked on the table f hop -- the test of the copy --, the edge
tables and the smallest inputs, independence of the rows, homogeneity, silence, more workgroups than compute units, argument errors,
no allocation, stretch= against d_pos=, and what the stage is for: a stretched and shifted tone keeps an even envelope.  The outputs
start as NaN, so every sample must have been written.  The STRETCHLOCK lines (-s) are the measured errors."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_lock_cases as LC  # noqa: E402
import pv_stretch_cases as SC  # noqa: E402
import pv_stretch_lock_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

F = K.F
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _nan_out(st):
    return torch.full((st.S, st.T), float("nan"), dtype=torch.float32, device="cuda")


def _locked(st, x, pos, ratio):
    """One vp_stft_time_stretch_locked call on x [S][n_in] with the tables pos [S][nF] (any integers) and ratio [S][nF]."""
    d_in, d_out = _dev(x, np.float32), _nan_out(st)
    st.time_stretch_locked(d_in, d_out, d_pos=_dev(np.clip(pos, SC.INT_MIN, SC.INT_MAX), np.int32), d_ratio=_dev(ratio, np.float64))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _launch(items):
    """The items of one launch (one input length, one output length, one hop) -> y [S][T]."""
    from vocoderproject_amd import StftRoundTrip
    it = items[0]
    assert all(len(i.x) == len(it.x) and i.T == it.T and i.hop == it.hop for i in items)
    st = StftRoundTrip(len(items), it.T, F, it.hop)
    assert st.n_frames == len(it.pos)
    y = _locked(st, np.stack([i.x for i in items]), np.stack([i.pos for i in items]), np.stack([i.ratio for i in items]))
    st.close()
    return y


def _check(y, items, tag):
    assert y.shape == (len(items), items[0].T) and np.all(np.isfinite(y)), tag
    for s, it in enumerate(items):
        ref = K.reference(it)
        if not K.pointwise(it):                                                          # (misses the conditioning probe: properties only)
            print(f"STRETCHLOCK {tag} {it.name}: properties only, max |y| {np.abs(y[s]).max():.3g}")
            assert np.abs(y[s]).max() <= K.ceiling(it) + 1e-6, it.name
            continue
        err, bnd = np.abs(y[s] - ref).max(), K.bound(it.hop, ref)
        print(f"STRETCHLOCK {tag} {it.name}: err {err:.3g} bound {bnd:.3g}")
        assert err <= bnd, (it.name, err, bnd)
    covered = (len(items[0].pos) - 1) * items[0].hop + F
    assert np.all(y[:, covered:] == 0)                                                   # samples no frame covers


# ---- 1. against NumPy -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.GPU_CASES, ids=K.gpu_id)
def test_locked_time_stretch_matches_numpy(c):
    items = K.gpu_items(c)
    assert len(items[0].x) % 2 == 1 and items[0].T - ((c.nF - 1) * c.hop + F) == c.hop - 1
    assert all(K.pointwise(it) for it in items)
    _check(_launch(items), items, "case")


# ---- 2. the table f hop is vp_stft_pitch_shift_locked, bit for bit: the test of the copy ---------------------------------------------------------
@pytest.mark.parametrize("hop", K.HOPS)
def test_grid_table_is_bit_identical_to_pitch_shift_locked(hop):
    from vocoderproject_amd import StftRoundTrip
    S = len(LC.GPU_STREAMS)
    for nF in (19, 6, 1):
        x = LC.gpu_input(hop, nF)
        T = x.shape[1]
        st = StftRoundTrip(S, T, F, hop)
        d_in = _dev(x, np.float32)
        d_pos = _dev(np.tile(np.arange(nF) * hop, (S, 1)), np.int32)
        for name in LC.GPU_CURVES:
            d_ratio = _dev(LC.gpu_ratios(name, hop, nF), np.float64)
            o1, o2 = _nan_out(st), _nan_out(st)
            st.time_stretch_locked(d_in, o1, d_pos=d_pos, d_ratio=d_ratio)
            st.pitch_shift_locked(d_in, o2, d_ratio=d_ratio)
            torch.cuda.synchronize()
            y, o = o1.cpu().numpy(), o2.cpu().numpy()
            assert np.all(np.isfinite(y)) and np.abs(y).max() > 0
            for s in range(S):
                assert np.array_equal(y[s], o[s]), (nF, name, s, np.abs(y[s] - o[s]).max())
        st.close()


# ---- 3. the edge tables: both clamps of the advance and of the position, unaligned frames -------------------------------------------------------
@pytest.mark.parametrize("c", K.EDGE_CASES, ids=SC.case_id)
def test_edge_tables_match_numpy(c):
    items = K.edge_case_items(c)
    _check(_launch(items), items, "edge")


@pytest.mark.parametrize("cn", K.SMALL_CASES, ids=SC.small_id)
def test_the_smallest_inputs_match_numpy(cn):
    c, n_in = cn
    items = K.edge_case_items(c, n_in)
    assert len(items[0].x) == n_in and all(K.pointwise(it) for it in items)
    _check(_launch(items), items, "small")


# ---- 4. rows, homogeneity, silence ------------------------------------------------------------------------------------------------------------------
def test_a_garbage_row_is_clamped_and_touches_no_other_stream():
    from vocoderproject_amd import StftRoundTrip
    c = K.GpuCase(256, 19, "steps")
    items = K.gpu_items(c)
    x, pos, r = np.stack([i.x for i in items]), np.stack([i.pos for i in items]), np.stack([i.ratio for i in items])
    n_in = x.shape[1]
    garbage = np.random.default_rng([F, 14]).integers(-3 * n_in, 3 * n_in, c.nF)
    garbage[:6] = [-1, -2 ** 31, 2 ** 31 - 1, n_in, n_in - F + 1, 5]
    dirty, clipped = pos.copy(), pos.copy()
    dirty[2], clipped[2] = garbage, np.clip(garbage, 0, n_in - F)
    rd = r.copy()
    rd[2, ::3] = [np.nan, 0.0, 7.0, -1.0, np.inf, 0.25, 3.0][:len(rd[2, ::3])]
    rc = rd.copy()
    rc[2] = np.clip(np.nan_to_num(rd[2], nan=0.5, posinf=2.0), 0.5, 2.0)
    st = StftRoundTrip(K.N_STREAMS, items[0].T, F, c.hop)
    yd, yc, y0 = _locked(st, x, dirty, rd), _locked(st, x, clipped, rc), _locked(st, x, pos, r)
    xs = x.copy()
    xs[2] = 0.0
    ys = _locked(st, xs, pos, r)
    st.close()
    assert np.all(np.isfinite(yd)) and np.array_equal(yd[2], yc[2]) and not np.array_equal(yd[2], y0[2])
    for s in (0, 1, 3, 4):
        assert np.array_equal(yd[s], y0[s]) and np.array_equal(ys[s], y0[s]), s
    assert np.all(ys[2] == 0)                                                            # silence gives zeros


@pytest.mark.parametrize("hop", [64, 512])
def test_scaling_by_a_power_of_two_scales_the_bits_and_silence_gives_zeros(hop):
    from vocoderproject_amd import StftRoundTrip
    c = next(g for g in K.GPU_CASES if g.hop == hop and g.nF == 6)
    items = K.gpu_items(c)
    x, pos, r = np.stack([i.x for i in items]), np.stack([i.pos for i in items]), np.stack([i.ratio for i in items])
    st = StftRoundTrip(K.N_STREAMS, items[0].T, F, hop)
    y1, y4, yq = _locked(st, x, pos, r), _locked(st, 4.0 * x, pos, r), _locked(st, 0.125 * x, pos, r)
    z = _locked(st, np.zeros_like(x), pos, r)
    st.close()
    assert np.abs(y1).max() > 1e-3
    assert np.array_equal(y4, 4.0 * y1) and np.array_equal(yq, 0.125 * y1)
    assert np.all(z == 0)


# ---- 5. more workgroups than compute units --------------------------------------------------------------------------------------------------------
def test_three_hundred_streams_each_with_its_own_stretch_and_curve():
    from vocoderproject_amd import StftRoundTrip
    x, pos, r = SC.big_input(), SC.big_positions(), K.big_ratios()
    st = StftRoundTrip(K.BIG_S, K.BIG_T, F, K.BIG_HOP)
    assert st.n_frames == K.BIG_NF
    y = _locked(st, x, pos, r)
    st.close()
    assert np.all(np.isfinite(y)) and np.all(y[:, (K.BIG_NF - 1) * K.BIG_HOP + F:] == 0)
    for s, it in zip(K.BIG_CHECKED, K.big_items()):
        ref = K.reference(it)
        err, bnd = np.abs(y[s] - ref).max(), K.bound(it.hop, ref)
        print(f"STRETCHLOCK big stream {s}: err {err:.3g} bound {bnd:.3g}")
        assert K.pointwise(it) and err <= bnd, (s, err, bnd)
    assert np.abs(y).max(axis=1).min() > 0                                               # every stream was written by its own workgroup


# ---- 6. errors, allocation, the table-building paths ------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing():
    """Through the raw C entry, on a handle that has run and runs again: a short input and each pointer NULL in turn return
    VP_ERR_INVALID_ARG with a message, a 2048-point handle VP_ERR_GEOMETRY; nothing is launched, and a valid call then still gives its bits."""
    from vocoderproject_amd import StftRoundTrip, VpError
    c = K.GpuCase(256, 6, "+7")
    items = K.gpu_items(c)
    x, pos, r = np.stack([i.x for i in items]), np.stack([i.pos for i in items]), np.stack([i.ratio for i in items])
    st = StftRoundTrip(K.N_STREAMS, items[0].T, F, c.hop)
    want = _locked(st, x, pos, r)
    d_in, d_pos, d_ratio, d_out = _dev(x, np.float32), _dev(pos, np.int32), _dev(r, np.float64), _nan_out(st)
    stream = torch.cuda.current_stream().cuda_stream
    call = st.L.vp_stft_time_stretch_locked
    good = dict(p=st.h, d_in=d_in.data_ptr(), n_in=x.shape[1], d_pos=d_pos.data_ptr(), d_out=d_out.data_ptr(), d_ratio=d_ratio.data_ptr())
    for change in (dict(n_in=F - 1), dict(d_in=None), dict(d_pos=None), dict(d_out=None), dict(d_ratio=None)):
        a = dict(good, **change)
        assert call(a["p"], a["d_in"], a["n_in"], a["d_pos"], a["d_out"], a["d_ratio"], stream) == VP_ERR_INVALID_ARG, change
        assert b"stretch locked" in st.L.vp_stft_last_error(st.h)
    assert call(None, good["d_in"], good["n_in"], good["d_pos"], good["d_out"], good["d_ratio"], stream) == VP_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_out).all())                                                # nothing was launched
    assert call(good["p"], good["d_in"], good["n_in"], good["d_pos"], good["d_out"], good["d_ratio"], stream) == 0
    torch.cuda.synchronize()
    st.close()
    assert np.array_equal(d_out.cpu().numpy(), want)
    T2 = 2048 + 5 * 512
    st2 = StftRoundTrip(2, T2, 2048, 512)
    i2, o2 = torch.zeros((2, T2), dtype=torch.float32, device="cuda"), torch.full((2, T2), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(VpError) as e:
        st2.time_stretch_locked(i2, o2, stretch=1.0)
    assert e.value.code == VP_ERR_GEOMETRY and "2048-point frames are not built" in str(e.value)
    torch.cuda.synchronize()
    st2.close()
    assert bool((o2 == 7.0).all())


def test_forty_calls_allocate_nothing_and_stretch_equals_d_pos():
    """stretch=, positions= and d_pos= are one table and give the same bits; semitones= (a scalar, a curve, a curve per stream) and
    d_ratio= likewise; the handle keeps one device table per shape, and forty calls leave the allocator's count of device blocks
    where it was."""
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios, stretch_positions
    hop, nF, n_in = 256, 19, 9001
    T = F + (nF - 1) * hop + 3
    x = np.stack([LC.SIGNALS[s](n_in, seed=3) for s in K.GPU_STREAMS])
    factors = np.array([0.25, 0.8, 1.0, 1.37, 4.0])
    semis = np.stack([np.log2(LC.curve("vibrato", nF, hop, s)) * 12.0 for s in range(K.N_STREAMS)])
    pos = np.stack([stretch_positions(nF, hop, a, n_in, F) for a in factors])
    st = StftRoundTrip(K.N_STREAMS, T, F, hop)
    d_in = _dev(x, np.float32)

    def run(**kw):
        o = _nan_out(st)
        st.time_stretch_locked(d_in, o, **kw)
        torch.cuda.synchronize()
        return o.cpu().numpy()
    y1 = run(stretch=factors, semitones=semis)
    y2 = run(d_pos=_dev(pos, np.int32), d_ratio=_dev(semitones_to_ratios(semis), np.float64))
    y3 = run(positions=pos, semitones=semis)
    assert np.array_equal(y1, y2) and np.array_equal(y1, y3) and np.all(np.isfinite(y1)) and np.abs(y1).max() > 0
    assert np.array_equal(run(stretch=1.37, semitones=semis[3]), run(positions=pos[3], d_ratio=_dev(np.tile(semitones_to_ratios(semis[3]), (K.N_STREAMS, 1)), np.float64)))
    assert np.array_equal(run(stretch=factors), run(stretch=factors, semitones=0.0))    # None means ones
    assert np.array_equal(run(stretch=factors, semitones=7.0), run(stretch=factors, semitones=np.full(nF, 7.0)))
    assert len(st._stretch_tables) == 1 and len(st._curve_tables) == 1                  # one table per handle and shape, shared with time_stretch
    tab = st._stretch_tables[(K.N_STREAMS, nF)]
    plain = _nan_out(st)
    st.time_stretch(d_in, plain, stretch=factors)
    assert st._stretch_tables[(K.N_STREAMS, nF)] is tab
    o = _nan_out(st)
    torch.cuda.synchronize()
    n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    for _ in range(40):
        st.time_stretch_locked(d_in, o, stretch=factors, semitones=semis)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0
    st.close()
    assert np.array_equal(o.cpu().numpy(), y1)


# ---- 7. what the stage is for -------------------------------------------------------------------------------------------------------------------------
def test_a_stretched_tone_keeps_an_even_envelope_and_lands_on_its_frequency():
    """The CPU quality test on the device: every (stretch, shift) pair of both tones in one launch per tone, beside the plain stretch."""
    from vocoderproject_amd import StftRoundTrip
    pairs = K.QUALITY_PAIRS
    for freq in K.QUALITY_TONES:
        setups = [K.quality_setup(freq, a) for a, _ in pairs]
        T, nF = setups[0][2], len(setups[0][1])
        n_in = max(len(x) for x, _, _ in setups)
        x = np.zeros((len(pairs), n_in), np.float32)
        for s, (xi, _, _) in enumerate(setups):
            x[s, :len(xi)] = xi
        pos = np.stack([p for _, p, _ in setups])
        st = StftRoundTrip(len(pairs), T, F, K.QUALITY_HOP)
        assert st.n_frames == nF
        yl = _locked(st, x, pos, np.stack([np.full(nF, K.ratio_of(v)) for _, v in pairs]))
        st.close()
        for s, (a, v) in enumerate(pairs):
            st1 = StftRoundTrip(1, T, F, K.QUALITY_HOP)
            d_out = torch.full((1, T), float("nan"), dtype=torch.float32, device="cuda")
            st1.time_stretch(_dev(x[s:s + 1], np.float32), d_out, positions=pos[s], semitones=v)
            torch.cuda.synchronize()
            yp = d_out.cpu().numpy()[0]
            st1.close()
            rl, al = LC.ripple(yl[s])
            rp, ap = LC.ripple(yp)
            fpk = K.peak_frequency(yl[s])
            print(f"STRETCHLOCK quality {freq} Hz x{a:g} {v:+g} st: ripple plain {rp:.4f} locked {rl:.4f} (ratio {rl / rp:.3f}), level plain {ap:.3f} locked {al:.3f}, "
                  f"peak {fpk:.2f} Hz")
            assert rl < rp, (freq, a, v, rl, rp)
            assert abs(fpk - freq * K.ratio_of(v)) <= 1.0, (freq, a, v, fpk)
