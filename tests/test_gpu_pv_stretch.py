"""The phase-vocoder time stretch on the GPU (include/vp_amd.h vp_stft_time_stretch; kernels vp_k_stft_pv_stretch and
vp_k_stft_pv2k_stretch of csrc/vp_stft_stretch.inc): against the NumPy reference of frames analysed at given positions on every case of
tests/pv_stretch_cases.py (whose conditioning tests/test_pv_stretch_reference_cpu.py gates), bit-identical to the fixed-grid kernels on
the table f hop, the clamp and the streams' independence, stretch= against d_pos=, more workgroups than compute units, and the neighbours
on the same handle."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_curve_cases as CC  # noqa: E402
import pv_stretch_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _stretch(st, x, semitones=0.0, **table):
    """One vp_stft_time_stretch call on x [S][n_in]; the output [S][T] starts as NaN, so every sample must have been written."""
    d_in = _dev(x, np.float32)
    d_out = torch.full((st.S, st.T), float("nan"), dtype=torch.float32, device="cuda")
    st.time_stretch(d_in, d_out, semitones=semitones, **table)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


# ---- 1. against NumPy -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.CASES, ids=SC.case_id)
def test_time_stretch_matches_numpy(c):
    from vocoderproject_amd import StftRoundTrip
    x, ref, T = SC.case_input(c), SC.reference(c), SC.out_length(c)
    st = StftRoundTrip(SC.N_STREAMS, T, c.F, c.hop)
    assert st.n_frames == c.nF and x.shape == (SC.N_STREAMS, SC.in_length(c))
    y = _stretch(st, x, c.semitones, positions=SC.positions(c))
    st.close()
    assert y.shape == (SC.N_STREAMS, T) and np.all(np.isfinite(y))
    for s in range(SC.N_STREAMS):
        err, bnd = np.abs(y[s] - ref[s]).max(), SC.bound(c, ref[s])
        print(f"STRETCH {SC.case_id(c)} stream {s}: err {err:.3g} bound {bnd:.3g}")
        assert err <= bnd, (s, err, bnd)
    covered = (c.nF - 1) * c.hop + c.F
    assert np.all(y[:, covered:] == 0) and y[:, covered:].shape[1] == c.extra            # samples no frame covers


# ---- 2. the table f hop is the fixed-grid kernel, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("F,hop", [(1024, 256), (1024, 512), (2048, 256), (2048, 512)])
def test_identity_table_is_bit_identical_to_pitch_shift(F, hop):
    from vocoderproject_amd import StftRoundTrip
    nF = 19
    T = F + (nF - 1) * hop + 3
    x = pv_cases.mixed_streams(T, seed=hop + 5)
    st = StftRoundTrip(SC.N_STREAMS, T, F, hop)
    d_in = _dev(x, np.float32)
    d_pos = _dev(np.tile(np.arange(nF) * hop, (SC.N_STREAMS, 1)), np.int32)
    for v in pv_cases.SEMITONES:
        o1, o2 = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
        st.time_stretch(d_in, o1, d_pos=d_pos, semitones=v)
        st.pitch_shift(d_in, o2, v)
        torch.cuda.synchronize()
        y, o = o1.cpu().numpy(), o2.cpu().numpy()
        assert np.all(np.isfinite(y)) and np.abs(y).max() > 0
        for s in range(SC.N_STREAMS):
            assert np.array_equal(y[s], o[s]), (v, s, np.abs(y[s] - o[s]).max())
    st.close()


# ---- 3. the clamp, and the streams' independence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1024, 2048])
def test_a_garbage_table_is_clamped_and_touches_no_other_stream(F):
    from vocoderproject_amd import StftRoundTrip
    c = SC.StretchCase(F, 256, 19, 3, 7.0)
    x, clean, n_in = SC.case_input(c), SC.positions(c), SC.in_length(c)
    rng = np.random.default_rng([F, 13])
    garbage = rng.integers(-3 * n_in, 3 * n_in, c.nF)
    garbage[:6] = [-1, -2 ** 31, 2 ** 31 - 1, n_in, n_in - F + 1, 5]                      # negative, beyond n_in, decreasing
    dirty, clipped = clean.astype(np.int64), clean.astype(np.int64)
    dirty[2], clipped[2] = garbage, np.clip(garbage, 0, n_in - F)
    assert np.any(np.diff(clipped[2]) < 0) and not np.array_equal(dirty[2], clipped[2])
    st = StftRoundTrip(SC.N_STREAMS, SC.out_length(c), F, 256)
    yd = _stretch(st, x, c.semitones, positions=dirty)                                  # (returns VP_OK: the wrapper raises otherwise)
    yc = _stretch(st, x, c.semitones, positions=clipped)
    y0 = _stretch(st, x, c.semitones, positions=clean)
    st.close()
    assert np.all(np.isfinite(yd))
    assert np.array_equal(yd[2], yc[2]) and not np.array_equal(yd[2], y0[2])
    for s in (0, 1, 3, 4):
        assert np.array_equal(yd[s], y0[s]), s


# ---- 4. stretch= against d_pos= ---------------------------------------------------------------------------------------------------------------
def test_stretch_factors_are_the_tables_of_stretch_positions():
    from vocoderproject_amd import StftRoundTrip, VpError, stretch_positions
    F, hop, nF, n_in = 1024, 256, 19, 9001
    T = F + (nF - 1) * hop + 3
    x = pv_cases.mixed_streams(n_in, seed=hop + 6)
    factors = np.array([0.25, 0.8, 1.0, 1.37, 4.0])
    st = StftRoundTrip(SC.N_STREAMS, T, F, hop)
    pos = np.stack([stretch_positions(nF, hop, a, n_in, F) for a in factors])
    y1 = _stretch(st, x, -3.0, stretch=factors)
    y2 = _stretch(st, x, -3.0, d_pos=_dev(pos, np.int32))
    y3 = _stretch(st, x, -3.0, positions=pos)
    assert len(st._stretch_tables) == 1                                                 # one table per handle and shape
    tab = st._stretch_tables[(SC.N_STREAMS, nF)]
    ya = _stretch(st, x, -3.0, stretch=1.37)                                            # a scalar: every stream
    yb = _stretch(st, x, -3.0, positions=pos[3])                                        # one row: every stream
    assert len(st._stretch_tables) == 1 and st._stretch_tables[(SC.N_STREAMS, nF)] is tab
    with pytest.raises(VpError):
        st.time_stretch(_dev(x, np.float32), torch.empty(SC.N_STREAMS, T, device="cuda"), stretch=4.5)
    with pytest.raises(VpError):
        st.time_stretch(_dev(x, np.float32), torch.empty(SC.N_STREAMS, T, device="cuda"), stretch=1.0, semitones=12.5)
    st.close()
    assert np.array_equal(y1, y2) and np.array_equal(y1, y3) and np.array_equal(ya, yb) and np.array_equal(ya[3], y1[3])
    assert not np.array_equal(y1[0], y1[4]) and np.all(np.isfinite(y1)) and np.abs(y1).max() > 0


# ---- 5. more workgroups than compute units ----------------------------------------------------------------------------------------------------
def test_three_hundred_streams_each_with_its_own_stretch():
    from vocoderproject_amd import StftRoundTrip
    x, ref = SC.big_input(), SC.big_reference()
    st = StftRoundTrip(SC.BIG_S, SC.BIG_T, SC.BIG_F, SC.BIG_HOP)
    assert st.n_frames == SC.BIG_NF
    y = _stretch(st, x, 0.0, stretch=SC.big_stretch())
    y2 = _stretch(st, x, 0.0, positions=SC.big_positions())
    st.close()
    assert np.all(np.isfinite(y)) and np.array_equal(y, y2)
    assert np.all(y[:, (SC.BIG_NF - 1) * SC.BIG_HOP + SC.BIG_F:] == 0)
    bnd_of = lambda r: 4.0 * (SC.BIG_F // SC.BIG_HOP) * 2.0 ** -24 * max(1.0, float(np.abs(r).max()))    # noqa: E731
    for s in SC.BIG_CHECKED:
        err, bnd = np.abs(y[s] - ref[s]).max(), bnd_of(ref[s])
        print(f"STRETCH big stream {s}: err {err:.3g} bound {bnd:.3g}")
        assert err <= bnd, (s, err, bnd)
    assert np.abs(y).max(axis=1).min() > 0                                              # every stream was written by its own workgroup


# ---- 6. the neighbours ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1024, 2048])
def test_neighbours_keep_their_bits_around_a_time_stretch_call(F):
    from vocoderproject_amd import StftRoundTrip
    c = CC.CurveCase(F, 512, 19, "steps")
    x = CC.case_input(c)
    T = CC.length(c)
    st = StftRoundTrip(CC.N_STREAMS, T, F, 512)
    d_in = _dev(x, np.float32)

    def three():
        o = [torch.full_like(d_in, float("nan")) for _ in range(3)]
        st(d_in, o[0])
        st.pitch_shift(d_in, o[1], -5.0)
        st.pitch_shift_curve(d_in, o[2], semitones=CC.semitones_of(c))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in o]
    before = three()
    y = _stretch(st, x, -5.0, stretch=[0.5, 0.8, 1.0, 1.37, 2.0])
    after = three()
    st.close()
    for a, b in zip(before, after):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    assert np.all(np.isfinite(y)) and not np.array_equal(y, before[1]) and np.array_equal(y[2], before[1][2])    # (stretch 1: stream 2 is the pitch shift)
