"""The phase-vocoder pitch shift for 2048-point frames on the GPU (vp_stft_pitch_shift on a handle with frame_len = 2048; kernel
vp_k_stft_pv2k of csrc/vp_stft.hip) against NumPy at every hop, length and edge.  The cases and the reference come from
tests/pv2k_cases.py, the list whose conditioning tests/test_pv2k_reference_cpu.py gates; every pointwise comparison is held at EVERY
sample to
    |y - ref| <= 4 O 2^-24 max(1, max |ref|),   O = 2048 / hop
(float32 output frames and float32 overlap-add of O terms; pv_cases.py derives it, nothing in it depends on F).  Degenerate inputs sit
on wrap ties where no pointwise reference exists; they are held to properties that do not depend on a wrap decision.  Output buffers
start as NaN: an unwritten sample shows."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv2k_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

F = K.F


def _device(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _one_shot(x, semis, hop, handle=None):
    """vp_stft_pitch_shift on x [S][T]; semis: one interval, or one per stream (then one batch call per distinct interval)."""
    from vocoderproject_amd import StftRoundTrip
    S, T = x.shape
    st = handle or StftRoundTrip(S, T, F, hop)
    assert st.fused
    per_stream = [float(semis)] * S if np.isscalar(semis) else [float(v) for v in semis]
    d_in = _device(x)
    y = np.full_like(x, np.nan)
    for v in sorted(set(per_stream)):
        d_out = torch.full_like(d_in, float("nan"))
        st.pitch_shift(d_in, d_out, v)
        torch.cuda.synchronize()
        o = d_out.cpu().numpy()
        for s in range(S):
            if per_stream[s] == v:
                y[s] = o[s]
    if handle is None:
        st.close()
    return y


def _roundtrip(st, x):
    d_in = _device(x)
    d_out = torch.full_like(d_in, float("nan"))
    st(d_in, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _bits(a, b, what):
    assert a.shape == b.shape, what
    assert not np.isnan(a).any() and not np.isnan(b).any(), what
    if not np.array_equal(a, b):
        d = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(d)} samples differ, first at {d[0]}, max {np.abs(a.astype(np.float64) - b).max():.3g}")


# ---- a. the one-shot against NumPy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.ONE_SHOT_CASES, ids=K.one_shot_id)
def test_one_shot_against_numpy(case):
    x = K.one_shot_input(case)
    y = _one_shot(x, case.semitones, case.hop)
    ref = K.one_shot_reference(case, x)
    what = f"one-shot {K.one_shot_id(case)} ({case.what})"
    assert y.shape == ref.shape and y.dtype == np.float32
    assert not np.isnan(y).any(), f"{what}: {int(np.isnan(y).sum())} samples unwritten or NaN, first at {np.argwhere(np.isnan(y))[0]}"
    err = np.abs(y.astype(np.float64) - ref)
    bnd = K.bound(case.hop, ref)
    rms = float(np.sqrt((err ** 2).mean()))
    share = float((err > 1e-5).mean())
    print(f"PV2K {what} max_err {err.max():.3e} bound {bnd:.3e} err/bound {err.max() / bnd:.3f} rms {rms:.3e} share>1e-5 {share:.2e}")
    if err.max() > bnd:
        s, t = np.unravel_index(np.argmax(err), err.shape)
        f_lo, f_hi = max(0, (t - F) // case.hop + 1), t // case.hop
        raise AssertionError(f"{what}: {int((err > bnd).sum())} samples beyond the bound {bnd:.3e}; worst {err.max():.3e} at stream {s} "
                             f"sample {t} (frames {f_lo}..{f_hi} cover it), y {y[s, t]!r} ref {ref[s, t]!r}; first bad sample "
                             f"{np.argwhere(err > bnd)[0]}")
    assert rms < 1e-4 and share < 1e-3, (what, rms, share)
    covered = (K.n_frames(case.T, case.hop) - 1) * case.hop + F
    assert np.all(y[:, covered:] == 0), "samples no frame covers must come out 0"
    assert np.sqrt((ref ** 2).mean()) > 0.01                                    # (a comparison of something)


# ---- b. degenerate inputs ---------------------------------------------------------------------------------------------------------------
DEG_SEMIS = (7.0, -12.0, 0.37, 12.0)


@pytest.mark.parametrize("hop", K.HOPS)
@pytest.mark.parametrize("name", ("silence", "dc", "nyquist", "impulses", "square"))
def test_degenerate_inputs(name, hop):
    """Silence gives exact zeros.  DC, a Nyquist tone, two clicks and a square wave sit on wrap ties, so: every sample finite and
    |y| <= 2 Mf (1 + 1e-6) -- a frame's inverse transform is bounded by its magnitude sum, the overlap-add weighs at most O frames by
    w <= 1 and 2 / O.  One odd length (scalar loads) and one of whole frames (float4 loads)."""
    for T in (8 * F + hop + 3, 9 * F):
        x = np.stack([K.degenerate(name, T)] * len(DEG_SEMIS))
        y = _one_shot(x, DEG_SEMIS, hop)
        assert np.isfinite(y).all(), (name, hop, T)
        if name == "silence":
            assert np.all(y == 0)
        top = K.magnitude_ceiling(x[0], hop) * (1 + 1e-6)
        print(f"PV2K degenerate {name} hop{hop} T{T}: max |y| {np.abs(y).max():.4f} ceiling {top:.4f}")
        assert np.abs(y).max() <= top


# ---- c. power-of-two homogeneity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", K.HOPS)
def test_power_of_two_homogeneity(hop):
    """Every operation of the stage commutes with a power-of-two scale while nothing under- or overflows: the output for x 2^e is the
    output for x times 2^e, bit for bit.  An absolute threshold or a single-precision intermediate would break it."""
    x = K.mixed_streams(28 * 256 + 1 + F, seed=hop)
    semis = K.SEMITONES
    y0 = _one_shot(x, semis, hop)
    assert np.abs(y0).max() > 0.1
    for e in (-40, 12):
        c = np.float32(2.0 ** e)
        _bits(_one_shot(x * c, semis, hop), y0 * c, f"hop {hop}: x 2^{e}")


# ---- d. rows and batch size ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", K.HOPS)
def test_rows_are_independent(hop):
    """Permuting the S input rows permutes the output rows, bit for bit (odd T: odd rows start unaligned)."""
    S = 37
    perm = np.random.default_rng(hop).permutation(S)
    x = K.harmonic_streams(S, 5 * F + hop + 1, seed=hop)
    assert x.shape[1] % 2 == 1
    x[5] = K.white(x.shape[1], seed=hop)
    y = _one_shot(x, -5.0, hop)
    _bits(_one_shot(np.ascontiguousarray(x[perm]), -5.0, hop), y[perm], f"hop {hop}: rows")
    assert np.abs(y).max() > 0.1


def test_a_batch_of_more_workgroups_than_compute_units():
    """261 rows (the chip has 256 compute units and a workgroup owns one), the 37 harmonic rows repeated: every copy gets the same bits."""
    hop, S = 512, 37
    x = K.harmonic_streams(S, 5 * F + hop + 1, seed=hop)
    y = _one_shot(x, -5.0, hop)
    idx = np.arange(261) % S
    yb = _one_shot(np.ascontiguousarray(x[idx]), -5.0, hop)
    _bits(yb, y[idx], "261 rows")
    assert np.abs(y).max() > 0.1


# ---- e. no state survives a call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", K.HOPS)
def test_no_state_survives_a_call(hop):
    from vocoderproject_amd import StftRoundTrip
    x = K.mixed_streams(6 * F + hop + 3, seed=hop + 9)
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    first = _one_shot(x, 7.0, hop, handle=st)
    second = _one_shot(x, -5.0, hop, handle=st)
    third = _one_shot(x, 7.0, hop, handle=st)
    st.close()
    _bits(first, _one_shot(x, 7.0, hop), f"hop {hop}: first call against a fresh handle")
    _bits(third, first, f"hop {hop}: the first interval again")
    assert not np.array_equal(first, second)


# ---- f. it shifts ---------------------------------------------------------------------------------------------------------------------------
def test_a_tone_moves_by_the_interval():
    hop, T, semis = 512, 16 * F, 7.0
    x = K.tone(T, 440.0, 0.4, seed=1)[None, :]
    y = _one_shot(x, semis, hop)[0].astype(np.float64)
    n = 8192
    seg = y[4 * F:4 * F + n]                                                  # the interior: every sample under O full frames
    spec = np.abs(np.fft.rfft(seg * np.hanning(n)))
    peak = int(np.argmax(spec))
    want = 440.0 * 2.0 ** (semis / 12.0) * n / K.FS
    print(f"PV2K tone: peak bin {peak} expected {want:.2f} rms {np.sqrt((seg ** 2).mean()):.3f}")
    assert abs(peak - want) <= 1.0
    assert np.sqrt((seg ** 2).mean()) > 0.1


# ---- g. neighbours unchanged ---------------------------------------------------------------------------------------------------------------
def test_the_neighbours_are_unchanged():
    """The round trip on the same handle gives the same bits before and after a pitch shift (the launcher's branch order: the stage's
    build only when asked for; no state shared between the two entry points); the precision switch does not reach the pitch shift;
    the streaming entry point still refuses 2048-point frames."""
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, VpError
    hop = 512
    x = K.mixed_streams(6 * F + hop + 1, seed=3)
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    before = _roundtrip(st, x)
    shifted = _one_shot(x, 7.0, hop, handle=st)
    after = _roundtrip(st, x)
    _bits(after, before, "round trip before and after a pitch shift")
    inner = slice(F, x.shape[1] - F)
    assert np.abs(before[:, inner] - x[:, inner]).max() < 1e-5                  # (the identity, not the stage)
    assert not np.array_equal(shifted, before) and np.abs(shifted).max() > 0.1
    st.set_precision("f32")
    _bits(_one_shot(x, 7.0, hop, handle=st), shifted, "pitch shift under f32")
    st.close()
    with pytest.raises(VpError) as e:
        PhaseVocoderStream(2, 256, frame_len=2048)
    assert e.value.code == -4                                                   # VP_ERR_GEOMETRY
