"""The two time-stretch kernels (vp_k_stft_pv_stretch, vp_k_stft_pv2k_stretch of csrc/vp_stft_stretch.inc) where they differ from their
fixed-grid parents: the clamp of a frame's position, the clamps of its analysis advance D_f = clamp(q_f - q_(f-1), 1, F), and the vector
load chosen per frame from the frame's address.  tests/test_gpu_pv_stretch.py advances by hop / 4 .. 2 hop and meets none of them against
NumPy.  Here: the edge tables of tests/pv_stretch_cases.py (EDGE_CASES: D = 1, 2, 3, F - 1 and F, clamped from both sides; q clamped at
both ends; every residue of a frame's address) against NumPy, the smallest inputs n_in = F and F + 1, translation of the input by one to
three samples, degenerate inputs, power-of-two homogeneity, the cached device table on a side stream, the C entry's error returns with
a live device, and the offline stretch flow with the real processor.  The references' conditioning and the teeth of every wrong clamp are
gated on the CPU (tests/test_pv_stretch_reference_cpu.py); every pointwise comparison is held at EVERY sample to
|y - ref| <= 4 O 2^-24 max(1, max |ref|),  O = F / hop.  Output buffers start as NaN."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_stretch_cases as SC  # noqa: E402
import pv_stretch_reference as SR  # noqa: E402

pytestmark = pytest.mark.gpu

GEOMETRIES = [(F, hop) for F in (1024, 2048) for hop in SC.HOPS[F]]
VP_ERR_INVALID_ARG = -1


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _nan_out(st):
    return torch.full((st.S, st.T), float("nan"), dtype=torch.float32, device="cuda")


def _stretch(st, x, semitones, positions):
    """One vp_stft_time_stretch call on x [S][n_in]; the output [S][T] starts as NaN, so every sample must have been written."""
    d_in, d_out = _dev(x, np.float32), _nan_out(st)
    st.time_stretch(d_in, d_out, positions=positions, semitones=semitones)
    torch.cuda.synchronize()
    y = d_out.cpu().numpy()
    assert np.all(np.isfinite(y)), f"{int((~np.isfinite(y)).sum())} samples unwritten or not finite"
    return y


def _one_call(x, F, hop, T, semitones, positions):
    from vocoderproject_amd import StftRoundTrip
    st = StftRoundTrip(x.shape[0], T, F, hop)
    try:
        return _stretch(st, x, semitones, positions)
    finally:
        st.close()


def _bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), what
    if not np.array_equal(a, b):
        d = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(d)} samples differ, first at {d[0]}, max {np.abs(a.astype(np.float64) - b).max():.3g}")


def _pointwise(c, what, y, ref):
    """Every stream at every sample within the bound; one line per stream for profiles/pv_stretch_errors.txt."""
    bad = []
    for s, row in enumerate(SC.EDGE_ROWS):
        e = np.abs(y[s].astype(np.float64) - ref[s])
        bnd = SC.bound(c, ref[s])
        print(f"STRETCHEDGE {what} {row}: err {e.max():.3g} bound {bnd:.3g} rms {np.sqrt((e ** 2).mean()):.3g}")
        if e.max() > bnd:
            bad.append((row, float(e.max()), bnd, int(np.argmax(e))))
    assert not bad, (what, bad)


# ---- a. the edge tables against NumPy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.EDGE_CASES, ids=SC.case_id)
def test_edge_tables_match_numpy(c):
    x, pos, ref, T = SC.edge_input(c), SC.edge_positions(c), SC.edge_reference(c), SC.out_length(c)
    assert x.shape == (SC.EDGE_STREAMS, SC.edge_in_length(c)) and (T - c.F) // c.hop + 1 == c.nF
    y = _one_call(x, c.F, c.hop, T, c.semitones, pos)
    assert y.shape == (SC.EDGE_STREAMS, T) and y.dtype == np.float32
    _pointwise(c, SC.case_id(c), y, ref)
    covered = (c.nF - 1) * c.hop + c.F
    assert np.all(y[:, covered:] == 0) and y[:, covered:].shape[1] == c.extra              # samples no frame covers


# ---- b. the smallest inputs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", SC.SMALL_CASES, ids=SC.small_id)
def test_smallest_inputs_match_numpy(cn):
    """n_in = F: qm = 0, every table is a freeze at 0, and the six rows given ONE input row are the same bits.  n_in = F + 1: positions 0
    and 1 only."""
    c, n_in = cn
    x, pos, ref, T = SC.edge_input(c, n_in), SC.edge_positions(c, n_in), SC.edge_reference(c, n_in=n_in), SC.out_length(c)
    assert x.shape == (SC.EDGE_STREAMS, n_in)
    y = _one_call(x, c.F, c.hop, T, c.semitones, pos)
    _pointwise(c, SC.small_id(cn), y, ref)
    assert np.all(y[:, (c.nF - 1) * c.hop + c.F:] == 0)
    if n_in == c.F:
        same = _one_call(np.stack([x[0]] * SC.EDGE_STREAMS), c.F, c.hop, T, c.semitones, pos)
        _bits(same[0], y[0], "stream 0 beside copies of itself")
        for s in range(1, SC.EDGE_STREAMS):
            _bits(same[s], same[0], f"{SC.small_id(cn)}: row {SC.EDGE_ROWS[s]} against freeze")


# ---- c. translation ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1024, 2048])
def test_a_shifted_input_and_table_give_the_same_bits(F):
    """c zeros in front of every input row and every position raised by c: the same frames at every other alignment of their addresses
    (and with other row starts) are the same samples, whichever load fetches them.  In-range tables only (a shifted negative position
    clamps elsewhere): crawl, skew and the first matrix's five tables."""
    from vocoderproject_amd import StftRoundTrip
    c = SC.StretchCase(F, 256, 19, 3, 7.0)
    x5, n_in = SC.case_input(c), SC.in_length(c)
    edge = SC.edge_positions(c)
    pos = np.concatenate([edge[[2, 5]], SC.positions(c).astype(np.int64)])
    x = np.ascontiguousarray(x5[[0, 1, 0, 1, 2, 3, 4]])
    assert pos.min() == 0 and pos.max() + F <= n_in and {int(v) % 4 for v in pos[1]} == {0, 1, 2, 3}
    st = StftRoundTrip(len(pos), SC.out_length(c), F, c.hop)
    y0 = _stretch(st, x, c.semitones, pos)
    assert np.abs(y0).max(axis=1).min() > 0.01
    for k in (1, 2, 3):
        xk = np.concatenate([np.zeros((len(pos), k), np.float32), x], axis=1)
        _bits(_stretch(st, xk, c.semitones, pos + k), y0, f"F {F}: input and table shifted by {k}")
    st.close()


# ---- d. degenerate inputs ------------------------------------------------------------------------------------------------------------------------
def _table_ceiling(x, q, F):
    """pv_cases.magnitude_ceiling over the frames x[q_f : q_f + F] that a table reads."""
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(F) / F))
    x = np.asarray(x, np.float64)
    m = max(float(np.abs(np.fft.rfft(x[v:v + F] * w)).sum()) for v in sorted(set(int(v) for v in q)))
    return 2.0 * (2.0 * m / F)


@pytest.mark.parametrize("F", [1024, 2048])
@pytest.mark.parametrize("name", pv_cases.DEGENERATE)
def test_degenerate_inputs_along_the_edge_tables(name, F):
    """Silence, DC, a Nyquist tone, two clicks and a square wave sit on wrap ties where no pointwise reference exists.  Along crawl, leap,
    reverse and a stretch of 0.5: every sample is finite, silence gives exact zeros and |y| <= 2 Mf (1 + 1e-6) (a frame's inverse transform
    is bounded by its magnitude sum whatever its advance is: pv_cases.magnitude_ceiling, over the frames the table reads)."""
    c = SC.StretchCase(F, 256, 19, 3, 7.0)
    n_in, T = SC.edge_in_length(c), SC.out_length(c)
    edge = SC.edge_positions(c)
    pos = np.stack([edge[2], edge[3], edge[1], SR.stretch_positions(c.nF, c.hop, 0.5, n_in, F).astype(np.int64)])
    x1 = pv_cases.degenerate(name, n_in)
    x = np.stack([x1] * len(pos))
    for v in SC.EDGE_SEMITONES:
        y = _one_call(x, F, c.hop, T, v, pos)
        if name == "silence":
            assert np.all(y == 0)
        for s in range(len(pos)):
            top = _table_ceiling(x1, SR.clamp_positions(pos[s], n_in, F), F) * (1 + 1e-6)
            print(f"STRETCHDEG {name} F{F} {v:+g}st table {s}: max |y| {np.abs(y[s]).max():.4f} ceiling {top:.4f}")
            assert np.abs(y[s]).max() <= top, (s, v)


# ---- e. power-of-two homogeneity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,hop", GEOMETRIES, ids=lambda v: str(v))
def test_power_of_two_homogeneity_along_the_edge_tables(F, hop):
    """The output for x 2^e is the output for x times 2^e, bit for bit, along the six edge tables."""
    from vocoderproject_amd import StftRoundTrip
    c = SC.StretchCase(F, hop, 19, 3, 7.0)
    x, pos = SC.edge_input(c), SC.edge_positions(c)
    st = StftRoundTrip(SC.EDGE_STREAMS, SC.out_length(c), F, hop)
    y0 = _stretch(st, x, c.semitones, pos)
    assert np.abs(y0).max(axis=1).min() > 0.01
    for e in (-40, 12):
        k = np.float32(2.0 ** e)
        _bits(_stretch(st, x * k, c.semitones, pos), y0 * k, f"F {F} hop {hop}: x 2^{e}")
    st.close()


# ---- f. the cached table and stream order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1024, 2048])
def test_two_tables_of_one_shape_back_to_back_on_a_side_stream(F):
    """positions= uploads into one device table per handle and shape.  Two calls of the same shape and different tables, issued on a side
    stream behind a matrix product without synchronising, each give the bits of a synchronised run of their table: the second upload is
    ordered behind the first kernel."""
    from vocoderproject_amd import StftRoundTrip
    c = SC.StretchCase(F, 256, 19, 3, 7.0)
    x, p1, T = SC.edge_input(c), SC.edge_positions(c), SC.out_length(c)
    p2 = np.ascontiguousarray(p1[::-1])
    want1, want2 = _one_call(x, F, c.hop, T, c.semitones, p1), _one_call(x, F, c.hop, T, c.semitones, p2)
    assert not np.array_equal(want1, want2)
    st = StftRoundTrip(SC.EDGE_STREAMS, T, F, c.hop)
    d_in = _dev(x, np.float32)
    o1, o2 = _nan_out(st), _nan_out(st)
    busy = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = busy @ busy * 1e-3
        st.time_stretch(d_in, o1, positions=p1, semitones=c.semitones)
        st.time_stretch(d_in, o2, positions=p2, semitones=c.semitones)
    side.synchronize()
    assert len(st._stretch_tables) == 1
    st.close()
    _bits(o1.cpu().numpy(), want1, f"F {F}: first table")
    _bits(o2.cpu().numpy(), want2, f"F {F}: second table")


# ---- g. errors with a live device ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1024, 2048])
def test_bad_arguments_return_invalid_arg_and_write_nothing(F):
    """Through the raw C entry, on a handle that has run and runs again: a short input, an interval outside +-12 or not a number, and each
    pointer NULL in turn return VP_ERR_INVALID_ARG and launch nothing; a valid call on the same handle then still gives its bits."""
    from vocoderproject_amd import StftRoundTrip
    c = SC.StretchCase(F, 256, 6, 2, 7.0)
    x, pos, n_in = SC.edge_input(c), SC.edge_positions(c), SC.edge_in_length(c)
    st = StftRoundTrip(SC.EDGE_STREAMS, SC.out_length(c), F, c.hop)
    want = _stretch(st, x, c.semitones, pos)
    d_in, d_pos, d_out = _dev(x, np.float32), _dev(np.clip(pos, SC.INT_MIN, SC.INT_MAX), np.int32), _nan_out(st)
    stream = torch.cuda.current_stream().cuda_stream
    call = st.L.vp_stft_time_stretch
    good = dict(p=st.h, d_in=d_in.data_ptr(), n_in=n_in, d_pos=d_pos.data_ptr(), d_out=d_out.data_ptr(), semitones=c.semitones)
    bad = [dict(n_in=F - 1), dict(semitones=12.5), dict(semitones=float("nan")), dict(p=None), dict(d_in=None), dict(d_pos=None), dict(d_out=None)]
    for change in bad:
        a = dict(good, **change)
        rc = call(a["p"], a["d_in"], a["n_in"], a["d_pos"], a["d_out"], a["semitones"], stream)
        assert rc == VP_ERR_INVALID_ARG, (change, rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_out).all())                                                  # nothing was launched
    assert call(good["p"], good["d_in"], good["n_in"], good["d_pos"], good["d_out"], good["semitones"], stream) == 0
    torch.cuda.synchronize()
    st.close()
    _bits(d_out.cpu().numpy(), want, f"F {F}: a valid call behind the refused ones")


# ---- h. the offline flow with the real processor ---------------------------------------------------------------------------------------------------
class _Recorder:
    """The offline flow's processor that only keeps what the flow built."""

    def run(self, x, pos, T, semitones):
        self.seen = (x.copy(), pos.copy(), T, semitones)
        return np.zeros((x.shape[0], T), np.float32)


def test_offline_stretch_is_the_direct_call_on_what_it_builds():
    """Three recordings -- longer than a frame, barely longer, shorter than a frame -- stretched by 1.5, 0.5 and 4.0 and shifted by +3:
    offline.pv_stretch with the real processor gives the lengths the CPU test asserts, L == R, and the bits of a direct time_stretch call
    on the padded batch and the table the flow builds, trimmed the same way."""
    from vocoderproject_amd import offline
    sig = pv_cases.mixed_streams(5000, seed=3)
    v = [sig[0], sig[2][:1700].copy(), sig[4][:300].copy()]
    stretch = [1.5, 0.5, 4.0]
    rec = _Recorder()
    offline.pv_stretch(v, stretch, shift=3.0, processor=rec)
    x, pos, T, semis = rec.seen
    assert x.shape == (3, 5000) and pos.shape == (3, (T - 1024) // 256 + 1) and semis == 3.0
    out = offline.pv_stretch(v, stretch, shift=3.0)
    assert [o.shape for o in out] == [(2, 7500), (2, 850), (2, 1200)] and all(o.dtype == np.float32 for o in out)
    y = _one_call(x, 1024, 256, T, 3.0, pos)
    for s, o in enumerate(out):
        np.testing.assert_array_equal(o[0], o[1])
        _bits(o[0], y[s, :o.shape[1]], f"recording {s}")
        assert np.abs(o).max() > 0.05


def test_offline_stretch_of_one_is_the_pvshift_flow_while_whole_frames_last():
    """Stretch 1.0 of a recording of whole frames (F + m hop samples) against offline.pv_shift (the streaming kernel, block by block), same
    shift: bit for bit on the (m + 1) hop samples that only frames 0 .. m reach.  Behind them the two flows are DEFINED differently: the
    frames past the recording's last whole frame read padding zeros in the stream, and the stretch table holds them at the recording's
    last frame (pos = min(f hop, len - F)), so the last F - hop samples cannot be compared."""
    from vocoderproject_amd import offline
    F, hop, m = 1024, 256, 12
    n = F + m * hop
    v = [pv_cases.mixed_streams(n, seed=4)[0], pv_cases.mixed_streams(n, seed=4)[1]]
    a = offline.pv_stretch(v, 1.0, shift=3.0, F=F, hop=hop)
    b = offline.pv_shift(v, 3.0, N=1024, hop=hop)
    done = (m + 1) * hop
    assert done == n - (F - hop)
    for s in range(len(v)):
        assert a[s].shape == b[s].shape == (2, n)
        print(f"STRETCHOFFLINE recording {s}: {int((a[s][0][done:] != b[s][0][done:]).sum())} of the last {n - done} samples differ")
        _bits(a[s][0][:done], b[s][0][:done], f"recording {s}: stretch 1 against pvshift")
        assert np.abs(a[s][0][:done]).max() > 0.05
