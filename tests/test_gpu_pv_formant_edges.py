"""The two formant kernels (vp_k_stft_pv_formant, vp_k_pv_stream_formant of csrc/vp_stft_formant.inc) where the additions marked "formant:"
can be wrong and tests/test_gpu_pv_formant.py, by its own design, does not look: the gain's clamp on both sides on bins that carry energy,
the top of the envelope's interpolation, the floor of the logarithm at quiet and at large levels and across a level step, every lifter the
entry accepts, the streaming kernel bit-identical to the one-shot at every hop and block size and against NumPy at hop 64, with calls
without a frame and with many rounds in a call, through a schedule of formant, curve and plain calls with interval changes and resets,
and on 300 streams, degenerate inputs, and the cached formant table's order on a side stream.
The cases and references come from tests/pv_formant_cases.py, whose conditioning tests/test_pv_formant_edges_cpu.py gates; every pointwise
comparison is held at EVERY sample to  |y - ref| <= 4 O 2^-24 max(1, max |ref|),  O = F / hop -- on the level cases without the max(1, .)
(pv_formant_cases.level_bound).  Output buffers start as NaN."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_curve_cases as CC  # noqa: E402
import pv_formant_cases as FC  # noqa: E402

pytestmark = pytest.mark.gpu

S, F = FC.N_STREAMS, FC.F


# ---- running the entry points -----------------------------------------------------------------------------------------------------------------
def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _formant(st, x, ratio, phi, nc):
    """One pitch_shift_formant call on x [S][T] with device tables of ratios; every sample must have been written."""
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    st.pitch_shift_formant(d_in, d_out, d_ratio=_dev(ratio, np.float64), d_formant=_dev(phi, np.float64), lifter=nc)
    torch.cuda.synchronize()
    y = d_out.cpu().numpy()
    assert np.all(np.isfinite(y)), f"{int((~np.isfinite(y)).sum())} samples unwritten or not finite"
    return y


def _one_shot(x, hop, ratio, phi, nc):
    from vocoderproject_amd import StftRoundTrip
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    assert st.n_frames == np.asarray(ratio).shape[1]
    y = _formant(st, x, ratio, phi, nc)
    st.close()
    return y


def _one_shot_curve(x, hop, ratio):
    from vocoderproject_amd import StftRoundTrip
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    st.pitch_shift_curve(d_in, d_out, d_ratio=_dev(ratio, np.float64))
    torch.cuda.synchronize()
    st.close()
    return d_out.cpu().numpy()


def _blocks(x, N):
    n, T = x.shape
    return _dev(x.reshape(n, T // N, N).transpose(1, 0, 2), np.float32)


def _rows(d):
    nb, n, N = d.shape
    return d.cpu().numpy().transpose(1, 0, 2).reshape(n, nb * N)


def _stream(x, N, hop, tab, phi, nc, calls=FC.STREAM_CALLS):
    """x [S][N n_blocks] through a fresh handle's formant calls of calls[i % len] blocks, block b with the ratios tab[b] [S], without
    synchronising between the calls.  The calls allocate nothing.  Returns the output and the latency."""
    from vocoderproject_amd import PhaseVocoderStream
    ps = PhaseVocoderStream(x.shape[0], N, hop=hop)
    d_in = _blocks(x, N)
    d_out = torch.full_like(d_in, float("nan"))
    d_tab, d_phi = _dev(tab, np.float64), _dev(phi, np.float64)
    n0, b = ps.debug_alloc_count(), 0
    for k in pv_cases.call_spans(d_in.shape[0], calls):
        ps.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k, d_ratio=d_tab[b:b + k], d_formant=d_phi, lifter=nc)
        b += k
    torch.cuda.synchronize()
    assert ps.debug_alloc_count() == n0 and n0 > 0
    L = ps.latency
    ps.close()
    y = _rows(d_out)
    assert np.all(np.isfinite(y)), f"{int((~np.isfinite(y)).sum())} samples unwritten or not finite"
    assert L == pv_cases.latency(N, hop) and np.all(y[:, :L] == 0)                                 # zeros during the latency
    return y, L


def _pointwise(what, y, ref, bound_of, streams=None):
    """Every stream at every sample within bound_of(ref[s]); one line per stream for profiles/pv_formant_errors.txt."""
    assert y.shape == ref.shape and y.dtype == np.float32
    bad = []
    for s in range(y.shape[0]):
        e = np.abs(y[s].astype(np.float64) - ref[s])
        bnd = bound_of(ref[s])
        print(f"FORMANTEDGE {what} stream {streams[s] if streams else s}: err {e.max():.3g} bound {bnd:.3g} ratio {e.max() / bnd:.3f} rms {np.sqrt((e ** 2).mean()):.3g}")
        if not e.max() <= bnd:
            bad.append((s, float(e.max()), bnd, int(np.argmax(e))))
    assert not bad, (what, bad)


def _bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), what
    if not np.array_equal(a, b):
        d = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(d)} samples differ, first at {d[0]}, max {np.abs(a.astype(np.float64) - b).max():.3g}")


def _stream_is_the_one_shot(what, x, N, hop, tab, phi, nc):
    """The streaming kernel's output is the one-shot's on the same samples, with the per-block table expanded per frame, delayed by the
    latency, bit for bit on every finished one-shot sample the stream has emitted.  Returns both."""
    T = x.shape[1]
    per_frame = FC.per_frame(tab, N, hop, T)
    y1 = _one_shot(x, hop, per_frame, phi, nc)
    y2, L = _stream(x, N, hop, tab, phi, nc)
    n = min(per_frame.shape[1] * hop, T - L)
    assert n > F
    _bits(y2[:, L:L + n], y1[:, :n], what)
    return y1, y2


# ---- 1. the clamp, both signs, on bins that carry energy --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.CLAMP_CASES, ids=FC.case_id)
def test_clamp_cases_match_numpy(c):
    """A 60 dB step in the spectrum: a fifth to a third of the (frame, bin) pairs sit at the + clamp on the streams with phi = 2, a tenth
    to a quarter at the - clamp on those with phi = 1/2 and 2^(-5/12), on content far above the bound (the CPU file asserts the shares,
    and that a clamp at ln 8, at 24 dB = 2.763 or with either side missing is outside the bound)."""
    y = _one_shot(FC.clamp_input(c), c.hop, FC.ratios_of(c), FC.CLAMP_PHIS, c.nc)
    _pointwise(f"clamp {FC.case_id(c)}", y, FC.clamp_reference(c), lambda r: FC.bound(c, r))


# ---- 2. the top of the interpolation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.TOP_CASES, ids=FC.top_id)
def test_top_cases_match_numpy(c):
    """phi = 1/2 and energy in frame bins 496 .. 512: every synthesis bin from 256 on reads the envelope at the clip (i0 = 511, t = 1,
    le[512]), where the envelope is steep."""
    y = _one_shot(FC.top_input(c), c.hop, FC.top_ratios(c), FC.TOP_PHIS, c.nc)
    _pointwise(f"top {FC.top_id(c)}", y, FC.top_reference(c), lambda r: pv_cases.bound(c.hop, r))


# ---- 3. levels: the floor -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.LEVEL_CASES, ids=FC.level_id)
def test_level_cases_match_numpy(c):
    """x 2^e: the floor m^2 + 1e-12 makes the stage non-homogeneous, and the bound here has no max(1, .) (pv_formant_cases.level_bound)."""
    y = _one_shot(FC.level_input(c), c.hop, FC.ratios_of(FC._level_case(c)), FC.FORMANT_RATIOS, FC.LEVEL_NC)
    _pointwise(f"level {FC.level_id(c)}", y, FC.level_reference(c), lambda r: FC.level_bound(c.hop, r))


def test_level_step_inside_frames_matches_numpy():
    """The first F + 300 and the last 700 samples 2^-22 times the rest: within the committed bound everywhere, and on the output's first
    512 samples, which only the two wholly quiet frames cover, within the level bound of that part."""
    c = FC.STEP_CASE
    y, ref = _one_shot(FC.step_input(), c.hop, FC.ratios_of(c), FC.FORMANT_RATIOS, c.nc), FC.step_reference()
    _pointwise("step", y, ref, lambda r: FC.bound(c, r))
    q = FC.STEP_QUIET
    _pointwise("step quiet head", y[:, :q], ref[:, :q], lambda r: FC.level_bound(c.hop, r))


def test_silence_in_front_of_an_onset():
    """Exact digital silence in front of an onset fails the gate (the all-zero frame's wrap ties; tests/test_pv_formant_edges_cpu.py), so
    there is no pointwise reference: the output is finite, exactly zero where every covering frame is silent, and the streaming kernel's
    bits are the one-shot's."""
    c, N, nb = FC.STEP_CASE, 100, 33
    x = np.ascontiguousarray(FC.silence_onset_input()[:, :N * nb])
    tab = pv_cases.ratio_of(np.stack([CC.steps(c.hop, s, nb) for s in range(S)]).T)
    y1, y2 = _stream_is_the_one_shot("silent onset", x, N, c.hop, tab, FC.FORMANT_RATIOS, c.nc)
    assert np.all(y1[:, :FC.STEP_QUIET] == 0) and np.abs(y1).max() > 0.1
    assert np.all(y2[:, :pv_cases.latency(N, c.hop) + FC.STEP_QUIET] == 0)


# ---- 4. every lifter ----------------------------------------------------------------------------------------------------------------------------
def test_every_lifter_matches_numpy():
    """Lifters 4 .. 64 on one handle, one call each."""
    from vocoderproject_amd import StftRoundTrip
    c = FC.LIFTER_CASE
    x, ratio = FC.case_input(c), FC.ratios_of(c)
    st = StftRoundTrip(S, FC.length(c), F, c.hop)
    for nc in FC.ALL_LIFTERS:
        _pointwise(f"lifter {nc}", _formant(st, x, ratio, FC.FORMANT_RATIOS, nc), FC.lifter_reference(nc), lambda r: pv_cases.bound(c.hop, r))
    st.close()


# ---- 5. the streaming kernel ----------------------------------------------------------------------------------------------------------------------
STREAM_BIT = [(c, FC.STREAM_BIT_LIFTERS[i % 3]) for i, c in enumerate(CC.STREAM_CURVE_CASES)]


@pytest.mark.parametrize("c,nc", STREAM_BIT, ids=[f"{CC.stream_curve_id(c)}-nc{nc}" for c, nc in STREAM_BIT])
def test_streaming_is_bit_identical_to_the_one_shot_at_every_hop_and_block_size(c, nc):
    x, tab = CC.stream_curve_input(c), pv_cases.ratio_of(CC.stream_curve_semitones(c))
    _, y2 = _stream_is_the_one_shot(CC.stream_curve_id(c), x, c.N, c.hop, tab, FC.FORMANT_RATIOS, nc)
    assert np.abs(y2).max() > 0.05


@pytest.mark.parametrize("c", FC.STREAM_EDGE_CASES, ids=FC.stream_id)
def test_streaming_edges_match_numpy(c):
    """Against the NumPy definition driven block by block: hop 64, blocks of 17 samples (calls without a frame), blocks of 4096 (many
    rounds in a call)."""
    y, _ = _stream(FC.stream_input(c), c.N, c.hop, pv_cases.ratio_of(FC.stream_semitones(c)), FC.FORMANT_RATIOS, c.nc)
    _pointwise(f"stream {FC.stream_id(c)}", y, FC.stream_edge_reference(c), lambda r: pv_cases.bound(c.hop, r))


@pytest.mark.parametrize("c", FC.FORMANT_SCENARIOS, ids=pv_cases.scenario_id)
def test_formant_scenario_matches_numpy(c):
    """Curve, plain and formant calls in turn on one handle, with interval changes and resets that land in the middle of a round (one of
    them pending at a formant call), against NumPy; the held intervals afterwards are set_semitones' alone."""
    from vocoderproject_amd import PhaseVocoderStream
    x = pv_cases.scenario_input(c)
    ref, _, held = FC.scenario_reference(c)
    n = x.shape[0]
    ps = PhaseVocoderStream(n, c.N, hop=c.hop)
    for s, v in enumerate(c.semitones):
        ps.set_semitones(v, stream=s)
    d_in = _blocks(x, c.N)
    d_out = torch.full_like(d_in, float("nan"))
    d_tab, d_phi = _dev(pv_cases.ratio_of(FC.scenario_semitones(c)), np.float64), _dev(FC.SCENARIO_PHIS, np.float64)
    b = 0
    for i, k in enumerate(pv_cases.call_spans(c.n_blocks, c.calls)):
        for s, v in c.changes.get(i, []):
            ps.set_semitones(v, stream=s)
        for s in c.resets.get(i, []):
            ps.reset(s)
        kind = FC.scenario_kind(i)
        kw = {} if kind == "plain" else {"d_ratio": d_tab[b:b + k]}
        if kind == "formant":
            kw.update(d_formant=d_phi, lifter=FC.SCENARIO_NC)
        ps.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k, **kw)
        b += k
    torch.cuda.synchronize()
    got = [ps.semitones(s) for s in range(n)]
    ps.close()
    y = _rows(d_out)
    assert np.all(np.isfinite(y)) and np.all(y[:, :pv_cases.latency(c.N, c.hop)] == 0)
    _pointwise(f"scenario {pv_cases.scenario_id(c)}", y, ref, lambda r: pv_cases.bound(c.hop, r))
    assert got == held


def test_300_streams_through_the_streaming_kernel():
    """300 workgroups on 256 compute units: every stream bit-identical to the one-shot, streams 0, 1, 255, 256 and 299 against NumPy."""
    c = FC.BIG_STREAM
    x, ref = FC.big_stream_input(), FC.big_stream_reference()
    assert x.shape == (FC.BIG_S, c.N * c.n_blocks)
    _, y = _stream_is_the_one_shot("300 streams", x, c.N, c.hop, FC.big_stream_ratios(), FC.big_formants(), c.nc)
    chk = list(FC.BIG_CHECKED)
    _pointwise("big-stream", y[chk], np.stack([ref[s] for s in chk]), lambda r: pv_cases.bound(c.hop, r), streams=chk)
    assert np.abs(y).max() > 0.1


# ---- 6. degenerate inputs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", FC.HOPS)
@pytest.mark.parametrize("name", pv_cases.DEGENERATE)
def test_degenerate_inputs(name, hop):
    """Silence, DC, a Nyquist tone, two clicks and a square wave sit on wrap ties where no pointwise reference exists.  Along the "steps"
    table every sample is finite, silence gives exact zeros, the streaming kernel (blocks of 100 samples) gives the one-shot's bits and
    |y| <= 16 x 2 Mf (1 + 1e-6) -- pv_cases.magnitude_ceiling, the gain being at most 16.  With every stream's formant ratio equal to
    its constant pitch ratio the output is the parent curve call's, bit for bit: the only statement available on a wrap tie."""
    N, nb = FC.DEG_N, FC.DEG_BLOCKS
    x = np.stack([pv_cases.degenerate(name, N * nb)] * S)
    y1, y2 = _stream_is_the_one_shot(f"{name} hop {hop}", x, N, hop, pv_cases.ratio_of(FC.deg_semitones(hop)), FC.FORMANT_RATIOS, 32)
    r = pv_cases.ratio_of(np.array(pv_cases.SEMITONES))
    const = np.repeat(r[:, None], (N * nb - F) // hop + 1, axis=1)
    same, parent = _one_shot(x, hop, const, r, 32), _one_shot_curve(x, hop, const)
    _bits(same, parent, f"{name} hop {hop}: formant ratio = pitch ratio against the curve call")
    if name == "silence":
        assert np.all(y1 == 0) and np.all(y2 == 0) and np.all(same == 0)
    top = 16.0 * pv_cases.magnitude_ceiling(x[0], hop) * (1 + 1e-6)
    print(f"FORMANTDEG {name} hop {hop}: max |y| {np.abs(y1).max():.4f} ceiling {top:.4f}")
    assert np.abs(y1).max() <= top and np.abs(y2).max() <= top and np.abs(same).max() <= top / 16.0


# ---- 7. the cached formant table and stream order ---------------------------------------------------------------------------------------------------
def _busy():
    b = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    return b


FSEMI_1, FSEMI_2 = np.array([0.0, 3.0, -5.0, 12.0, -12.0]), np.array([-12.0, 12.0, 7.0, -3.0, 0.0])


def test_two_formant_tables_back_to_back_on_a_side_stream():
    """formant_semitones= uploads into ONE device table per handle.  Two calls with different formant intervals, issued on a side stream
    behind a matrix product without synchronising, each give the bits of a synchronised run: the second upload is ordered behind the
    first kernel."""
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios
    c = FC.FormantCase(256, 19, 3, "steps", 32)
    x, ratio = FC.case_input(c), FC.ratios_of(c)
    want1 = _one_shot(x, c.hop, ratio, semitones_to_ratios(FSEMI_1), c.nc)
    want2 = _one_shot(x, c.hop, ratio, semitones_to_ratios(FSEMI_2), c.nc)
    assert not any(np.array_equal(want1[s], want2[s]) for s in range(S))
    st = StftRoundTrip(S, FC.length(c), F, c.hop)
    d_in, d_ratio = _dev(x, np.float32), _dev(ratio, np.float64)
    o1, o2 = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    busy = _busy()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = busy @ busy * 1e-3
        st.pitch_shift_formant(d_in, o1, d_ratio=d_ratio, formant_semitones=FSEMI_1, lifter=c.nc)
        tab = st._formant_table
        st.pitch_shift_formant(d_in, o2, d_ratio=d_ratio, formant_semitones=FSEMI_2, lifter=c.nc)
    side.synchronize()
    assert st._formant_table is tab and tuple(tab.shape) == (S,)                                   # one table per handle
    st.close()
    _bits(o1.cpu().numpy(), want1, "first formant table")
    _bits(o2.cpu().numpy(), want2, "second formant table")


def test_two_streaming_formant_tables_back_to_back_on_a_side_stream():
    from vocoderproject_amd import PhaseVocoderStream
    N, hop, k = 256, 256, 8
    x = pv_cases.mixed_streams(N * 2 * k, seed=12)
    d_tab = _dev(pv_cases.ratio_of(np.random.default_rng([N, hop, 15]).uniform(-12.0, 12.0, (2 * k, S))), np.float64)
    d_in = _blocks(x, N)
    twin = PhaseVocoderStream(S, N, hop=hop)
    want = torch.full_like(d_in, float("nan"))
    for b, fs in ((0, FSEMI_1), (k, FSEMI_2)):
        twin.process_device(d_in[b:b + k], want[b:b + k], n_blocks=k, d_ratio=d_tab[b:b + k], formant_semitones=fs)
        torch.cuda.synchronize()
    twin.close()
    ps = PhaseVocoderStream(S, N, hop=hop)
    got = torch.full_like(d_in, float("nan"))
    busy = _busy()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = busy @ busy * 1e-3
        ps.process_device(d_in[:k], got[:k], n_blocks=k, d_ratio=d_tab[:k], formant_semitones=FSEMI_1)
        tab = ps._formant_table
        ps.process_device(d_in[k:], got[k:], n_blocks=k, d_ratio=d_tab[k:], formant_semitones=FSEMI_2)
    side.synchronize()
    assert ps._formant_table is tab and tuple(tab.shape) == (S,)
    ps.close()
    _bits(_rows(got), _rows(want), "two formant calls on a side stream")
    assert np.abs(_rows(want)[:, k * N:]).max() > 0.1
    # ... and the second table was in force: the same blocks under the first table are another signal
    again = PhaseVocoderStream(S, N, hop=hop)
    other = torch.full_like(d_in, float("nan"))
    again.process_device(d_in, other, n_blocks=2 * k, d_ratio=d_tab, formant_semitones=FSEMI_1)
    torch.cuda.synchronize()
    again.close()
    assert not np.array_equal(_rows(other)[:, k * N:], _rows(want)[:, k * N:])
