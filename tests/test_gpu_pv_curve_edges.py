"""The three ratio-curve kernels (vp_k_stft_pv_curve, vp_k_stft_pv2k_curve, vp_k_pv_stream_curve of csrc/vp_stft_curve.inc) at the edges
their parents are tested at (tests/test_gpu_pv_matrix.py, tests/test_gpu_pv2k.py, tests/test_gpu_pv_stream.py).  The kernels are written-out
copies of the fixed-interval ones; only tests keep them equal.  Here: last rounds of one and two frames and one- and two-frame signals
against NumPy, the streaming kernel against NumPy at every hop and block size and through a schedule of curve calls, plain calls, interval
changes and resets, a constant curve against the parent's bits on the parents' whole matrices, 300 streams, a curve call behind more
pending changes than a call carries, degenerate inputs, power-of-two homogeneity, and the cached ratio table's order on a side stream.
The cases and references come from tests/pv_curve_cases.py, whose conditioning tests/test_pv_curve_reference_cpu.py gates; every pointwise
comparison is held at EVERY sample to  |y - ref| <= 4 O 2^-24 max(1, max |ref|),  O = F / hop.  Output buffers start as NaN."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv2k_cases  # noqa: E402
import pv_cases  # noqa: E402
import pv_curve_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

CALLS = CC.STREAM_CURVE_CALLS
KINDS = [("one-shot", F, hop) for F in (1024, 2048) for hop in CC.HOPS[F]] + [("stream", 1024, 64), ("stream", 1024, 512)]


def _kind_id(k):
    return f"{k[0]}-F{k[1]}-hop{k[2]}"


# ---- running the entry points -----------------------------------------------------------------------------------------------------------------
def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _one_shot_curve(x, F, hop, semitones=None, ratio=None):
    """vp_stft_pitch_shift_curve on x [S][T] with a table of intervals or of ratios [S][nF], on a handle of its own."""
    from vocoderproject_amd import StftRoundTrip
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    st.pitch_shift_curve(d_in, d_out, semitones=semitones, d_ratio=None if ratio is None else _dev(ratio, np.float64))
    torch.cuda.synchronize()
    st.close()
    y = d_out.cpu().numpy()
    assert np.all(np.isfinite(y)), f"{int((~np.isfinite(y)).sum())} samples unwritten or not finite"
    return y


def _one_shot_plain(x, F, hop, semis):
    """vp_stft_pitch_shift, one batch call per distinct interval of semis [S]."""
    from vocoderproject_amd import StftRoundTrip
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    d_in = _dev(x, np.float32)
    y = np.full(x.shape, np.nan, np.float32)
    for v in sorted(set(semis)):
        d_out = torch.full_like(d_in, float("nan"))
        st.pitch_shift(d_in, d_out, float(v))
        torch.cuda.synchronize()
        o = d_out.cpu().numpy()
        for s in range(x.shape[0]):
            if semis[s] == v:
                y[s] = o[s]
    st.close()
    assert np.all(np.isfinite(y))
    return y


def _blocks(x, N):
    S, T = x.shape
    return _dev(x.reshape(S, T // N, N).transpose(1, 0, 2), np.float32)


def _rows(d):
    nb, S, N = d.shape
    return d.cpu().numpy().transpose(1, 0, 2).reshape(S, nb * N)


def _stream(ps, x, calls, semis=None, how=None, before_call=None):
    """x [S][T] (whole blocks) through ps.process_device in calls of calls[i % len] blocks, no synchronisation between them.  how(i):
    "semitones" (semitones_per_block = the call's rows of semis [n_blocks][S]), "ratio" (d_ratio = their ratios) or "plain"; default:
    the two curve forms alternating.  before_call(i) runs in front of call i."""
    from vocoderproject_amd import semitones_to_ratios
    d_in = _blocks(x, ps.N)
    d_out = torch.full_like(d_in, float("nan"))
    b = 0
    for i, k in enumerate(pv_cases.call_spans(d_in.shape[0], calls)):
        if before_call:
            before_call(i)
        h = how(i) if how else ("semitones", "ratio")[i & 1]
        if h == "plain":
            ps.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k)
        elif h == "semitones":
            ps.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k, semitones_per_block=semis[b:b + k])
        else:
            ps.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k, d_ratio=_dev(semitones_to_ratios(semis[b:b + k]), np.float64))
        b += k
    torch.cuda.synchronize()
    y = _rows(d_out)
    assert np.all(np.isfinite(y)), f"{int((~np.isfinite(y)).sum())} samples unwritten or not finite"
    return y


def _pointwise(tag, what, y, ref, O):
    """Every stream at every sample within 4 O 2^-24 max(1, max |ref|); one line per stream for profiles/pv_curve_errors.txt."""
    assert y.shape == ref.shape and y.dtype == np.float32
    bad = []
    for s in range(y.shape[0]):
        e = np.abs(y[s].astype(np.float64) - ref[s])
        bnd = 4.0 * O * 2.0 ** -24 * max(1.0, float(np.abs(ref[s]).max()))
        print(f"{tag} {what} stream {s}: err {e.max():.3g} bound {bnd:.3g} rms {np.sqrt((e ** 2).mean()):.3g}")
        if e.max() > bnd:
            bad.append((s, float(e.max()), bnd, int(np.argmax(e))))
    assert not bad, (what, bad)


def _bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), what
    if not np.array_equal(a, b):
        d = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(d)} samples differ, first at {d[0]}, max {np.abs(a.astype(np.float64) - b).max():.3g}")


# ---- 1. one-shot edges against NumPy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CC.EDGE_CASES, ids=CC.edge_id)
def test_one_shot_edges_match_numpy(c):
    x, ref = CC.edge_input(c), CC.edge_reference(c)
    T = CC.edge_length(c)
    assert (T - c.F) // c.hop + 1 == c.nF
    y = _one_shot_curve(x, c.F, c.hop, semitones=CC.semitones_of(c))
    _pointwise("CURVE", CC.edge_id(c), y, ref, c.F // c.hop)
    covered = (c.nF - 1) * c.hop + c.F
    assert np.all(y[:, covered:] == 0) and y[:, covered:].shape[1] == c.extra                      # samples no frame covers
    assert np.sqrt((ref ** 2).mean()) > 0.01


# ---- 2. streaming against NumPy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CC.STREAM_CURVE_CASES, ids=CC.stream_curve_id)
def test_streaming_curve_matches_numpy_at_every_hop_and_block_size(c):
    from vocoderproject_amd import PhaseVocoderStream
    x, ref = CC.stream_curve_input(c), CC.stream_curve_reference(c)
    ps = PhaseVocoderStream(CC.N_STREAMS, c.N, hop=c.hop)
    L = ps.latency
    y = _stream(ps, x, CALLS, CC.stream_curve_semitones(c))
    ps.close()
    assert L == pv_cases.latency(c.N, c.hop) and np.all(y[:, :L] == 0)
    _pointwise("CURVESTREAM", CC.stream_curve_id(c), y, ref, pv_cases.F // c.hop)
    assert np.sqrt((ref ** 2).mean()) > 0.01


# ---- 3. curve calls, plain calls, interval changes and resets against NumPy -------------------------------------------------------------------
@pytest.mark.parametrize("c", CC.CURVE_SCENARIOS, ids=pv_cases.scenario_id)
def test_curve_scenario_matches_numpy(c):
    from vocoderproject_amd import PhaseVocoderStream
    x = pv_cases.scenario_input(c)
    ref, landed, held = CC.scenario_reference(c)
    ps = PhaseVocoderStream(x.shape[0], c.N, hop=c.hop)
    for s, v in enumerate(c.semitones):
        ps.set_semitones(v, stream=s)

    def before_call(i):
        for s, v in c.changes.get(i, []):
            ps.set_semitones(v, stream=s)
        for s in c.resets.get(i, []):
            ps.reset(s)

    y = _stream(ps, x, c.calls, CC.scenario_semitones(c),
                how=lambda i: "plain" if CC.scenario_is_plain(i) else ("semitones", "ratio")[i & 1], before_call=before_call)
    got = [ps.semitones(s) for s in range(x.shape[0])]
    ps.close()
    assert np.all(y[:, :pv_cases.latency(c.N, c.hop)] == 0)
    _pointwise("CURVESCENARIO", pv_cases.scenario_id(c), y, ref, pv_cases.F // c.hop)
    assert got == held                                                                             # curve calls leave the held interval


# ---- 4. a constant curve is the parent, bit for bit, on the parents' whole matrices -----------------------------------------------------------
def _constant_is_the_parent(F, case):
    from vocoderproject_amd import semitones_to_ratios
    x = pv_cases.one_shot_input(case)
    nF = (case.T - F) // case.hop + 1
    ratio = np.full((x.shape[0], nF), semitones_to_ratios([case.semitones])[0])
    _bits(_one_shot_curve(x, F, case.hop, ratio=ratio), _one_shot_plain(x, F, case.hop, [case.semitones] * x.shape[0]),
          f"F {F} {pv_cases.one_shot_id(case)} ({case.what})")


@pytest.mark.parametrize("case", pv_cases.ONE_SHOT_CASES, ids=pv_cases.one_shot_id)
def test_constant_curve_is_the_parent_bit_for_bit_1024(case):
    _constant_is_the_parent(1024, case)


@pytest.mark.parametrize("case", pv2k_cases.ONE_SHOT_CASES, ids=pv2k_cases.one_shot_id)
def test_constant_curve_is_the_parent_bit_for_bit_2048(case):
    _constant_is_the_parent(2048, case)


@pytest.mark.parametrize("case", pv_cases.STREAM_CASES, ids=pv_cases.stream_id)
def test_constant_streaming_curve_is_the_parent_bit_for_bit(case):
    from vocoderproject_amd import PhaseVocoderStream
    x = pv_cases.stream_input(case)
    S = x.shape[0]
    a = PhaseVocoderStream(S, case.N, hop=case.hop)                                                # rows that repeat every stream's interval
    ya = _stream(a, x, case.calls, np.tile(np.array(case.semitones), (case.n_blocks, 1)))
    a.close()
    b = PhaseVocoderStream(S, case.N, hop=case.hop)                                                # the twin: set_semitones and plain calls
    for s, v in enumerate(case.semitones):
        b.set_semitones(v, stream=s)
    yb = _stream(b, x, case.calls, how=lambda i: "plain")
    b.close()
    _bits(ya, yb, f"stream {pv_cases.stream_id(case)}")
    assert np.abs(yb).max() > 0.1


# ---- 5. more workgroups than compute units ------------------------------------------------------------------------------------------------------
BIG_ROWS = (slice(0, 5), slice(254, 259), slice(295, 300))


@pytest.mark.parametrize("g", CC.BIG_LEGS, ids=CC.big_id)
def test_300_streams_every_one_its_own_curve(g):
    """300 workgroups on 256 compute units: streams 0, 1, 255, 256 and 299 against NumPy, and the first, the middle (across workgroup 256)
    and the last five rows bit-identical to the same rows and curves run as batches of five on handles of their own."""
    from vocoderproject_amd import PhaseVocoderStream
    x, semis, ref = CC.big_input(g), CC.big_semitones(g), CC.big_reference(g)
    assert x.shape == (CC.BIG_S, g.T)
    if g.kind == "stream":
        def run(rows):
            ps = PhaseVocoderStream(x[rows].shape[0], g.N, hop=g.hop)
            y = _stream(ps, np.ascontiguousarray(x[rows]), CALLS, np.ascontiguousarray(semis[rows].T))
            ps.close()
            return y
    else:
        def run(rows):
            return _one_shot_curve(np.ascontiguousarray(x[rows]), g.F, g.hop, semitones=semis[rows])
    y = run(slice(None))
    chk = list(CC.BIG_CHECKED)
    _pointwise("CURVEBIG", CC.big_id(g), y[chk], np.stack([ref[s] for s in chk]), g.F // g.hop)
    for rows in BIG_ROWS:
        _bits(y[rows], run(rows), f"{CC.big_id(g)} rows {rows.start}..{rows.stop - 1}")
    assert np.abs(y).max() > 0.1


# ---- 6. a curve call behind more pending changes than a call carries ----------------------------------------------------------------------------
def test_curve_call_behind_many_pending_changes():
    """40 interval changes and 40 resets are pending at a curve call (a call carries 16: the rest go in update launches of the PLAIN
    kernel in front of it).  Same bits as a reset of all streams, the same curve call, and the 40 changes set behind it."""
    from vocoderproject_amd import PhaseVocoderStream
    S, N, hop, k = 40, 256, 256, 4
    x = pv_cases.harmonic_streams(S, N * 3 * k, seed=2)
    v = [float((s % 25) - 12) for s in range(S)]
    semis = np.random.default_rng([N, hop, 8]).uniform(-12.0, 12.0, (k, S))

    def curve_then_plain(i):
        return "semitones" if i == 0 else "plain"

    def run(order):
        ps = PhaseVocoderStream(S, N, hop=hop)
        ps.set_semitones(0.0)
        _stream(ps, x[:, :k * N], (k,), how=lambda i: "plain")

        def before_call(i):
            if order == "a" and i == 0:
                for s in range(S):
                    ps.set_semitones(v[s], stream=s)
                    ps.reset(s)
            if order != "a" and i == 0:
                ps.reset(-1)
            if order == "b" and i == 1:
                for s in range(S):
                    ps.set_semitones(v[s], stream=s)
        y = _stream(ps, x[:, k * N:], (k,), semis, how=curve_then_plain, before_call=before_call)
        ps.close()
        return y
    ya, yb, y0 = run("a"), run("b"), run("zero")
    _bits(ya, yb, "changes in front of the curve call against changes behind it")
    _bits(ya[:, :k * N], y0[:, :k * N], "the curve call does not use the held interval")
    assert sum(not np.array_equal(ya[s, k * N:], y0[s, k * N:]) for s in range(S)) == sum(1 for s in range(S) if v[s] != 0.0)
    assert np.abs(ya[:, k * N:]).max() > 0.1


# ---- 7. degenerate inputs -----------------------------------------------------------------------------------------------------------------------
DEG_SEMIS = (7.0, -12.0, 0.37, 12.0)


@pytest.mark.parametrize("kind", KINDS, ids=_kind_id)
@pytest.mark.parametrize("name", pv_cases.DEGENERATE)
def test_degenerate_inputs_along_a_curve(name, kind):
    """Silence, DC, a Nyquist tone, two clicks and a square wave sit on wrap ties where no pointwise reference exists.  A constant curve
    gives the parent's bits; along the "steps" curve every sample is finite, silence gives exact zeros and |y| <= 2 Mf (1 + 1e-6) (a
    frame's inverse transform is bounded by its magnitude sum whatever the ratios are: pv_cases.magnitude_ceiling)."""
    from vocoderproject_amd import PhaseVocoderStream
    what, F, hop = kind
    S, N = len(DEG_SEMIS), 100
    T = N * 42 if what == "stream" else 4 * F + hop + 3
    x = np.stack([pv_cases.degenerate(name, T)] * S)
    if what == "stream":
        nb = T // N
        a = PhaseVocoderStream(S, N, hop=hop)
        const = _stream(a, x, CALLS, np.tile(np.array(DEG_SEMIS), (nb, 1)))
        a.reset(-1)
        for s, v in enumerate(DEG_SEMIS):
            a.set_semitones(v, stream=s)
        parent = _stream(a, x, CALLS, how=lambda i: "plain")
        a.reset(-1)
        y = _stream(a, x, CALLS, np.stack([CC.steps(hop, s, nb) for s in range(S)]).T)
        a.close()
    else:
        nF = (T - F) // hop + 1
        const = _one_shot_curve(x, F, hop, semitones=np.repeat(np.array(DEG_SEMIS)[:, None], nF, axis=1))
        parent = _one_shot_plain(x, F, hop, DEG_SEMIS)
        y = _one_shot_curve(x, F, hop, semitones=np.stack([CC.steps(hop, s, nF) for s in range(S)]))
    _bits(const, parent, f"{name} {_kind_id(kind)}: constant curve against the parent")
    if name == "silence":
        assert np.all(y == 0) and np.all(const == 0)
    top = (pv_cases if F == 1024 else pv2k_cases).magnitude_ceiling(x[0], hop) * (1 + 1e-6)
    print(f"CURVEDEG {name} {_kind_id(kind)}: max |y| {np.abs(y).max():.4f} ceiling {top:.4f}")
    assert np.abs(y).max() <= top and np.abs(const).max() <= top


# ---- 8. power-of-two homogeneity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,hop", [(F, hop) for F in (1024, 2048) for hop in CC.HOPS[F]], ids=lambda v: str(v))
def test_power_of_two_homogeneity_along_a_curve(F, hop):
    """The output for x 2^e is the output for x times 2^e, bit for bit, along the "steps" curve: the one-shot kernel of F at this hop,
    and at 1024 points the streaming kernel (reset between the runs)."""
    from vocoderproject_amd import PhaseVocoderStream
    N, S = 256, CC.N_STREAMS
    x = pv_cases.mixed_streams(N * 28 + 1 + (F if F == 2048 else 0), seed=hop)                     # odd T for the one-shot
    nF = (x.shape[1] - F) // hop + 1
    semis = np.stack([CC.steps(hop, s, nF) for s in range(S)])
    y0 = _one_shot_curve(x, F, hop, semitones=semis)
    assert np.abs(y0).max() > 0.1
    ps = s0 = None
    if F == 1024:
        per_block = np.stack([CC.steps(hop, s, 28) for s in range(S)]).T
        ps = PhaseVocoderStream(S, N, hop=hop)
        s0 = _stream(ps, x[:, :-1], CALLS, per_block)
        assert np.abs(s0).max() > 0.1
    for e in (-40, 12):
        c = np.float32(2.0 ** e)
        _bits(_one_shot_curve(x * c, F, hop, semitones=semis), y0 * c, f"F {F} hop {hop}: one-shot, x 2^{e}")
        if ps is not None:
            ps.reset(-1)
            _bits(_stream(ps, x[:, :-1] * c, CALLS, per_block), s0 * c, f"hop {hop}: stream, x 2^{e}")
    if ps is not None:
        ps.close()


# ---- 9. the cached ratio table and stream order ---------------------------------------------------------------------------------------------------
def _busy():
    b = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize("F", [1024, 2048])
def test_two_curves_of_one_shape_back_to_back_on_a_side_stream(F):
    """semitones= uploads into one device table per handle and shape.  Two calls of the same shape and different curves, issued on a side
    stream behind a matrix product without synchronising, each give the bits of a synchronised run of their curve: the second upload
    is ordered behind the first kernel."""
    from vocoderproject_amd import StftRoundTrip
    c = CC.CurveCase(F, 256, 19, "steps")
    x = CC.case_input(c)
    s1 = CC.semitones_of(c)
    s2 = np.ascontiguousarray(s1[::-1, ::-1])
    want1, want2 = _one_shot_curve(x, F, c.hop, semitones=s1), _one_shot_curve(x, F, c.hop, semitones=s2)
    assert not np.array_equal(want1, want2)
    st = StftRoundTrip(CC.N_STREAMS, CC.length(c), F, c.hop)
    d_in = _dev(x, np.float32)
    o1, o2 = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    busy = _busy()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = busy @ busy * 1e-3
        st.pitch_shift_curve(d_in, o1, semitones=s1)
        st.pitch_shift_curve(d_in, o2, semitones=s2)
    side.synchronize()
    assert len(st._curve_tables) == 1
    st.close()
    _bits(o1.cpu().numpy(), want1, f"F {F}: first curve")
    _bits(o2.cpu().numpy(), want2, f"F {F}: second curve")


def test_two_streaming_curve_calls_back_to_back_on_a_side_stream():
    from vocoderproject_amd import PhaseVocoderStream
    S, N, hop, k = CC.N_STREAMS, 256, 256, 8
    x = pv_cases.mixed_streams(N * 2 * k, seed=11)
    semis = np.random.default_rng([N, hop, 10]).uniform(-12.0, 12.0, (2 * k, S))
    twin = PhaseVocoderStream(S, N, hop=hop)
    d_in = _blocks(x, N)
    want = torch.full_like(d_in, float("nan"))
    for b in (0, k):
        twin.process_device(d_in[b:b + k], want[b:b + k], n_blocks=k, semitones_per_block=semis[b:b + k])
        torch.cuda.synchronize()
    twin.close()
    ps = PhaseVocoderStream(S, N, hop=hop)
    got = torch.full_like(d_in, float("nan"))
    busy = _busy()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = busy @ busy * 1e-3
        ps.process_device(d_in[:k], got[:k], n_blocks=k, semitones_per_block=semis[:k])
        ps.process_device(d_in[k:], got[k:], n_blocks=k, semitones_per_block=semis[k:])
    side.synchronize()
    assert len(ps._curve_tables) == 1
    ps.close()
    _bits(_rows(got), _rows(want), "two curve calls on a side stream")
    assert np.abs(_rows(want)[:, k * N:]).max() > 0.1
