"""CPU-side checks of the ratio-curve pitch shift (vp_stft_pitch_shift_curve, vp_pv_process_blocks_curve_device): the reference of a
time-varying ratio is well conditioned on every case the GPU tests compare against it (the gate), a curve that is one frame off cannot
hide inside the bound (teeth), a constant curve is the fixed-interval definition, vp_semitones_to_ratios gives the library's bits, the
symbols and their argument checks, and the offline glide's plumbing.  The same gate and teeth hold for every list that
tests/test_gpu_pv_curve_edges.py compares pointwise: the one-shot edges, the streaming cases, the scenarios of curve and plain calls, and
the streams checked in the batch of 300.  The kernels are checked on the GPU (tests/test_gpu_pv_curve.py, tests/test_gpu_pv_curve_edges.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_curve_cases as CC  # noqa: E402
import stft_reference as R  # noqa: E402

SYMBOLS = ["vp_stft_pitch_shift_curve", "vp_semitones_to_ratios", "vp_pv_process_blocks_curve_device"]


@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    L = C.CDLL(build.build())
    L.vp_semitones_to_ratios.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    return L


def test_the_cases_are_the_ones_the_matrix_names():
    assert {(c.F, c.hop) for c in CC.CASES} == {(1024, h) for h in (64, 128, 256, 512)} | {(2048, h) for h in (128, 256, 512, 1024)}
    for c in CC.CASES:
        T, st = CC.length(c), CC.semitones_of(c)
        assert (T - c.F) // c.hop + 1 == c.nF and st.shape == (CC.N_STREAMS, c.nF) and np.abs(st).max() <= 12.0
        if c.nF == 19:
            assert T % 2 == 1 and T - (c.F + 18 * c.hop) == 3 and c.nF % 4 == 3      # odd, a tail, a last round of three frames
        else:
            assert c.nF == 4 and T == c.F + 3 * c.hop                                 # exactly one round
    glide = CC.semitones_of(CC.CurveCase(1024, 256, 19, "glide"))
    assert glide[0, 0] == -12.0 and glide[0, -1] == 12.0 and np.array_equal(glide[1], -glide[0])
    octv = CC.semitones_of(CC.CurveCase(1024, 256, 19, "octaves"))
    assert list(octv[3, :7]) == [-12.0] * 3 + [12.0] * 3 + [-12.0]


@pytest.mark.parametrize("c", CC.CASES, ids=CC.case_id)
def test_gate_and_teeth(c):
    """Gate: the two statements of the reference (radians / turns) agree on every stream of the case.  Teeth: with the curve rolled by
    one frame the reference moves by more than TEETH x the bound of the GPU comparison, on every stream that the roll changes at all."""
    ref, turns, rolled = CC.reference(c), CC.reference(c, "turns"), CC.reference(c, roll=1)
    ratio = CC.ratios_of(c)
    for s in range(CC.N_STREAMS):
        gate = np.abs(ref[s] - turns[s]).max()
        tol = CC.GATE_TOL * max(1.0, np.abs(ref[s]).max())
        bnd = CC.bound(c, ref[s])
        teeth = np.abs(ref[s] - rolled[s]).max()
        print(f"CURVE {CC.case_id(c)} stream {s}: gate {gate:.3g} (tol {tol:.3g})  rolled/bound {teeth / bnd:.3g}")
        assert gate <= tol, (s, gate)
        assert not np.array_equal(np.roll(ratio[s], 1), ratio[s])
        assert teeth > CC.TEETH * bnd, (s, teeth / bnd)


def _gate_and_teeth(tag, what, ref, turns, others, bound_of):
    """Per stream: the radians and turns forms agree to GATE_TOL max(1, max |ref|); every reference of `others` ({name: [S][T]}), the
    schedule off by one, is more than TEETH bounds away."""
    for s in range(ref.shape[0]):
        gate = np.abs(ref[s] - turns[s]).max()
        tol = CC.GATE_TOL * max(1.0, np.abs(ref[s]).max())
        bnd = bound_of(ref[s])
        teeth = {k: np.abs(ref[s] - o[s]).max() / bnd for k, o in others.items()}
        print(f"{tag} {what} stream {s}: gate {gate:.3g} (tol {tol:.3g})  " + "  ".join(f"{k}/bound {v:.3g}" for k, v in teeth.items()))
        assert gate <= tol, (s, gate)
        for k, v in teeth.items():
            assert v > CC.TEETH, (s, k, v)


def test_the_new_lists_are_the_ones_the_issue_names():
    assert {(c.F, c.hop) for c in CC.EDGE_CASES} == {(c.F, c.hop) for c in CC.CASES}
    for F in (1024, 2048):
        for hop in CC.HOPS[F]:
            cs = [c for c in CC.EDGE_CASES if (c.F, c.hop) == (F, hop)]
            assert sorted((c.nF, c.extra, c.curve) for c in cs) == sorted(
                [(1, hop - 1, "steps")] + [(nF, ex, cv) for nF, ex in ((2, 0), (5, hop - 1), (6, 2)) for cv in ("glide", "steps")])
    for c in CC.EDGE_CASES:
        T, st = CC.edge_length(c), CC.semitones_of(c)
        assert (T - c.F) // c.hop + 1 == c.nF and T - (c.F + (c.nF - 1) * c.hop) == c.extra < c.hop
        assert (c.nF - 1) % 4 + 1 in (1, 2)                                             # frames of the last round
        assert st.shape == (CC.N_STREAMS, c.nF) and np.abs(st).max() <= 12.0
    assert {(c.hop, c.N) for c in CC.STREAM_CURVE_CASES} == {(h, n) for h in (64, 128, 256, 512) for n in (17, 64, 100, 1000, 1024, 4096)}
    for c in CC.STREAM_CURVE_CASES:
        assert c.n_blocks == max(-(-10 * 1024 // c.N), 5) and CC.stream_curve_semitones(c).shape == (c.n_blocks, CC.N_STREAMS)
    assert [c.hop for c in CC.CURVE_SCENARIOS] == list(pv_cases.HOPS)
    for c in CC.CURVE_SCENARIOS:
        spans = pv_cases.call_spans(c.n_blocks, c.calls)
        assert (c.N, c.n_blocks, c.calls) == (100, 124, (1, 3, 16, 2)) and sorted(c.resets) == [4, 8, 13]
        assert not any(CC.scenario_is_plain(i) for i in c.resets)                     # every reset precedes a curve call
        assert 0 < sum(CC.scenario_is_plain(i) for i in range(len(spans))) < len(spans) // 4 + 1


@pytest.mark.parametrize("c", CC.EDGE_CASES, ids=CC.edge_id)
def test_gate_and_teeth_edges(c):
    """Last rounds of one and two frames, one- and two-frame signals, a tail of hop - 1 samples.  Teeth: the curve rolled by a frame; on
    one frame every stream with its neighbour stream's ratio."""
    ratio = CC.ratios_of(c)
    off = np.roll(ratio, 1, axis=1) if c.nF >= 2 else np.roll(ratio, -1, axis=0)
    assert all(not np.array_equal(off[s], ratio[s]) for s in range(CC.N_STREAMS))
    _gate_and_teeth("CURVE", CC.edge_id(c), CC.edge_reference(c), CC.edge_reference(c, "turns"), {"off": CC.edge_reference(c, off=True)},
                    lambda r: CC.bound(c, r))


@pytest.mark.parametrize("c", CC.STREAM_CURVE_CASES, ids=CC.stream_curve_id)
def test_gate_and_teeth_stream_curve(c):
    """The streaming curve cases.  Teeth: every block with the ratio of the block behind it, and of the block in front of it."""
    _gate_and_teeth("CURVESTREAM", CC.stream_curve_id(c), CC.stream_curve_reference(c), CC.stream_curve_reference(c, "turns"),
                    {"next": CC.stream_curve_reference(c, shift=1), "prev": CC.stream_curve_reference(c, shift=-1)},
                    lambda r: pv_cases.bound(c.hop, r))


@pytest.mark.parametrize("c", CC.CURVE_SCENARIOS, ids=pv_cases.scenario_id)
def test_gate_and_teeth_curve_scenarios_and_where_their_resets_land(c):
    ref, landed, held = CC.scenario_reference(c)
    hits = {i: (fr, m) for per_stream in landed for i, fr, m in per_stream}
    assert sorted(hits) == [4, 8, 13]
    assert hits[4][0] != 0 and hits[8][0] != 0, hits                                  # in the middle of a round, at every hop
    assert any(fr != 0 and m < pv_cases.F for fr, m in hits.values()), hits           # ... followed by a call shorter than a frame
    assert held == [-12.0, 5.0, 0.37, -4.0]                                           # the last change of every stream
    _gate_and_teeth("CURVESCENARIO", pv_cases.scenario_id(c), ref, CC.scenario_reference(c, "turns")[0],
                    {"next": CC.scenario_reference(c, shift=1)[0], "all-plain": CC.scenario_reference(c, all_plain=True)[0]},
                    lambda r: pv_cases.bound(c.hop, r))


@pytest.mark.parametrize("g", CC.BIG_LEGS, ids=CC.big_id)
def test_gate_and_teeth_of_the_streams_checked_in_the_large_batch(g):
    ref, turns, off = CC.big_reference(g), CC.big_reference(g, "turns"), CC.big_reference(g, off=True)
    O = g.F // g.hop
    assert sorted(ref) == sorted(CC.BIG_CHECKED) and (g.T % 2 == 1 or g.F == 2048 or g.kind == "stream")

    def rows(d):
        return np.stack([d[s] for s in CC.BIG_CHECKED])
    _gate_and_teeth("CURVEBIG", CC.big_id(g), rows(ref), rows(turns), {"off": rows(off)},
                    lambda r: 4.0 * O * 2.0 ** -24 * max(1.0, float(np.abs(r).max())))


@pytest.mark.parametrize("F,hop", [(1024, 64), (1024, 256), (1024, 512), (2048, 128), (2048, 512), (2048, 1024)])
def test_a_constant_curve_is_the_fixed_interval_definition(F, hop):
    T = F + 18 * hop + 3
    x = pv_cases.mixed_streams(T, seed=hop + 5)
    for s, v in enumerate(pv_cases.SEMITONES):
        r = pv_cases.ratio_of(v)
        assert np.array_equal(CC.frame_loop(x[s], F, hop, np.full(19, r)), R.stft_roundtrip(x[s], F, hop, ratio=r)), (s, v)


def test_semitones_to_ratios_gives_the_librarys_bits(lib):
    st = np.array(list(pv_cases.SEMITONES) + [12.0, -12.0, 0.0], np.float64)
    r = np.full(st.shape, -1.0)
    assert lib.vp_semitones_to_ratios(st.ctypes.data, r.ctypes.data, st.size) == 0
    assert np.array_equal(r, np.array([pv_cases.ratio_of(v) for v in st]))
    assert r[-3] == 2.0 and r[-2] == 0.5 and r[-1] == 1.0
    for bad in (12.5, -12.0000001, float("nan"), float("inf")):
        st2 = np.array([0.0, bad, 3.0])
        r2 = np.full(3, -1.0)
        assert lib.vp_semitones_to_ratios(st2.ctypes.data, r2.ctypes.data, 3) == -1
        assert np.all(r2 == -1.0)                                                     # nothing is written
    assert lib.vp_semitones_to_ratios(st.ctypes.data, r.ctypes.data, 0) == 0
    assert lib.vp_semitones_to_ratios(None, r.ctypes.data, 1) == -1 and lib.vp_semitones_to_ratios(st.ctypes.data, None, 1) == -1
    # the Python wrapper keeps the shape and raises on a bad entry
    from vocoderproject_amd import VpError, semitones_to_ratios
    tab = semitones_to_ratios([[7.0, -12.0], [0.37, 12.0]])
    assert tab.shape == (2, 2) and tab[0, 0] == pv_cases.ratio_of(7.0) and tab[1, 1] == 2.0
    with pytest.raises(VpError):
        semitones_to_ratios([0.0, 12.5])


def test_symbols_are_declared_and_exported_and_null_arguments_fail(lib):
    txt = open(os.path.join(ROOT, "include", "vp_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s + "(" in txt, s
    assert "processBlocksCurve" in open(os.path.join(ROOT, "include", "vp_amd.hpp")).read()
    assert lib.vp_abi_version() == 3
    one = C.c_void_p(8)                                                               # (a non-null pointer that is never followed)
    lib.vp_stft_pitch_shift_curve.argtypes = [C.c_void_p] * 5
    lib.vp_pv_process_blocks_curve_device.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
    assert lib.vp_stft_pitch_shift_curve(None, one, one, one, None) == -1
    assert lib.vp_pv_process_blocks_curve_device(None, one, one, one, 1, None) == -1


class _DelayCurveStream:
    """PhaseVocoderStream's latency and run(x, blocks_per_call, curve), the DSP replaced by the identity (run returns its input: what an
    aligned output of a pure delay is)."""

    def __init__(self, S, N, latency=768):
        self.S, self.N, self._lat, self.curve, self.bpc = S, N, latency, None, None

    @property
    def latency(self):
        return self._lat

    def run(self, x, blocks_per_call=8, curve=None):
        assert x.shape[0] == self.S and x.dtype == np.float32
        self.curve, self.bpc = np.array(curve), blocks_per_call
        return x.copy()


def test_offline_glide_builds_one_interval_per_block_and_recording():
    from vocoderproject_amd import offline
    v = [np.arange(1, 2501, dtype=np.float32) / 4096, np.linspace(-1, 1, 700).astype(np.float32), np.zeros(0, np.float32)]
    p = _DelayCurveStream(3, 256, latency=768)
    out = offline.pv_glide(v, -12.0, 12.0, N=256, processor=p)
    assert [o.shape for o in out] == [(2, 2500), (2, 700), (2, 0)]
    for o, x in zip(out, v):
        np.testing.assert_array_equal(o[0], x)
        np.testing.assert_array_equal(o[1], x)
    nb = -(-(2500 + 768) // 256)
    assert p.curve.shape == (nb, 3) and p.bpc == 16 and np.abs(p.curve).max() <= 12.0
    # recording 0 has 10 blocks: -12 at block 0, +12 at block 9 and behind it, linear between
    np.testing.assert_allclose(p.curve[:10, 0], np.linspace(-12.0, 12.0, 10), rtol=0, atol=1e-12)
    assert np.all(p.curve[9:, 0] == 12.0)
    # recording 1 has 3 blocks, the empty one a single value and then the end
    np.testing.assert_allclose(p.curve[:3, 1], [-12.0, 0.0, 12.0], rtol=0, atol=1e-12)
    assert np.all(p.curve[2:, 1] == 12.0) and p.curve[0, 2] == -12.0 and np.all(p.curve[1:, 2] == 12.0)
    with pytest.raises(ValueError):
        offline.pv_glide(v, -13.0, 0.0, N=256, processor=p)
    with pytest.raises(ValueError):
        offline.pv_glide([], 0.0, 1.0, N=256, processor=p)


def test_offline_command_line_takes_a_glide_or_a_shift(tmp_path, monkeypatch):
    from vocoderproject_amd import offline
    f = str(tmp_path / "a.wav")
    offline.write_wav(f, 44100, np.linspace(-0.5, 0.5, 1000))
    seen = {}

    def fake_glide(voices, start, end, **kw):
        seen["glide"] = (start, end, kw["N"], kw["hop"])
        return [np.stack([v, v]) for v in voices]

    def fake_shift(voices, shift, **kw):
        seen["shift"] = shift
        return [np.stack([v, v]) for v in voices]
    monkeypatch.setattr(offline, "pv_glide", fake_glide)
    monkeypatch.setattr(offline, "pv_shift", fake_shift)
    assert offline.main(["pvshift", f, "--glide", "-3:7.5", "--hop", "128", "--out-dir", str(tmp_path / "o")]) == 0
    assert seen == {"glide": (-3.0, 7.5, 1024, 128)} and os.path.exists(str(tmp_path / "o" / "a_pvshift.wav"))
    assert offline.main(["pvshift", f, "--shift", "7", "--out-dir", str(tmp_path / "o")]) == 0       # --shift keeps its path
    assert seen["shift"] == 7.0 and set(seen) == {"glide", "shift"}
    for bad in (["--glide", "3"], ["--glide", "a:b"], ["--glide", "1:2", "--shift", "3"], []):
        with pytest.raises(SystemExit):
            offline.main(["pvshift", f, "--out-dir", str(tmp_path / "o")] + bad)
