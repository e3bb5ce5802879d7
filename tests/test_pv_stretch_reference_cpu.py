"""CPU-side checks of the phase-vocoder time stretch (vp_stft_time_stretch): the reference of frames analysed at given positions is well
conditioned on every case the GPU test compares against it (the gate), a table that is one frame off or a stage that unwraps with hop
instead of the frame's advance cannot hide inside the bound (teeth), the table f hop is the fixed-grid definition, the clamps,
vp_stretch_positions against its formula, the symbols and their argument checks, and the offline stretch's plumbing; and on the edge
tables (both clamps of the advance and of the position) the same gate, with teeth for every plausible wrong clamp.  The kernels are
checked on the GPU (tests/test_gpu_pv_stretch.py, tests/test_gpu_pv_stretch_edges.py)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_stretch_cases as SC  # noqa: E402
import pv_stretch_reference as SR  # noqa: E402
import stft_reference as R  # noqa: E402

SYMBOLS = ["vp_stft_time_stretch", "vp_stretch_positions"]


@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    L = C.CDLL(build.build())
    L.vp_stretch_positions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]
    return L


def test_the_cases_are_the_ones_the_matrix_names():
    assert len(SC.CASES) == 96 and len(set(SC.CASES)) == 96
    assert {(c.F, c.hop) for c in SC.CASES} == {(1024, h) for h in (64, 128, 256, 512)} | {(2048, h) for h in (128, 256, 512, 1024)}
    semis = {c.semitones for c in SC.CASES}
    assert 12.0 in semis and -12.0 in semis and semis == {0.0} | set(pv_cases.SEMITONES)
    for F in (1024, 2048):
        for hop in SC.HOPS[F]:
            cs = [c for c in SC.CASES if (c.F, c.hop) == (F, hop)]
            assert sorted({(c.nF, c.extra) for c in cs}) == sorted([(19, 3), (4, 0), (1, hop - 1), (2, 0), (5, hop - 1), (6, 2)])
            for shape in {(c.nF, c.extra) for c in cs}:
                two = [c.semitones for c in cs if (c.nF, c.extra) == shape]
                assert len(two) == 2 and two[0] == 0.0 and two[1] != 0.0
    assert sorted({(c.nF - 1) % 4 + 1 for c in SC.CASES}) == [1, 2, 3, 4]                 # frames of the last round
    for c in SC.CASES:
        T, n_in, pos = SC.out_length(c), SC.in_length(c), SC.positions(c)
        assert (T - c.F) // c.hop + 1 == c.nF and pos.shape == (SC.N_STREAMS, c.nF) and pos.dtype == np.int32
        assert n_in >= c.F + pos.max() + 1 and pos.min() == 0 and np.all(pos[:, 0] == 0)
        if c.nF in (19, 5):
            assert n_in % 2 == 1
        if c.nF == 19:
            assert T % 2 == 1
        f = np.arange(c.nF)
        for s, a in enumerate((0.5, 0.8, 1.37, 4.0)):
            assert np.array_equal(pos[s], np.floor(f * c.hop / a))
        if c.nF >= 3:
            inc = np.diff(pos[4])
            assert inc[0] == 2 * c.hop and inc[-1] == round(c.hop / 4) and np.all(np.diff(inc) <= 0)
    inc = np.diff(SC.positions(SC.StretchCase(1024, 256, 19, 3, 0.0))[4])
    assert np.any(inc % 2 == 1) and np.any(inc % 2 == 0)                                  # odd and even advances


@pytest.mark.parametrize("c", SC.CASES, ids=SC.case_id)
def test_gate_and_teeth(c):
    """Gate: the two statements of the reference (radians / turns) agree on every stream of the case.  Teeth: with the table rolled by one
    frame (from three frames on), and with a stage that unwraps with hop instead of the frame's advance (from two frames on), the
    reference moves by more than TEETH x the bound of the GPU comparison."""
    ref, turns = SC.reference(c), SC.reference(c, "turns")
    roll = SC.reference(c, variant="roll") if c.nF >= 3 else None
    hopw = SC.reference(c, variant="hop") if c.nF >= 2 else None
    pos = SC.positions(c)
    for s in range(SC.N_STREAMS):
        gate = np.abs(ref[s] - turns[s]).max()
        tol = SC.GATE_TOL * max(1.0, np.abs(ref[s]).max())
        bnd = SC.bound(c, ref[s])
        msg = f"STRETCH {SC.case_id(c)} stream {s}: gate {gate:.3g} (tol {tol:.3g})"
        assert np.all(np.isfinite(ref[s])) and gate <= tol, (s, gate)
        if roll is not None:
            assert not np.array_equal(SC.rolled(pos[s]), pos[s])
            t = np.abs(ref[s] - roll[s]).max() / bnd
            msg += f"  rolled/bound {t:.3g}"
            assert t > SC.TEETH, (s, "rolled", t)
        if hopw is not None:
            q = SR.clamp_positions(pos[s], SC.in_length(c), c.F)
            assert np.any(SR.advances(q, c.hop, c.F)[1:] != c.hop)
            t = np.abs(ref[s] - hopw[s]).max() / bnd
            msg += f"  hop-unwrap/bound {t:.3g}"
            assert t > SC.TEETH, (s, "hop", t)
        print(msg)


def test_gate_and_teeth_of_the_streams_checked_in_the_large_batch():
    a = SC.big_stretch()
    assert a.shape == (SC.BIG_S,) and 0.25 <= a.min() < 0.5 and 3.5 < a.max() <= 4.0
    pos = SC.big_positions()
    assert pos.shape == (SC.BIG_S, SC.BIG_NF) and pos.max() <= SC.BIG_N_IN - SC.BIG_F and SC.BIG_T % 2 == 1 and SC.BIG_N_IN % 2 == 1
    ref, turns, roll, hopw = SC.big_reference(), SC.big_reference("turns"), SC.big_reference(variant="roll"), SC.big_reference(variant="hop")
    assert sorted(ref) == sorted(SC.BIG_CHECKED)
    for s in SC.BIG_CHECKED:
        m = max(1.0, np.abs(ref[s]).max())
        bnd = 4.0 * (SC.BIG_F // SC.BIG_HOP) * 2.0 ** -24 * m
        assert np.abs(ref[s] - turns[s]).max() <= SC.GATE_TOL * m, s
        assert np.abs(ref[s] - roll[s]).max() > SC.TEETH * bnd and np.abs(ref[s] - hopw[s]).max() > SC.TEETH * bnd, s


# ---- the edge tables: both clamps of the advance, both clamps of the position ------------------------------------------------------------
def test_the_edge_tables_reach_what_they_name():
    assert len(set(SC.EDGE_CASES)) == 48 and {(c.F, c.hop) for c in SC.EDGE_CASES} == {(F, h) for F in (1024, 2048) for h in SC.HOPS[F]}
    assert {(c.nF, c.extra) for c in SC.EDGE_CASES} == {(19, 3), (6, 2), (2, 0)} and {c.semitones for c in SC.EDGE_CASES} == {0.0, 7.0}
    for c in SC.EDGE_CASES:
        F, hop, nF = c.F, c.hop, c.nF
        n_in, pos, x = SC.edge_in_length(c), SC.edge_positions(c), SC.edge_input(c)
        qm = n_in - F
        assert pos.shape == (6, nF) and x.shape == (6, n_in) and x.dtype == np.float32 and np.array_equal(x[5], x[0])
        assert n_in % 4 == 3 and n_in - 4 < F + pos[3].max() + 1 <= n_in and {s * n_in % 4 for s in range(6)} == {0, 1, 2, 3}
        assert (SC.out_length(c) - F) // hop + 1 == nF and np.all(pos >= SC.INT_MIN) and np.all(pos <= SC.INT_MAX)
        q = [SR.clamp_positions(p, n_in, F) for p in pos]
        D = [SR.advances(v, hop, F) for v in q]
        raw = [np.diff(p) for p in pos]
        assert np.all(raw[0] == 0) and np.all(D[0][1:] == 1)                               # freeze
        assert np.all(raw[1] == -hop) and np.all(D[1][1:] == 1) and np.array_equal(q[1], pos[1])            # reverse
        assert np.array_equal(D[2][1:], ([1, 2, 3] * 6)[:nF - 1]) and np.array_equal(q[2], pos[2])          # crawl
        assert np.array_equal(raw[3], ([F, F + 1, F - 1, 2 * F + 3] * 5)[:nF - 1]) and np.array_equal(q[3], pos[3])       # leap
        assert np.array_equal(D[3][1:], ([F, F, F - 1, F] * 5)[:nF - 1])
        assert np.array_equal(q[4], ([0, qm, qm, 0, qm, 0, qm - 1, 1] * 3)[:nF]) and qm > F                  # ends
        assert np.array_equal(D[4][1:], ([F, 1, 1, F, 1, F, 1, 1, F, 1, 1, F, 1, F, 1, 1, F, 1])[:nF - 1])
        assert np.array_equal(q[5], pos[5]) and np.all(D[5][1:] == hop + 1)                 # skew
        assert nF < 6 or {int(v) % 4 for v in q[5]} == {0, 1, 2, 3}
    c = SC.StretchCase(1024, 256, 19, 3, 0.0)                                             # the mutants are what they say
    q = SR.clamp_positions(SC.edge_positions(c)[4], SC.edge_in_length(c), 1024)
    qm = SC.edge_in_length(c) - 1024
    assert list(SR.advances(q, 256, 1024, "nohigh")[1:4]) == [qm, 1, 1] and list(SR.advances(q, 256, 1024, "abs")[1:5]) == [1024, 1, 1024, 1024]
    assert list(SR.advances(q, 256, 1024, "lowhop")[1:4]) == [1024, 256, 256] and np.all(SR.advances(q, 256, 1024, "hop") == 256)


def _mutants_of(row, c):
    """The mutants that must show on a row of an edge case."""
    m = [] if (row == "freeze" and c.semitones == 0.0) else ["hop"]
    if (row == "leap" and c.nF >= 6) or row == "ends":
        m.append("nohigh")
    if row == "reverse" or (row == "ends" and c.nF >= 6):
        m += ["abs", "lowhop"]
    if row == "freeze" and c.semitones == 7.0:
        m.append("lowhop")
    if row == "ends":
        m.append("qmax-1")
    return m


@pytest.mark.parametrize("c", SC.EDGE_CASES, ids=SC.case_id)
def test_edge_gate_and_teeth(c):
    """On every stream of an edge case.  Gate: the two statements of the reference agree.  Teeth: each mutant of the advance or of the
    position's clamp moves the reference by more than TEETH x the bound of the GPU comparison on the rows that reach its clamp.  freeze at 0
    semitones: a repeated frame's deviation is -(k D) / F; at ratio 1 any D that divides hop gives whole turns per hop, so the pure stretch
    cannot see this clamp -- the definition and the "hop" mutant agree within the gate, which is asserted instead."""
    ref, turns = SC.edge_reference(c), SC.edge_reference(c, "turns")
    for s, row in enumerate(SC.EDGE_ROWS):
        m = max(1.0, np.abs(ref[s]).max())
        gate, bnd = np.abs(ref[s] - turns[s]).max(), SC.bound(c, ref[s])
        msg = f"STRETCHEDGE {SC.case_id(c)} {row}: gate {gate:.3g} (tol {SC.GATE_TOL * m:.3g})"
        assert np.all(np.isfinite(ref[s])) and np.abs(ref[s]).max() > 0.01 and gate <= SC.GATE_TOL * m, (row, gate)
        for mutant in _mutants_of(row, c):
            t = np.abs(ref[s] - SC.edge_reference(c, advance=mutant, rows=[s])[s]).max() / bnd
            msg += f"  {mutant}/bound {t:.3g}"
            assert t > SC.TEETH, (row, mutant, t)
        if row == "freeze" and c.semitones == 0.0:
            t = np.abs(ref[s] - SC.edge_reference(c, advance="hop", rows=[s])[s]).max()
            msg += f"  hop (unseen at ratio 1) {t:.3g}"
            assert t <= SC.GATE_TOL * m, (row, "hop", t)
        print(msg)


@pytest.mark.parametrize("cn", SC.SMALL_CASES, ids=SC.small_id)
def test_gate_of_the_smallest_inputs(cn):
    """n_in = F and F + 1: the edge tables collapse onto positions 0 and 0 / 1; the two statements of the reference agree there too."""
    c, n_in = cn
    q = SR.clamp_positions(SC.edge_positions(c, n_in), n_in, c.F)
    assert q.min() == 0 and q.max() == n_in - c.F and (n_in > c.F or np.all(q == 0))
    ref, turns = SC.edge_reference(c, n_in=n_in), SC.edge_reference(c, "turns", n_in=n_in)
    for s, row in enumerate(SC.EDGE_ROWS):
        m = max(1.0, np.abs(ref[s]).max())
        gate = np.abs(ref[s] - turns[s]).max()
        print(f"STRETCHEDGE {SC.small_id(cn)} {row}: gate {gate:.3g} (tol {SC.GATE_TOL * m:.3g})")
        assert np.all(np.isfinite(ref[s])) and np.abs(ref[s]).max() > 0.01 and gate <= SC.GATE_TOL * m, (row, gate)


@pytest.mark.parametrize("F,hop", [(1024, 256), (1024, 64), (2048, 512)])
def test_the_table_f_hop_is_the_fixed_grid_definition(F, hop):
    T = F + 18 * hop + 3
    x = pv_cases.mixed_streams(T, seed=hop + 5)
    pos = np.arange(19) * hop
    for s, v in enumerate(pv_cases.SEMITONES):
        r = pv_cases.ratio_of(v)
        ref = R.stft_roundtrip(x[s], F, hop, ratio=r)
        y = SR.stretch_roundtrip(x[s], pos, T, F, hop, r)
        err, tol = np.abs(y - ref).max(), SC.GATE_TOL * max(1.0, np.abs(ref).max())
        print(f"STRETCH identity F{F} hop{hop} {v:+g}st: {err:.3g} (tol {tol:.3g})")
        assert err <= tol, (s, v, err)


@pytest.mark.parametrize("F,hop", [(1024, 256), (2048, 512)])
def test_a_table_outside_the_input_is_the_table_clipped_by_hand(F, hop):
    nF, n_in = 9, F + 5 * hop + 1
    T = F + (nF - 1) * hop
    x = pv_cases.mixed_streams(n_in, seed=hop + 5)[0]
    dirty = np.array([-7, 3, -2 ** 31, 2 ** 31 - 1, 4 * hop, 2 * hop, n_in, n_in - F + 1, hop])     # negative, past the end, decreasing
    clean = np.clip(dirty, 0, n_in - F)
    assert not np.array_equal(dirty, clean) and np.any(np.diff(clean) < 0) and np.any(np.diff(clean) == 0)
    for form in ("radians", "turns"):
        yd, yc = SR.stretch_roundtrip(x, dirty, T, F, hop, 1.3, form), SR.stretch_roundtrip(x, clean, T, F, hop, 1.3, form)
        assert np.all(np.isfinite(yd)) and np.array_equal(yd, yc) and np.abs(yd).max() > 0
    D = SR.advances(clean, hop, F)
    assert D[0] == hop and D.min() == 1 and D.max() <= F                                 # a non-increasing step counts as 1


def test_stretch_positions_against_the_formula(lib):
    from vocoderproject_amd import VpError, stretch_positions
    for nF, hop, a, n_in, F in ((19, 256, 1.5, 9000, 1024), (19, 256, 0.25, 19457, 1024), (40, 64, 4.0, 1024, 1024), (7, 1024, 1.37, 5001, 2048),
                                (1, 512, 0.8, 2048, 2048), (0, 256, 1.0, 1024, 1024), (33, 128, 1.0, 6000, 1024)):
        want = np.array([min(math.floor(f * hop / a), n_in - F) for f in range(nF)], np.int64)
        pos = np.full(nF + 1, -77, np.int32)
        assert lib.vp_stretch_positions(pos.ctypes.data, nF, hop, a, n_in, F) == 0
        assert np.array_equal(pos[:nF], want) and pos[nF] == -77
        assert np.array_equal(stretch_positions(nF, hop, a, n_in, F), want) and np.array_equal(SR.stretch_positions(nF, hop, a, n_in, F), want)
    assert np.array_equal(stretch_positions(33, 128, 1.0, 6000), np.minimum(np.arange(33) * 128, 6000 - 1024))    # stretch 1: the grid
    pos = np.full(4, -77, np.int32)
    for bad in (0.2499, 4.0001, 0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert lib.vp_stretch_positions(pos.ctypes.data, 4, 256, bad, 4096, 1024) == -1
        with pytest.raises(VpError):
            stretch_positions(4, 256, bad, 4096, 1024)
    assert lib.vp_stretch_positions(None, 4, 256, 1.0, 4096, 1024) == -1
    assert lib.vp_stretch_positions(pos.ctypes.data, -1, 256, 1.0, 4096, 1024) == -1
    assert lib.vp_stretch_positions(pos.ctypes.data, 4, 0, 1.0, 4096, 1024) == -1
    assert lib.vp_stretch_positions(pos.ctypes.data, 4, 256, 1.0, 1023, 1024) == -1
    assert np.all(pos == -77)                                                             # nothing is written
    assert lib.vp_stretch_positions(pos.ctypes.data, 4, 256, 0.25, 4096, 1024) == 0 and lib.vp_stretch_positions(pos.ctypes.data, 4, 256, 4.0, 4096, 1024) == 0


def test_symbols_are_declared_and_exported_and_bad_arguments_fail_before_the_device(lib):
    txt = open(os.path.join(ROOT, "include", "vp_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s + "(" in txt, s
    assert lib.vp_abi_version() == 3 and "#define VP_ABI_VERSION 3 " in txt
    one = C.c_void_p(8)                                                                   # (a non-null pointer that is never followed)
    lib.vp_stft_time_stretch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    assert lib.vp_stft_time_stretch(None, one, 4096, one, one, 0.0, None) == -1
    import vocoderproject_amd
    assert vocoderproject_amd.stretch_positions is vocoderproject_amd.processor.stretch_positions
    assert hasattr(vocoderproject_amd.StftRoundTrip, "time_stretch")
    from vocoderproject_amd import build
    assert "vp_stft_stretch.inc" in build.DEPS


class _EchoStretch:
    """The offline flow's processor, the DSP replaced by a read of the input at the table's positions: output sample f hop + i (i < hop)
    of stream s is x[s][pos[s][f] + i]."""

    def __init__(self, hop):
        self.hop, self.seen = hop, None

    def run(self, x, pos, T, semitones):
        self.seen = (x.copy(), pos.copy(), T, semitones)
        y = np.zeros((x.shape[0], T), np.float32)
        for s in range(x.shape[0]):
            for f in range(pos.shape[1]):
                y[s, f * self.hop:(f + 1) * self.hop] = x[s, pos[s, f]:pos[s, f] + self.hop]
        return y


def test_offline_stretch_pads_builds_one_table_per_recording_and_trims():
    from vocoderproject_amd import offline
    v = [np.arange(1, 5001, dtype=np.float32) / 8192, np.linspace(-1, 1, 1700).astype(np.float32), np.zeros(300, np.float32)]
    p = _EchoStretch(256)
    out = offline.pv_stretch(v, [1.5, 0.5, 4.0], shift=3.0, processor=p)
    assert [o.shape for o in out] == [(2, 7500), (2, 850), (2, 1200)]
    x, pos, T, semis = p.seen
    assert x.shape == (3, 5000) and x.dtype == np.float32 and semis == 3.0
    assert np.array_equal(x[0], v[0]) and np.array_equal(x[1, :1700], v[1]) and np.all(x[1, 1700:] == 0)
    nF = (T - 1024) // 256 + 1
    assert T == 1024 + -(-7500 // 256) * 256 and pos.shape == (3, nF) and pos.dtype == np.int32
    f = np.arange(nF)
    assert np.array_equal(pos[0], np.minimum(np.floor(f * 256 / 1.5), 5000 - 1024))
    assert np.array_equal(pos[1], np.minimum(np.floor(f * 256 / 0.5), 1700 - 1024))        # held at the recording's own last frame
    assert np.all(pos[2] == 0)                                                            # shorter than a frame: its only frame
    for o in out:
        np.testing.assert_array_equal(o[0], o[1])
    np.testing.assert_array_equal(out[0][0][:256], v[0][:256])
    one = offline.pv_stretch(v[:1], 2.0, processor=p)
    assert one[0].shape == (2, 10000) and p.seen[3] == 0.0
    for bad in (dict(stretch=0.2), dict(stretch=4.5), dict(stretch=[1.0, 2.0]), dict(stretch=1.0, shift=13.0)):
        with pytest.raises(ValueError):
            offline.pv_stretch(v, processor=p, **bad)
    with pytest.raises(ValueError):
        offline.pv_stretch([], 1.0, processor=p)


def test_offline_command_line_takes_a_stretch(tmp_path, monkeypatch):
    from vocoderproject_amd import offline
    f, g = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    offline.write_wav(f, 44100, np.linspace(-0.5, 0.5, 1000))
    offline.write_wav(g, 44100, np.linspace(-0.5, 0.5, 400))
    seen = {}

    def fake(voices, stretch, **kw):
        seen.update(n=[len(v) for v in voices], stretch=stretch, kw=kw)
        return [np.stack([v, v]) for v in voices]
    monkeypatch.setattr(offline, "pv_stretch", fake)
    assert offline.main(["stretch", f, g, "--stretch", "1.5", "--shift", "3", "--hop", "128", "--out-dir", str(tmp_path / "o")]) == 0
    assert seen["n"] == [1000, 400] and seen["stretch"] == 1.5 and seen["kw"] == dict(shift=3.0, F=1024, hop=128, device=0)
    assert os.path.exists(str(tmp_path / "o" / "a_stretch.wav")) and os.path.exists(str(tmp_path / "o" / "b_stretch.wav"))
    assert offline.main(["stretch", f, "--stretch", "0.5", "--frame", "2048", "--out-dir", str(tmp_path / "o")]) == 0
    assert seen["kw"] == dict(shift=0.0, F=2048, hop=256, device=0)
    with pytest.raises(SystemExit):
        offline.main(["stretch", f, "--out-dir", str(tmp_path / "o")])
