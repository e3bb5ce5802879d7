"""CPU-side checks of the formant definition (tests/pv_formant_reference.py) on the EDGE cases of tests/pv_formant_cases.py, which
tests/test_gpu_pv_formant_edges.py compares pointwise: the gate of every case (the radians and the turns form agree), the share of (frame,
bin) pairs at each side of the gain's clamp where a case is there for the clamp, and the teeth -- every named wrong kernel of
pv_formant_reference.WRONG is more than TEETH x the GPU test's bound from the definition on the cases meant to exclude it.  One line per
case and stream is printed (-s)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_curve_cases as CC  # noqa: E402
import pv_formant_cases as FC  # noqa: E402
import pv_formant_reference as FR  # noqa: E402

S = FC.N_STREAMS


def _away(ref, other, bnd):
    return float(np.abs(other - ref).max()) / bnd


def test_the_variants_default_to_the_definition_and_the_lists_are_the_ones_named():
    assert len(FR.WRONG) == 11 and abs(FR.clamp_limits("clamp-db")[1] - 2.763) < 1e-3 and FR.clamp_limits() == (-FR.LN16, FR.LN16)
    assert FR.clamp_limits("clamp-nolow") == (-np.inf, FR.LN16) and FR.clamp_limits("clamp-nohigh") == (-FR.LN16, np.inf)
    c = FC.FormantCase(256, 4, 0, "glide", 32)
    x, ratio = FC.case_input(c), FC.ratios_of(c)
    assert np.array_equal(FR.frame_loop(x[3], FC.F, c.hop, ratio[3], 2.0, c.nc, wrong=None), FC.reference(c)[3])
    assert {(c.hop, c.curve, c.nc) for c in FC.CLAMP_CASES} == {(h, cv, nc) for h in (64, 512) for cv in ("glide", "steps") for nc in (32, 64)}
    assert {(c.hop, c.semitones, c.nc) for c in FC.TOP_CASES} == {(h, st, nc) for h in (64, 512) for st in (0.0, -7.0) for nc in (32, 64)}
    assert {(c.hop, c.e) for c in FC.LEVEL_CASES} == {(h, e) for h in FC.HOPS for e in (-16, -20, -24, 15)}
    for c in FC.CLAMP_CASES + FC.TOP_CASES + FC.LEVEL_CASES + [FC.LIFTER_CASE]:
        assert (c.nF, c.extra) == (6, 3) and (FC.length(c) - FC.F) // c.hop + 1 == 6
    assert list(FC.CLAMP_PHIS) == [2.0, 0.5, 2.0 ** (-5.0 / 12.0), 2.0, 0.5] and FC.ALL_LIFTERS == tuple(range(4, 65))
    assert [(c.hop, c.N) for c in FC.STREAM_EDGE_CASES] == [(64, 17), (64, 4096), (512, 17), (512, 4096), (256, 1000), (128, 64)]
    assert (FC.BIG_STREAM.N, FC.BIG_STREAM.hop, FC.BIG_STREAM.n_blocks) == (256, 256, 24)
    # the signals: a 60 dB step down at frame bin 128, and everything below frame bin 496 at -40 dB
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FC.F) / FC.F))
    m = np.abs(np.fft.rfft(FC.step_noise(4099, 7)[:FC.F] * w))
    assert 50.0 < 20.0 * np.log10(np.sqrt((m[8:120] ** 2).mean() / (m[136:500] ** 2).mean())) < 70.0
    m = np.abs(np.fft.rfft(FC.bright_noise(4099, 7)[:FC.F] * w))
    assert 30.0 < 20.0 * np.log10(np.sqrt((m[500:512] ** 2).mean() / (m[8:488] ** 2).mean())) < 50.0


# ---- 1. the clamp ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.CLAMP_CASES, ids=FC.case_id)
def test_clamp_cases_gate_share_and_teeth(c):
    """CLAMP_SHARE_CAP does not apply here: the cases are there for the clamp.  At least CLAMP_MIN_SHARE of the (frame, bin) pairs of the
    streams with phi = 2 reach the + clamp, of those with phi = 1/2 the - clamp; the clamp at ln 8 is more than TEETH bounds away on all four,
    a missing lower clamp on the phi = 1/2 streams, a missing upper one on the phi = 2 streams; the clamp written from "24 dB" (2.763 for
    2.7726) more than 2 bounds on all four, which is what a pass within one bound needs to exclude it."""
    ref, turns = FC.clamp_reference(c), FC.clamp_reference(c, "turns")
    wrong = {w: FC.clamp_reference(c, wrong=w) for w in ("clamp-ln8", "clamp-db", "clamp-nolow", "clamp-nohigh")}
    stats = FC.clamp_stats(c)
    for s in range(S):
        gate = np.abs(ref[s] - turns[s]).max() / max(1.0, np.abs(ref[s]).max())
        bnd = FC.bound(c, ref[s])
        hi, lo = stats[s]["clamped_hi"] / stats[s]["pairs"], stats[s]["clamped_lo"] / stats[s]["pairs"]
        away = {w: _away(ref[s], r[s], bnd) for w, r in wrong.items()}
        print(f"FORMANTEDGE GATE clamp {FC.case_id(c)} stream {s}: forms {gate:.3g} share +{hi:.3f} -{lo:.3f} max {np.abs(ref[s]).max():.3f}  "
              + "  ".join(f"{w} {v:.3g}" for w, v in away.items()))
        assert gate <= FC.GATE_TOL, (s, gate)
        assert stats[s]["pairs"] == c.nF * (FC.F // 2 + 1)
        if s in FC.CLAMP_HIGH:
            assert hi >= FC.CLAMP_MIN_SHARE, (s, hi)
            assert away["clamp-nohigh"] > FC.TEETH, (s, away)
        if s in FC.CLAMP_LOW:
            assert lo >= FC.CLAMP_MIN_SHARE, (s, lo)
            assert away["clamp-nolow"] > FC.TEETH, (s, away)
        if s in FC.CLAMP_HIGH + FC.CLAMP_LOW:
            assert away["clamp-ln8"] > FC.TEETH, (s, away)
            assert away["clamp-db"] > 2.0, (s, away)


# ---- 2. the top of the interpolation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.TOP_CASES, ids=FC.top_id)
def test_top_cases_gate_and_teeth(c):
    """The clamp share is near one half here (the envelope steps by 40 dB and phi = 1/2 reads it at twice the bin): no cap.  "top511" and
    "interp-t0" are more than TEETH bounds away on every case.  "interp-nearest" is on the cases at -7 semitones; at 0 semitones every
    source position is an integer (kk / phi = 2 kk, kk / r = kk: t is 0, or 1 at the clip), rounding the weight changes nothing and the
    variant IS the definition there, which is asserted instead."""
    ref, turns = FC.top_reference(c), FC.top_reference(c, "turns")
    wrong = {w: FC.top_reference(c, wrong=w) for w in ("top511", "interp-t0", "interp-nearest")}
    stats = FC.top_stats(c)
    for s in range(S):
        gate = np.abs(ref[s] - turns[s]).max() / max(1.0, np.abs(ref[s]).max())
        bnd = pv_cases.bound(c.hop, ref[s])
        away = {w: _away(ref[s], r[s], bnd) for w, r in wrong.items()}
        print(f"FORMANTEDGE GATE top {FC.top_id(c)} stream {s}: forms {gate:.3g} share {stats[s]['clamped'] / stats[s]['pairs']:.3f} "
              f"max {np.abs(ref[s]).max():.3f}  " + "  ".join(f"{w} {v:.3g}" for w, v in away.items()))
        assert gate <= FC.GATE_TOL, (s, gate)
        for w, v in away.items():
            if w == "interp-nearest" and c.semitones == 0.0:
                assert v == 0.0, (s, w, v)
            else:
                assert v > FC.TEETH, (s, w, v)


def test_the_clip_on_the_pitch_ratio_side_cannot_be_observed():
    """Why no case is written for it: with r = 1/2 (and phi = 1) a clip at 511 gives the same output, sample for sample."""
    c = FC.TOP_CASES[0]
    x = FC.top_input(c)[0]
    ratio = np.full(c.nF, 0.5)
    a = FR.frame_loop(x, FC.F, c.hop, ratio, 1.0, c.nc)
    b = FR.frame_loop(x, FC.F, c.hop, ratio, 1.0, c.nc, wrong="top511")
    assert np.abs(a - b).max() <= 1e-3 * pv_cases.bound(c.hop, a)


# ---- 3. levels ------------------------------------------------------------------------------------------------------------------------------------
FLOORS = ("floor-1e-11", "floor-1e-13", "floor-none", "floor-on-m")


@pytest.mark.parametrize("c", FC.LEVEL_CASES, ids=FC.level_id)
def test_level_cases_gate_and_teeth(c):
    """The bound is level_bound (no max(1, .)), the gate relative to max |ref|.  Every wrong floor is more than TEETH of these bounds away at
    e <= -16 (at 2^15 the floor plays no part: that case is there for the large level).  At e = -20 the reference is NOT 2^-20 x the
    full-level reference: a scale-invariant kernel cannot pass."""
    ref, turns = FC.level_reference(c), FC.level_reference(c, "turns")
    wrong = {w: FC.level_reference(c, wrong=w) for w in FLOORS} if c.e <= -16 else {}
    full = FC.level_reference(FC.LevelCase(c.hop, c.nF, c.extra, 0)) if c.e == -20 else None
    for s in range(S):
        peak = np.abs(ref[s]).max()
        gate = np.abs(ref[s] - turns[s]).max() / peak
        bnd = FC.level_bound(c.hop, ref[s])
        away = {w: _away(ref[s], r[s], bnd) for w, r in wrong.items()}
        print(f"FORMANTEDGE GATE level {FC.level_id(c)} stream {s}: forms {gate:.3g} max {peak:.3g}  " + "  ".join(f"{w} {v:.3g}" for w, v in away.items()))
        assert peak > 0.05 * 2.0 ** c.e and gate <= FC.LEVEL_GATE_TOL, (s, gate)
        for w, v in away.items():
            assert v > FC.TEETH, (s, w, v)
        if full is not None:
            off = np.abs(ref[s] - full[s] * 2.0 ** c.e).max() / peak
            print(f"FORMANTEDGE GATE level {FC.level_id(c)} stream {s}: from the scaled full-level reference {off:.3g} of the peak")
            assert off > FC.NON_HOMOGENEITY, (s, off)


def test_level_step_gate_and_the_silent_onset_fails_it():
    ref, turns = FC.step_reference(), FC.step_reference("turns")
    x = FC.step_input()
    assert np.abs(x[:, :FC.STEP_HEAD]).max() < 1e-6 and np.abs(x[:, FC.STEP_HEAD:-FC.STEP_TAIL]).max() > 0.5
    c = FC.STEP_CASE
    assert c.hop + FC.F <= FC.STEP_HEAD < 2 * c.hop + FC.F and FC.STEP_QUIET == 2 * c.hop          # frames 0 and 1 wholly quiet, frame 2 not
    for s in range(S):
        gate = np.abs(ref[s] - turns[s]).max() / max(1.0, np.abs(ref[s]).max())
        head = np.abs(ref[s, :FC.STEP_QUIET] - turns[s, :FC.STEP_QUIET]).max() / np.abs(ref[s, :FC.STEP_QUIET]).max()
        print(f"FORMANTEDGE GATE step stream {s}: forms {gate:.3g}, on the quiet head {head:.3g} of its peak {np.abs(ref[s, :FC.STEP_QUIET]).max():.3g}")
        assert gate <= FC.GATE_TOL and head <= FC.LEVEL_GATE_TOL, (s, gate, head)
    # exact digital silence in front of the onset: the all-zero frame's wrap ties.  Recorded, and the reason it gets property checks only
    x, ratio, worst = FC.silence_onset_input(), FC.ratios_of(c), 0.0
    for s in range(S):
        a = FR.frame_loop(x[s], FC.F, c.hop, ratio[s], FC.FORMANT_RATIOS[s], c.nc)
        b = FR.frame_loop(x[s], FC.F, c.hop, ratio[s], FC.FORMANT_RATIOS[s], c.nc, "turns")
        worst = max(worst, np.abs(a - b).max() / np.abs(a).max())
        assert np.all(a[:c.hop * 2] == 0)                                                           # every covering frame silent
    print(f"FORMANTEDGE GATE silent onset: the two forms differ by up to {worst:.3g} of the peak")
    assert worst > 1e-3


# ---- 4. every lifter --------------------------------------------------------------------------------------------------------------------------------
def test_every_lifter_gate():
    """The clamp share reaches 0.15 on the pure tone: no cap applies here."""
    worst, share = 0.0, 0.0
    for nc in FC.ALL_LIFTERS:
        ref, turns = FC.lifter_reference(nc), FC.lifter_reference(nc, "turns")
        for s in range(S):
            gate = np.abs(ref[s] - turns[s]).max() / max(1.0, np.abs(ref[s]).max())
            assert gate <= FC.GATE_TOL, (nc, s, gate)
            worst = max(worst, gate)
            share = max(share, FC.lifter_stats(nc)[s]["clamped"] / FC.lifter_stats(nc)[s]["pairs"])
    # neighbouring lifters are different signals, by more than TEETH bounds (a call that took another call's lifter)
    c = FC.LIFTER_CASE
    near = min(_away(FC.lifter_reference(nc)[s], FC.lifter_reference(nc + 1)[s], pv_cases.bound(c.hop, FC.lifter_reference(nc)[s]))
               for nc in FC.ALL_LIFTERS[:-1] for s in range(S))
    print(f"FORMANTEDGE GATE lifters 4 .. 64: forms {worst:.3g}, largest clamp share of a stream {share:.3f}, neighbouring lifters {near:.3g} bounds apart")
    assert near > FC.TEETH


# ---- 5. streaming -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.STREAM_EDGE_CASES, ids=FC.stream_id)
def test_streaming_edge_cases_gate_and_teeth(c):
    ref, turns, nxt = FC.stream_edge_reference(c), FC.stream_edge_reference(c, "turns"), FC.stream_edge_reference(c, shift=1)
    assert ref.shape == (S, c.N * c.n_blocks) and c.N * c.n_blocks >= 6 * FC.F
    for s in range(S):
        gate = np.abs(ref[s] - turns[s]).max() / max(1.0, np.abs(ref[s]).max())
        away = _away(ref[s], nxt[s], pv_cases.bound(c.hop, ref[s]))
        print(f"FORMANTEDGE GATE stream {FC.stream_id(c)} stream {s}: forms {gate:.3g}  next-block {away:.3g}")
        assert gate <= FC.GATE_TOL and away > FC.TEETH, (s, gate, away)
        assert np.all(ref[s, :pv_cases.latency(c.N, c.hop)] == 0) and np.sqrt((ref[s] ** 2).mean()) > 0.01


@pytest.mark.parametrize("c", FC.FORMANT_SCENARIOS, ids=pv_cases.scenario_id)
def test_formant_scenarios_gate_teeth_and_where_their_resets_land(c):
    ref, landed, held = FC.scenario_reference(c)
    hits = {i: (fr, m) for per_stream in landed for i, fr, m in per_stream}
    assert sorted(hits) == [4, 8, 13]
    assert hits[4][0] != 0 and hits[8][0] != 0, hits                                  # in the middle of a round, at every hop
    assert any(fr != 0 and m < pv_cases.F for fr, m in hits.values()), hits           # ... followed by a call shorter than a frame
    spans = pv_cases.call_spans(c.n_blocks, c.calls)
    assert FC.scenario_kind(8) == "formant" and hits[8][0] != 0                        # a reset in the middle of a round, pending at a formant call
    assert [FC.scenario_kind(i) for i in sorted(c.changes)] == ["formant", "formant", "curve", "formant", "formant"]
    assert [FC.scenario_kind(i) for i in (4, 13)] == ["plain", "plain"] and len(spans) > 20
    assert held == [-12.0, 5.0, 0.37, -4.0]
    turns = FC.scenario_reference(c, "turns")[0]
    late, early = FC.scenario_reference(c, shift=1)[0], FC.scenario_reference(c, shift=-1)[0]
    for s in range(ref.shape[0]):
        gate = np.abs(ref[s] - turns[s]).max() / max(1.0, np.abs(ref[s]).max())
        bnd = pv_cases.bound(c.hop, ref[s])
        a, b = _away(ref[s], late[s], bnd), _away(ref[s], early[s], bnd)
        print(f"FORMANTEDGE GATE scenario {pv_cases.scenario_id(c)} stream {s}: forms {gate:.3g}  late {a:.3g}  early {b:.3g}")
        assert gate <= FC.GATE_TOL, (s, gate)
        if s == 1:
            # stream 1 has no reset, and its two changes (calls 2 and 5) are pending at formant calls, which store the interval and do not
            # use it.  One call late they still precede the plain calls 4 and 7 that do: the late schedule computes the same stream.  One
            # call early they precede the plain calls 1 and 4, and only at hop 64 does a frame end inside either.  The schedule of this
            # stream is held by the held intervals (asserted on the GPU), the others' by the samples.
            assert a == 0.0 and (b == 0.0 or b > FC.TEETH), (a, b)
        else:
            assert a > FC.TEETH and b > FC.TEETH, (s, a, b)


def test_three_hundred_streaming_streams_gate():
    ref, turns = FC.big_stream_reference(), FC.big_stream_reference("turns")
    for s in FC.BIG_CHECKED:
        gate = np.abs(ref[s] - turns[s]).max() / max(1.0, np.abs(ref[s]).max())
        print(f"FORMANTEDGE GATE big-stream stream {s}: forms {gate:.3g}")
        assert gate <= FC.GATE_TOL and np.abs(ref[s]).max() > 0.05, (s, gate)
