"""The phase-vocoder reference on the CPU (tests/pv_cases.py): the conditioning gate of every case that tests/test_gpu_pv_matrix.py
compares pointwise -- the restatement in radians (tests/stft_reference.py, tests/pv_stream_reference.py) and the one in turns
(pv_cases.roundtrip_turns / PvStreamTurns) must agree at EVERY sample within 1e-9 max(1, max |ref|) (measured: a few 1e-13) -- the
record that the degenerate inputs do NOT pass it (which is why they are tested without a pointwise reference), and the streaming
restatement's reset and per-frame ratio schedule at every hop."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases as K  # noqa: E402
import pv_stream_reference as P  # noqa: E402
import stft_reference as R  # noqa: E402


def _gate(a, b, what):
    """Every sample, none left out."""
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
    tol = K.GATE_TOL * max(1.0, float(np.abs(a).max()))
    worst = float(np.abs(a - b).max())
    print(f"PVGATE {what} radians-vs-turns max {worst:.3e} tol {tol:.3e}")
    assert worst <= tol, (what, worst, tol)


def test_the_case_table_covers_what_it_claims():
    for hop in K.HOPS:
        cs = [c for c in K.ONE_SHOT_CASES if c.hop == hop]
        semis = {c.semitones for c in cs}
        assert len(semis) >= 3 and {12.0, -12.0} <= semis and semis <= set(K.SEMITONES)
        for v in semis:
            Ts = [c.T for c in cs if c.semitones == v]
            assert {K.n_frames(T, hop) % 4 for T in Ts} == {0, 1, 2, 3}
            assert any(T % 2 for T in Ts) and any(T % hop for T in Ts) and K.F in Ts and K.F + hop - 1 in Ts
            assert all(T >= K.F for T in Ts)
    assert {(c.hop, c.N) for c in K.STREAM_CASES} == {(h, n) for h in (64, 128, 512) for n in (17, 64, 100, 1000, 1024, 4096)}
    for c in K.STREAM_CASES:
        assert c.N * c.n_blocks >= 10 * K.F and len(set(c.semitones)) == len(c.semitones) == 5
    assert [c.hop for c in K.SCENARIOS] == list(K.HOPS)


@pytest.mark.parametrize("case", K.ONE_SHOT_CASES, ids=K.one_shot_id)
def test_gate_one_shot_cases(case):
    x = K.one_shot_input(case)
    assert x.dtype == np.float32 and x.shape == (5, case.T)
    _gate(K.one_shot_reference(case, x), K.one_shot_reference(case, x, "turns"), "one-shot " + K.one_shot_id(case))


@pytest.mark.parametrize("case", K.STREAM_CASES, ids=K.stream_id)
def test_gate_stream_cases(case):
    x = K.stream_input(case)
    ref = K.stream_reference(case, x)
    _gate(ref, K.stream_reference(case, x, "turns"), "stream " + K.stream_id(case))
    # and the streamed restatement is the one-shot one delayed by the latency (here at N = 17 and hop 64 / 512 too)
    L = K.latency(case.N, case.hop)
    for s in (0, 3):
        one = R.stft_roundtrip(x[s], K.F, case.hop, ratio=K.ratio_of(case.semitones[s]))
        assert np.all(ref[s, :L] == 0) and np.abs(ref[s, L:] - one[:x.shape[1] - L]).max() <= 1e-12


@pytest.mark.parametrize("case", K.SCENARIOS, ids=K.scenario_id)
def test_gate_scenarios_and_where_their_resets_land(case):
    x = K.scenario_input(case)
    ref, landed = K.scenario_reference(case, x)
    _gate(ref, K.scenario_reference(case, x, "turns")[0], "scenario " + K.scenario_id(case))
    hits = [h for per_stream in landed for h in per_stream]
    assert len(hits) == sum(len(v) for v in case.resets.values())
    assert any(fr != 0 for _, fr, _ in hits), hits                       # a reset in the middle of a round ...
    assert any(fr != 0 and m < K.F for _, fr, m in hits), hits           # ... followed by a call shorter than a frame
    # the schedule one call early or late is another signal, far beyond the GPU test's bound
    for sh in (-1, 1):
        other = K.scenario_reference(case, x, shift=sh)[0]
        assert np.abs(other - ref).max() > 1e3 * K.bound(case.hop, ref), sh


@pytest.mark.parametrize("hop", K.HOPS)
@pytest.mark.parametrize("name", K.DEGENERATE)
def test_degenerate_inputs_do_not_pass_the_gate(name, hop):
    """Silence passes trivially (all zeros in both forms).  The others sit on wrap ties: the two forms of the SAME definition differ far
    beyond the gate, so neither is a reference for the kernel there; the GPU file tests them by properties instead."""
    T = 8 * K.F + hop + 3
    x = K.degenerate(name, T)
    worst = 0.0
    for v in (7.0, -12.0, 0.37):
        a = R.stft_roundtrip(x, K.F, hop, ratio=K.ratio_of(v))
        b = K.roundtrip_turns(x, K.F, hop, K.ratio_of(v))
        assert np.isfinite(a).all() and np.isfinite(b).all()
        worst = max(worst, float(np.abs(a - b).max()) / max(1.0, float(np.abs(a).max())))
        # the amplitude ceiling holds for both forms, whatever they decided
        top = K.magnitude_ceiling(x, hop) * (1 + 1e-6)
        assert np.abs(a).max() <= top and np.abs(b).max() <= top
    print(f"PVGATE degenerate {name} hop{hop} radians-vs-turns max {worst:.3e}")
    if name == "silence":
        assert worst == 0.0
    else:
        assert worst > 1e3 * K.GATE_TOL, (name, hop, worst)


def test_turns_form_is_a_round_trip_at_ratio_one():
    """With ratio 1 on a steady tone the stage is close to the identity: the interior comes back (an end-to-end check of the second
    statement that does not involve the first)."""
    x = K.tone(12 * K.F, 1000.0, 0.5).astype(np.float64)
    for hop in K.HOPS:
        y = K.roundtrip_turns(x, K.F, hop, 1.0)
        assert np.abs(y[2 * K.F:-2 * K.F] - x[2 * K.F:-2 * K.F]).max() < 1e-6


@pytest.mark.parametrize("hop", K.HOPS)
def test_reset_mid_round_equals_a_fresh_stream(hop):
    N = 100
    x = K.harmonic(N * 150, 3, seed=hop).astype(np.float64)
    ratio = K.ratio_of(-5.0)
    s = P.PvStreamRef(N, hop, ratio=ratio)
    pos = 0
    while not (s.nf >= 6 and s.nf % K.ROUND != 0):                       # stop in the middle of a round
        s.process(x[pos:pos + N])
        pos += N
    assert s.nf % K.ROUND != 0 and pos < N * 60
    s.reset()
    assert s.nf == 0 and s.n == 0 and s.frame_ratios == []
    tail = x[pos:]
    fresh = P.PvStreamRef(N, hop, ratio=ratio)
    ya = np.concatenate([s.process(tail[i:i + 3 * N]) for i in range(0, len(tail), 3 * N)])
    yb = np.concatenate([fresh.process(tail[i:i + 3 * N]) for i in range(0, len(tail), 3 * N)])
    assert np.array_equal(ya, yb) and np.abs(ya).max() > 0.1
    assert s.frame_ratios == fresh.frame_ratios and len(s.frame_ratios) == K.n_frames(len(tail), hop)


@pytest.mark.parametrize("hop", [64, 512])
def test_ratio_schedule_is_per_frame(hop):
    """A frame is computed in the call in which its last sample arrives, with that call's ratio: frame_ratios, by frame index."""
    N, F = 100, K.F
    s = P.PvStreamRef(N, hop, ratio=1.0)
    x = K.white(N * 60, seed=hop).astype(np.float64)
    sched = {0: 1.0, 11: K.ratio_of(7.0), 12: K.ratio_of(-3.0), 30: 2.0, 31: 0.5}
    want, cur, n = [], 1.0, 0
    for i in range(60):
        cur = sched.get(i, cur)
        s.process(x[i * N:(i + 1) * N], sched.get(i))
        n += N
        done = (n - F) // hop + 1 if n >= F else 0
        want += [cur] * (done - len(want))
    assert s.frame_ratios == want and len(want) == K.n_frames(N * 60, hop)
    assert len(set(want)) == (5 if hop == 64 else 4)                    # hop 512: no frame ends in calls 11 and 12, the +7 never shows
