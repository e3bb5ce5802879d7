"""The NumPy definition of the cross-synthesis (tests/pv_cross_reference.py) against itself: the two identities hold exactly, the streaming
form equals the one-shot delayed by the latency, the envelope equals its direct cosine sum, every WRONG variant is at least ten gates away
from the definition on some case of tests/pv_cross_cases.py (otherwise the GPU test could not tell it apart), the clamp engages on
carrier bins that are not exactly zero, and silent inputs give finite output."""
import numpy as np
import pytest

import pv_cross_cases as XC
import pv_cross_reference as XR
import pv_formant_reference as FR
import pv_stream_reference as P
import stft_reference as R

F = XC.F


def test_depth_zero_and_voice_equal_carrier_are_the_plain_round_trip_exactly():
    for hop in XC.HOPS:
        T = F + 7 * hop + 5
        v, c = XC.signals(T, seed=hop)
        for s in range(XC.N_STREAMS):
            plain = R.stft_roundtrip(c[s], F, hop)
            for depth in (0.0, -0.0, -3.0, float("nan")):                    # (fmax first: a NaN is 0)
                assert np.array_equal(XR.cross_synth(v[s], c[s], F, hop, depth, 32), plain), (hop, s, depth)
            for depth in (None, 1.0, 0.5):
                assert np.array_equal(XR.cross_synth(c[s], c[s], F, hop, depth, 4), plain), (hop, s, depth)
            assert not np.array_equal(XR.cross_synth(v[s], c[s], F, hop, 1.0, 32), plain)


def test_depth_is_clamped_to_the_unit_interval():
    assert [XR.clamp_depth(d) for d in (None, 2.0, 1.0, 0.25, 0.0, -1.0, float("nan"), float("inf"))] == [1.0, 1.0, 1.0, 0.25, 0.0, 0.0, 0.0, 1.0]
    v, c = XC.signals(F + 512)
    assert np.array_equal(XR.cross_synth(v[0], c[0], depth=7.0), XR.cross_synth(v[0], c[0], depth=None))


@pytest.mark.parametrize("N,hop", [(64, 256), (100, 256), (256, 256), (1024, 256), (1536, 256), (256, 64), (256, 512)])
def test_streaming_form_is_the_one_shot_delayed_by_the_latency(N, hop):
    L = P.latency(N, hop)
    assert L == F - int(np.gcd(N, hop))
    nb = max(3, -(-(F + 6 * hop + L) // N))
    T = nb * N
    v, c = XC.signals(T, seed=N + hop)
    for s, depth in ((0, None), (1, 0.5)):
        one = XR.cross_synth(v[s], c[s], F, hop, depth, 32)
        for calls in ([1], [3, 1, 16]):
            y = XR.stream(v[s], c[s], N, hop, depth, 32, calls)
            assert np.array_equal(y[:L], np.zeros(L)) and np.array_equal(y[L:], one[:T - L]), (s, calls)


def test_stream_reset_restarts_the_stream():
    N, hop = 256, 128
    v, c = XC.signals(12 * N)
    r = XR.CrossStreamRef(N, hop)
    r.process(v[0][:5 * N], c[0][:5 * N])
    r.reset()
    y = np.concatenate([r.process(v[0][b * N:(b + 1) * N], c[0][b * N:(b + 1) * N]) for b in range(5, 12)])
    assert np.array_equal(y, XR.stream(v[0][5 * N:], c[0][5 * N:], N, hop))


def test_envelope_is_its_direct_cosine_sum():
    v, c = XC.signals(F)
    w = R.window(F)
    for x in (v[0], c[0], c[1], c[2], np.zeros(F)):
        m = np.abs(np.fft.rfft(x * w))
        for nc in XC.LIFTERS:
            a, b = FR.envelope(m, F, nc), FR.envelope_direct(m, F, nc)
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), nc


def test_every_wrong_variant_is_ten_gates_from_the_definition_on_some_case(capsys):
    worst = {w: (0.0, None) for w in XR.WRONG}
    for c in XC.CASES:
        if c.length not in ("tail", "uncovered"):
            continue
        ref = XC.reference(c)
        for w in XR.WRONG:
            if worst[w][0] >= XC.TEETH:                                       # (one case is enough)
                continue
            bad = XC.reference(c, w)
            d = max(np.abs(bad[s] - ref[s]).max() / XC.gate(ref[s]) for s in range(XC.N_STREAMS))
            if d > worst[w][0]:
                worst[w] = (d, XC.case_id(c))
    with capsys.disabled():
        for w, (d, cid) in worst.items():
            print(f"\n  cross wrong {w:18s} {d:12.1f} gates on {cid}", end="")
    assert all(d >= XC.TEETH for d, _ in worst.values()), worst


def test_the_clamp_engages_on_carrier_bins_that_are_not_zero():
    # stream 1 ("late"): in front of the sawtooth's start; stream 2 ("band"): above the band -- with the NULL table (depth 1)
    c = XC.CrossCase(256, "uncovered", 32, False)
    v, x = XC.case_input(c)
    for s, least in ((1, 0.01), (2, 0.5)):
        stats = {}
        XR.cross_synth(v[s], x[s], F, c.hop, None, c.nc, stats=stats)
        assert stats["clamped_nonzero"] >= least * stats["pairs"], (s, stats)
    stats = {}
    XR.cross_synth(v[0], x[0], F, c.hop, None, c.nc, stats=stats)
    assert stats["clamped"] == 0, stats                                       # the plain pair never reaches it


def test_silent_inputs_give_finite_output_and_a_silent_carrier_gives_zeros():
    T, hop = F + 5 * 256, 256
    v, c = XC.signals(T)
    z = np.zeros(T, np.float32)
    for nc in XC.LIFTERS:
        y = XR.cross_synth(z, c[0], F, hop, None, nc)                        # a silent voice silences the carrier: no lower clamp
        assert np.all(np.isfinite(y)) and np.abs(y).max() < 1e-3 * np.abs(R.stft_roundtrip(c[0], F, hop)).max()
        assert np.array_equal(XR.cross_synth(v[0], z, F, hop, None, nc), np.zeros(T))
        assert np.array_equal(XR.cross_synth(z, z, F, hop, None, nc), np.zeros(T))
