"""CPU-side checks of the formant definition (tests/pv_formant_reference.py) on the cases the GPU tests compare pointwise
(tests/pv_formant_cases.py): the gate -- its radians and its turns form agree within GATE_TOL, the project's standing condition for a
pointwise comparison --, the envelope by two transforms against a direct cosine sum, the teeth -- four plausible wrong kernels each differ
from the reference by more than TEETH x the GPU test's bound --, bit identity with the plain pitch shift where the formant ratio follows
the pitch, the share of (frame, bin) pairs at the gain's clamp, and the conditioning of the envelope stage."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_curve_cases as CC  # noqa: E402
import pv_formant_cases as FC  # noqa: E402
import pv_formant_reference as FR  # noqa: E402


# ---- the gate -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.ALL_CASES, ids=FC.case_id)
def test_gate_the_two_forms_agree_and_the_clamp_share_is_small(c):
    ref, turns = FC.reference(c), FC.reference(c, "turns")
    assert ref.shape == (FC.N_STREAMS, FC.length(c)) and np.all(np.isfinite(ref))
    gap = np.abs(ref - turns).max() / max(1.0, np.abs(ref).max())
    st = FC.STATS[c]
    share = st["clamped"] / st["pairs"]
    print(f"FORMANT GATE {FC.case_id(c)}: forms {gap:.3g} clamp share {share:.4f}")
    assert gap <= FC.GATE_TOL, gap
    assert st["pairs"] == FC.N_STREAMS * c.nF * (FC.F // 2 + 1)
    assert share <= FC.CLAMP_SHARE_CAP, share                   # the cases test the envelope, not the clamp
    assert np.abs(ref).max() > 0.05


def test_gate_of_the_streaming_and_the_big_case():
    c = FC.STREAM_CASES[1]                                       # the one test_gpu_pv_formant.py compares with NumPy
    x, ratio = FC.stream_input(c), pv_cases.ratio_of(FC.stream_semitones(c))
    stats = {}
    for s in range(FC.N_STREAMS):
        a = FR.by_block(x[s], c.N, c.hop, ratio[:, s], FC.FORMANT_RATIOS[s], c.nc, stats=stats)
        b = FR.by_block(x[s], c.N, c.hop, ratio[:, s], FC.FORMANT_RATIOS[s], c.nc, "turns")
        assert np.abs(a - b).max() <= FC.GATE_TOL * max(1.0, np.abs(a).max()), s
        # the stream is the one-shot delayed by the latency, with the table expanded per frame
        T, L = c.N * c.n_blocks, pv_cases.latency(c.N, c.hop)
        one = FR.frame_loop(x[s], FC.F, c.hop, FC.per_frame(ratio, c.N, c.hop, T)[s], FC.FORMANT_RATIOS[s], c.nc)
        n = min(((T - FC.F) // c.hop + 1) * c.hop, T - L)
        assert np.abs(a[L:L + n] - one[:n]).max() <= 1e-12 and np.all(a[:L] == 0), s
    big, big_t = FC.big_reference(), FC.big_reference("turns")
    for s in FC.BIG_CHECKED:
        assert np.abs(big[s] - big_t[s]).max() <= FC.GATE_TOL * max(1.0, np.abs(big[s]).max()), s
    # the clamp share of these two pointwise comparisons, as in every one-shot case
    for name, st in (("stream", stats), ("big", FC.STATS["big"])):
        share = st["clamped"] / st["pairs"]
        print(f"FORMANT GATE {name}: clamp share {share:.4f} of {st['pairs']} pairs")
        assert st["pairs"] > 0 and share <= FC.CLAMP_SHARE_CAP, (name, share)


def test_envelope_by_two_transforms_equals_the_direct_cosine_sum():
    x = pv_cases.mixed_streams(FC.F, seed=3)
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FC.F) / FC.F))
    for s in range(FC.N_STREAMS):
        m = np.abs(np.fft.rfft(x[s] * w))
        for nc in (4, 5, 32, 63, 64):
            a, b = FR.envelope(m, FC.F, nc), FR.envelope_direct(m, FC.F, nc)
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max()), (s, nc, np.abs(a - b).max())
    # digital silence is a flat envelope: the gain is 1 whatever the ratios
    d, n = FR.log_gain(np.zeros(FC.F // 2 + 1), FC.F, 2.0, 0.5, 32)
    assert n == 0 and np.abs(d).max() < 1e-12
    lw = FR.lifter_window(FC.F, 7)
    assert lw[:7].tolist() == [1.0] * 7 and lw[7] == 0.5 and lw[8] == 0 and np.array_equal(lw[1:], lw[1:][::-1]) and lw.sum() == 7 + 6 + 1.0


# ---- the teeth ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["nc+1", "nc-1", "nohalf", "phi-next", "roll"])
def test_teeth_a_wrong_kernel_is_far_outside_the_bound(variant):
    worst = np.inf
    for c in FC.ALL_CASES:
        if variant == "roll" and c.nF < 2:
            continue                                             # (a roll of one frame's curve changes nothing)
        ref = FC.reference(c)
        d = np.abs(FC.reference(c, variant=variant) - ref).max() / FC.bound(c, ref)
        worst = min(worst, d)
        assert d > FC.TEETH, (FC.case_id(c), variant, d)
    print(f"FORMANT TEETH {variant}: smallest difference {worst:.0f} x bound")


# ---- phi = r is the plain pitch shift ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", FC.HOPS)
def test_formant_ratio_equal_to_the_pitch_ratio_is_the_plain_output_bit_for_bit(hop):
    c = FC.FormantCase(hop, 19, 3, "steps", 32)
    x, ratio = FC.case_input(c), FC.ratios_of(c)
    for form in ("radians", "turns"):
        for s in range(FC.N_STREAMS):
            plain = CC.frame_loop(x[s], FC.F, hop, ratio[s], form)
            same = FR.frame_loop(x[s], FC.F, hop, ratio[s], "pitch", c.nc, form)
            assert np.array_equal(plain, same), (form, s)
            assert not np.array_equal(plain, FR.frame_loop(x[s], FC.F, hop, ratio[s], 1.0, c.nc, form))
    assert np.exp(0.0) == 1.0


# ---- conditioning ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", FC.HOPS)
def test_the_envelope_stage_adds_no_conditioning_problem(hop):
    """A perturbation of the input at the 1e-10 level (the size of the difference between two correct double-precision implementations,
    with margin) moves the formant output by no more than 16 times what it moves the plain pitch shift's -- 16 is the gain's clamp, the
    most a bin's change can be scaled by -- plus 1e-3 of the GPU test's bound for the envelope's own smooth dependence on the spectrum."""
    c = FC.FormantCase(hop, 19, 3, "glide", 32)
    x, ratio = FC.case_input(c).astype(np.float64), FC.ratios_of(c)
    xp = x + 1e-10 * np.random.default_rng([hop, 13]).standard_normal(x.shape)
    for s in range(FC.N_STREAMS):
        f0 = FR.frame_loop(x[s], FC.F, hop, ratio[s], FC.FORMANT_RATIOS[s], c.nc)
        f1 = FR.frame_loop(xp[s], FC.F, hop, ratio[s], FC.FORMANT_RATIOS[s], c.nc)
        p0 = CC.frame_loop(x[s], FC.F, hop, ratio[s])
        p1 = CC.frame_loop(xp[s], FC.F, hop, ratio[s])
        df, dp = np.abs(f1 - f0).max(), np.abs(p1 - p0).max()
        print(f"FORMANT CONDITIONING hop {hop} stream {s}: formant moved {df:.3g}, plain {dp:.3g}")
        assert df <= 16.0 * dp + 1e-3 * pv_cases.bound(hop, f0), (s, df, dp)
