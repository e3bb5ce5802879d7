"""CPU-side checks of the peak-locked pitch shift's definition (tests/pv_lock_reference.py) and of the cases the GPU tests compare on
(tests/pv_lock_cases.py): the gate (two statements of the reference agree on every case), the identity at ratio 1, the clamp, the
degenerate inputs' properties, the teeth (named mutants of the reference are far away on a gated case chosen to see them), the quality the
stage exists for (a shifted tone's envelope ripples less than under the plain stage), the streaming statement, and that the entry points
are declared and exported.  profiles/pv_lock_quality.txt is tools/pv_lock_quality.py's print of the same table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_lock_cases as LC  # noqa: E402
import pv_lock_reference as LR  # noqa: E402
import stft_reference  # noqa: E402

SYMBOLS = ["vp_stft_pitch_shift_locked", "vp_pv_process_blocks_locked_device"]


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.GATE_CASES, ids=LC.gate_id)
def test_the_two_forms_of_the_reference_agree(c):
    a, b = LC.gate_reference(c), LC.gate_reference(c, "b")
    assert np.all(np.isfinite(a)) and np.abs(a).max() > 1e-3
    rel = np.abs(a - b).max() / max(1.0, np.abs(a).max())
    print(f"PVLOCK gate {LC.gate_id(c)}: {rel:.3g}")
    assert rel <= LC.GATE_TOL, rel


def test_the_gpu_cases_pass_the_gate_too():
    """The pointwise GPU cases (shorter, six curves, the tail): the streams of the shortest and the longest case of two hops."""
    for hop, nF in ((64, 8), (512, 5), (256, 1)):
        x = LC.gpu_input(hop, nF)
        for name in LC.GPU_CURVES:
            r = LC.gpu_ratios(name, hop, nF)
            ref = LC.gpu_reference(hop, nF, name)
            for s in range(len(x)):
                b = LR.locked_roundtrip_b(x[s], r[s], LC.F, hop)
                assert np.abs(ref[s] - b).max() <= LC.GATE_TOL * max(1.0, np.abs(b).max()), (hop, nF, name, s)


@pytest.mark.parametrize("hop", [64, 512])
def test_degenerate_inputs_are_finite_and_bounded_and_their_gate_is_recorded(hop):
    T = LC.length(9, hop, 5)
    for name in LC.DEGENERATE:
        x = pv_cases.degenerate(name, T)
        for cv in ("steps", "outside"):
            r = LC.curve(cv, 9, hop)
            a, b = LR.locked_roundtrip(x, r, LC.F, hop), LR.locked_roundtrip_b(x, r, LC.F, hop)
            rel = np.abs(a - b).max() / max(1.0, np.abs(a).max())
            print(f"PVLOCK degenerate {name} hop{hop} {cv}: forms differ by {rel:.3g} ({'passes' if rel <= LC.GATE_TOL else 'FAILS'} the gate)")
            assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
            assert np.abs(a).max() <= pv_cases.magnitude_ceiling(x, hop) + 1e-9             # a translation and a rotation of the bins
            if name == "silence":
                assert np.all(a == 0) and np.all(b == 0)


# ---- identity, clamp --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", LC.GPU_HOPS)
def test_ratio_one_is_the_round_trip_exactly(hop):
    for sig in ("voice+noise", "noise", "silence-noise"):
        x = LC.SIGNALS[sig](LC.length(9, hop, 5), 1)
        assert np.array_equal(LR.locked_roundtrip(x, 1.0, LC.F, hop), stft_reference.stft_roundtrip(x, LC.F, hop)), sig
        assert np.array_equal(LR.locked_roundtrip(x, np.ones(9), LC.F, hop), stft_reference.stft_roundtrip(x, LC.F, hop)), sig


def test_a_curve_outside_the_clamp_equals_the_clamped_one():
    x = LC.SIGNALS["voice"](LC.length(9, 256, 5), 2)
    for out, inside in ((0.3, 0.5), (0.0, 0.5), (-1.0, 0.5), (np.nan, 0.5), (2.7, 2.0), (np.inf, 2.0)):
        assert np.array_equal(LR.locked_roundtrip(x, out, LC.F, 256), LR.locked_roundtrip(x, inside, LC.F, 256)), out
    r = LC.curve("outside", 9)
    assert np.array_equal(LR.locked_roundtrip(x, r, LC.F, 256), LR.locked_roundtrip(x, np.clip(np.nan_to_num(r, nan=0.5), 0.5, 2.0), LC.F, 256))


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", LR.MUTANTS)
def test_every_mutant_is_far_from_the_reference_on_a_gated_case(mutant):
    c = LC.TEETH_CASES[mutant]
    if c is None:                                                # strict: the plateau
        hop, x, r = LC.PLATEAU_HOP, LC.plateau_input(), LC.ratio_of(7.0)
        ref, b = LR.locked_roundtrip(x, r, LC.F, hop), LR.locked_roundtrip_b(x, r, LC.F, hop)
        mu = LR.locked_roundtrip(x, r, LC.F, hop, mutant)
        what = "centre clicks"
    else:
        assert c in LC.GATE_CASES
        hop, ref, b, mu, what = c.hop, LC.gate_reference(c), LC.gate_reference(c, "b"), LC.gate_reference(c, "a", mutant), LC.gate_id(c)
    assert np.abs(ref - b).max() <= LC.GATE_TOL * max(1.0, np.abs(ref).max())
    dist = np.abs(ref - mu).max() / LC.bound(hop, ref)
    print(f"PVLOCK mutant {mutant} on {what}: {dist:.3g} GPU bounds from the reference")
    assert dist >= LC.TEETH, dist


def test_the_plateau_case_has_one_peak_at_the_leftmost_bin():
    x = LC.plateau_input().astype(np.float64)
    w = stft_reference.window(LC.F)
    flat = 0
    for f in range(LC.PLATEAU_NF):
        m = np.abs(np.fft.rfft(x[f * LC.PLATEAU_HOP:f * LC.PLATEAU_HOP + LC.F] * w))
        assert len(np.unique(m)) == 1                                                     # flat to the last bit, or silence
        flat += m[0] > 0
    assert flat == 2


# ---- quality ------------------------------------------------------------------------------------------------------------------------------------
def test_a_shifted_tone_ripples_less_than_under_the_plain_stage():
    for freq in LC.QUALITY_TONES:
        x = LC.quality_tone(freq)
        for st in LC.QUALITY_SEMITONES:
            r = LC.ratio_of(st)
            rp, ap = LC.ripple(stft_reference.stft_roundtrip(x, LC.F, 256, ratio=r))
            rl, al = LC.ripple(LR.locked_roundtrip(x, r, LC.F, 256))
            print(f"PVLOCK quality {freq} Hz {st:+g} st: ripple plain {rp:.4f} locked {rl:.4f} (ratio {rl / rp:.3f}), amplitude plain {ap:.3f} locked {al:.3f}")
            assert rl < rp, (freq, st, rl, rp)


# ---- streaming ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,N", [(128, 100), (512, 17), (64, 1024)])
def test_block_by_block_is_the_one_shot_delayed_by_the_latency(hop, N):
    nb = max(-(-4 * LC.F // N), 8)
    x = LC.SIGNALS["voice+noise"](N * nb, seed=hop)
    tab = LC.ratio_of(np.random.default_rng([hop, N]).uniform(-13.0, 13.0, nb))
    y = LR.by_block(x, N, hop, tab)
    T = N * nb
    per_frame = LC.per_frame(tab[:, None], N, hop, T)[0]
    y1 = LR.locked_roundtrip(x, per_frame, LC.F, hop)
    L = pv_cases.latency(N, hop)
    n = min(len(per_frame) * hop, T - L)
    assert n > LC.F and np.all(y[:L] == 0) and np.array_equal(y[L:L + n], y1[:n])


# ---- the entry points -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_and_null_arguments_fail():
    from vocoderproject_amd import build
    lib = C.CDLL(build.build())
    txt = open(os.path.join(ROOT, "include", "vp_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s + "(" in txt, s
    assert "processBlocksLocked" in open(os.path.join(ROOT, "include", "vp_amd.hpp")).read()
    assert lib.vp_abi_version() == 3
    one = C.c_void_p(8)                                                               # (a non-null pointer that is never followed)
    lib.vp_stft_pitch_shift_locked.argtypes = [C.c_void_p] * 5
    lib.vp_pv_process_blocks_locked_device.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
    assert lib.vp_stft_pitch_shift_locked(None, one, one, one, None) == -1
    assert lib.vp_pv_process_blocks_locked_device(None, one, one, one, 1, None) == -1


def test_python_front_ends_refuse_locked_with_formant_before_any_launch():
    """No GPU here: the refusal must come before the library is asked for anything."""
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip
    ps = PhaseVocoderStream.__new__(PhaseVocoderStream)                                # (no handle: a call that reached the library would fail differently)
    ps.h = None
    with pytest.raises(ValueError):
        ps.process_device(None, None, locked=True, formant_semitones=0.0)
    with pytest.raises(ValueError):
        ps.run(np.zeros((1, 8), np.float32), locked=True, formant_semitones=0.0)
    with pytest.raises(ValueError):
        ps.autotune_device(None, None, None, locked=True, formant_semitones=0.0)
    assert callable(StftRoundTrip.pitch_shift_locked)
