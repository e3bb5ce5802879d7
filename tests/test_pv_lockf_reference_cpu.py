"""CPU-side checks of the definition of the peak-locked pitch shift with sub-bin region offsets (tests/pv_lockf_reference.py) and of the
cases the GPU tests compare on (tests/pv_lockf_cases.py): the gate (the two statements agree on every gate case), the identity at ratio 1
(the integer definition's array, exactly), the clamp, the teeth (every named mutant of the new steps is far away on a gated case chosen to
see it), the conditioning of every item the GPU compares against NumPy, the quality the stage exists for (level and ripple against the
plain and the integer-offset stages), the spectral maximum at f r, the streaming statement, and that the entry points are declared and
exported.  profiles/pv_lockf_quality.txt is tools/pv_lockf_quality.py's print of the quality table."""
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
import pv_lockf_cases as FC  # noqa: E402
import pv_lockf_reference as FR  # noqa: E402
import stft_reference  # noqa: E402

SYMBOLS = ["vp_stft_pitch_shift_locked_subbin", "vp_pv_process_blocks_locked_subbin_device"]
F = LC.F


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.GATE_CASES, ids=LC.gate_id)
def test_the_two_forms_of_the_reference_agree(c):
    a, b = FC.gate_reference(c), FC.gate_reference(c, "b")
    assert np.all(np.isfinite(a)) and np.abs(a).max() > 1e-3
    rel = np.abs(a - b).max() / max(1.0, np.abs(a).max())
    print(f"PVLOCKF gate {LC.gate_id(c)}: {rel:.3g}")
    assert rel <= FC.GATE_TOL, rel


def test_the_gpu_cases_pass_the_gate_too():
    """The pointwise GPU cases (shorter, six curves, the tail): the streams of the shortest and the longest case of two hops."""
    for hop, nF in ((64, 8), (512, 5), (256, 1)):
        x = LC.gpu_input(hop, nF)
        for name in LC.GPU_CURVES:
            r = LC.gpu_ratios(name, hop, nF)
            ref = FC.gpu_reference(hop, nF, name)
            for s in range(len(x)):
                b = FR.lockf_roundtrip_b(x[s], r[s], F, hop)
                assert np.abs(ref[s] - b).max() <= FC.GATE_TOL * max(1.0, np.abs(b).max()), (hop, nF, name, s)


def test_the_trace_changes_no_bit_and_carries_the_offsets():
    for c in LC.GATE_CASES[::5]:
        x, r, tr = LC.gate_input(c), LC.curve(c.curve, c.nF, c.hop), []
        y = FR.lockf_roundtrip(x, r, F, c.hop, trace=tr)
        assert np.array_equal(y, FC.gate_reference(c)), LC.gate_id(c)
        assert len(tr) == c.nF
        for t in tr:
            assert len(t["delta"]) == len(t["P"]) == len(t["D"]) and np.all(np.abs(t["delta"]) <= 0.5)
            inner = (t["P"] > 0) & (t["P"] < F // 2)
            assert np.all(t["delta"][~inner] == 0)
            assert np.allclose(t["D"], (t["P"] + t["delta"]) * (t["r"] - 1.0), rtol=0, atol=1e-12)


# ---- identity, clamp --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", LC.GPU_HOPS)
def test_ratio_one_is_the_integer_definition_s_array_exactly(hop):
    for sig in ("voice+noise", "noise", "silence-noise", "square"):
        x = LC.SIGNALS[sig](LC.length(9, hop, 5), 1)
        want = LR.locked_roundtrip(x, 1.0, F, hop)
        assert np.array_equal(FR.lockf_roundtrip(x, 1.0, F, hop), want), sig
        assert np.array_equal(FR.lockf_roundtrip(x, np.ones(9), F, hop), want), sig
        assert np.array_equal(want, stft_reference.stft_roundtrip(x, F, hop)), sig


def test_a_curve_outside_the_clamp_equals_the_clamped_one():
    x = LC.SIGNALS["voice"](LC.length(9, 256, 5), 2)
    for out, inside in ((0.3, 0.5), (0.0, 0.5), (-1.0, 0.5), (np.nan, 0.5), (2.7, 2.0), (np.inf, 2.0)):
        assert np.array_equal(FR.lockf_roundtrip(x, out, F, 256), FR.lockf_roundtrip(x, inside, F, 256)), out


@pytest.mark.parametrize("hop", [64, 512])
def test_degenerate_inputs_are_finite_and_silence_is_zero(hop):
    T = LC.length(9, hop, 5)
    for name in LC.DEGENERATE:
        x = pv_cases.degenerate(name, T)
        for cv in ("steps", "outside"):
            r = LC.curve(cv, 9, hop)
            a, b = FR.lockf_roundtrip(x, r, F, hop), FR.lockf_roundtrip_b(x, r, F, hop)
            rel = np.abs(a - b).max() / max(1.0, np.abs(a).max())
            print(f"PVLOCKF degenerate {name} hop{hop} {cv}: forms differ by {rel:.3g} ({'passes' if rel <= FC.GATE_TOL else 'FAILS'} the gate)")
            assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
            if name == "silence":
                assert np.all(a == 0) and np.all(b == 0)
    x, tr = FC.shifted_out(hop, 7), []
    y = FR.lockf_roundtrip(x, 2.0, F, hop, trace=tr)
    assert any(t["gone"] for t in tr) and all(t["gone"] or t["silent"] for t in tr) and np.all(y == 0)


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", FR.MUTANTS)
def test_every_mutant_is_far_from_the_reference_on_a_gated_case(mutant):
    c = FC.TEETH_CASES[mutant]
    assert c in LC.GATE_CASES
    ref, b, mu = FC.gate_reference(c), FC.gate_reference(c, "b"), FC.gate_reference(c, "a", mutant)
    assert np.abs(ref - b).max() <= FC.GATE_TOL * max(1.0, np.abs(ref).max())
    dist = np.abs(ref - mu).max() / FC.bound(c.hop, ref)
    print(f"PVLOCKF mutant {mutant} on {LC.gate_id(c)}: {dist:.3g} GPU bounds from the reference")
    assert dist >= FC.TEETH, dist


# ---- conditioning --------------------------------------------------------------------------------------------------------------------------------
def test_every_item_the_gpu_compares_is_well_conditioned_and_at_most_one_in_eight_is_dropped():
    """The lock family's probe at every (hop, nF, curve, stream) of the GPU one-shot matrix: the items that miss it are exactly DROPPED."""
    missed, worst = set(), (0.0, None)
    for hop in LC.GPU_HOPS:
        for nF in LC.GPU_NF:
            x = LC.gpu_input(hop, nF)
            for name in LC.GPU_CURVES:
                r, ref = LC.gpu_ratios(name, hop, nF), FC.gpu_reference(hop, nF, name)
                for s in range(len(x)):
                    moved = FC.probe(x[s], r[s], hop, ref[s])
                    worst = max(worst, (moved, FC.Item(hop, nF, name, s)))
                    if not moved < FC.CONDITION_SHARE:
                        missed.add(FC.Item(hop, nF, name, s))
    print(f"PVLOCKF conditioning: {len(missed)} of {len(FC.CANDIDATES)} items miss the probe; the worst moves by {worst[0]:.3g} of the bound ({worst[1]})")
    assert missed == set(FC.DROPPED), sorted(missed ^ set(FC.DROPPED))
    assert len(FC.DROPPED) <= FC.MAX_DROPPED_SHARE * len(FC.CANDIDATES)
    assert set(FC.DROPPED) <= set(FC.CANDIDATES)


# ---- quality ------------------------------------------------------------------------------------------------------------------------------------
def test_subbin_offsets_keep_the_level_and_ripple_less_than_the_plain_stage():
    for freq in LC.QUALITY_TONES:
        x = LC.quality_tone(freq)
        for st in LC.QUALITY_SEMITONES:
            r = LC.ratio_of(st)
            rp, ap = LC.ripple(stft_reference.stft_roundtrip(x, F, 256, ratio=r))
            ri, ai = LC.ripple(LR.locked_roundtrip(x, r, F, 256))
            rf, af = LC.ripple(FR.lockf_roundtrip(x, r, F, 256))
            print(f"PVLOCKF quality {freq} Hz {st:+g} st: level plain {ap:.3f} integer {ai:.3f} sub-bin {af:.3f}; ripple plain {rp:.4f} integer {ri:.4f} sub-bin {rf:.4f}")
            assert rf < rp, (freq, st, rf, rp)
            di, df = abs(0.5 - ai), abs(0.5 - af)
            assert df <= di, (freq, st, af, ai)
            if di > 0.05:
                assert df <= 0.25 * di, (freq, st, af, ai)


def test_the_spectral_maximum_lies_at_the_shifted_frequency():
    """The locked stretch test's criterion: the maximum of |sum y e^(-2 pi i f t)| over f, found on a fine grid around f r and refined by
    golden-section search, lies within 1e-3 Hz of f r."""
    for freq in LC.QUALITY_TONES:
        x = LC.quality_tone(freq)
        for st in (7.0, -12.0):
            r = float(LC.ratio_of(st))
            y = FR.lockf_roundtrip(x, r, F, 256)[LC.QUALITY_TRIM:-LC.QUALITY_TRIM]
            n = np.arange(len(y))
            wy = y * np.hanning(len(y))

            def mag(fq):
                return abs(np.dot(wy, np.exp(-2j * np.pi * fq / LC.FS * n)))
            grid = freq * r + np.linspace(-2.0, 2.0, 81)
            k = int(np.argmax([mag(g) for g in grid]))
            lo, hi = grid[max(k - 1, 0)], grid[min(k + 1, len(grid) - 1)]
            g = (np.sqrt(5.0) - 1.0) / 2.0
            for _ in range(60):
                a, b = hi - g * (hi - lo), lo + g * (hi - lo)
                if mag(a) > mag(b):
                    hi = b
                else:
                    lo = a
            peak = 0.5 * (lo + hi)
            print(f"PVLOCKF maximum {freq} Hz {st:+g} st: {peak:.6f} Hz, f r = {freq * r:.6f} Hz")
            assert abs(peak - freq * r) < 1e-3, (freq, st, peak, freq * r)


# ---- streaming ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,N", [(128, 100), (512, 17), (64, 1024)])
def test_block_by_block_is_the_one_shot_delayed_by_the_latency(hop, N):
    nb = max(-(-4 * F // N), 8)
    x = LC.SIGNALS["voice+noise"](N * nb, seed=hop)
    tab = LC.ratio_of(np.random.default_rng([hop, N]).uniform(-13.0, 13.0, nb))
    y = FR.by_block(x, N, hop, tab)
    T = N * nb
    per_frame = LC.per_frame(tab[:, None], N, hop, T)[0]
    y1 = FR.lockf_roundtrip(x, per_frame, F, hop)
    L = pv_cases.latency(N, hop)
    assert L == F - np.gcd(N, hop)
    n = min(len(per_frame) * hop, T - L)
    assert n > F and np.all(y[:L] == 0) and np.array_equal(y[L:L + n], y1[:n])


# ---- the entry points -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_and_null_arguments_fail():
    from vocoderproject_amd import build
    lib = C.CDLL(build.build())
    txt = open(os.path.join(ROOT, "include", "vp_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s + "(" in txt, s
    assert "processBlocksLockedSubbin" in open(os.path.join(ROOT, "include", "vp_amd.hpp")).read()
    assert lib.vp_abi_version() == 3
    one = C.c_void_p(8)                                                               # (a non-null pointer that is never followed)
    lib.vp_stft_pitch_shift_locked_subbin.argtypes = [C.c_void_p] * 5
    lib.vp_pv_process_blocks_locked_subbin_device.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
    assert lib.vp_stft_pitch_shift_locked_subbin(None, one, one, one, None) == -1
    assert lib.vp_pv_process_blocks_locked_subbin_device(None, one, one, one, 1, None) == -1
