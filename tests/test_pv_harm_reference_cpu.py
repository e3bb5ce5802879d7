"""The harmonizer's NumPy definition (tests/pv_harm_reference.py) against the two definitions it is made of, and the teeth of the GPU
test: each named wrong variant lies at least pv_lock_cases.TEETH GPU bounds from the definition on the GPU case chosen to see it
(tests/pv_harm_cases.py), so a kernel that makes that mistake cannot pass tests/test_gpu_pv_harm.py.  No GPU."""
import numpy as np
import pytest

import pv_harm_cases as HC
import pv_harm_reference as HR
import pv_lock_cases as LC
import pv_lock_reference as LR
from stft_reference import stft_roundtrip


def test_one_voice_with_gain_one_and_no_dry_part_is_the_locked_definition():
    for hop, nF, curve in ((256, 8, "steps"), (64, 5, "vibrato"), (512, 7, "outside")):
        x, r = LC.gpu_input(hop, nF), LC.gpu_ratios(curve, hop, nF)
        for s in range(HC.S):
            want = LR.locked_roundtrip(x[s], r[s], HC.F, hop)
            assert np.array_equal(HR.harmonize(x[s], r[s][None], [1.0], 0.0, HC.F, hop), want)
            assert np.array_equal(HR.harmonize(x[s], r[s][None], None, 0.0, HC.F, hop), want)
            assert np.array_equal(HR.harmonize(x[s], r[s][None], None, float("nan"), HC.F, hop), want)      # (a NaN dry value is 0)


def test_no_gain_with_dry_one_is_the_plain_round_trip():
    for hop, nF in ((256, 8), (128, 6)):
        x = LC.gpu_input(hop, nF)
        r = HC.ratios(3, hop, nF)
        for s in range(HC.S):
            want = stft_roundtrip(x[s], HC.F, hop)
            assert np.array_equal(HR.harmonize(x[s], r[s], [0.0, 0.0, 0.0], 1.0, HC.F, hop), want)
            assert np.array_equal(HR.harmonize(x[s], r[s], [float("nan"), float("inf"), -float("inf")], 1.0, HC.F, hop), want)


def test_gains_are_cleaned_as_the_kernels_clean_them():
    got = HR.clean_gain([1.0, -0.5, 4.0, 4.5, -7.0, float("nan"), float("inf"), -float("inf"), 0.0])
    assert np.array_equal(got, [1.0, -0.5, 4.0, 4.0, -4.0, 0.0, 0.0, 0.0, 0.0])


def test_the_cached_parts_give_the_definition():
    """pv_harm_cases.reference builds a case's reference from the locked matrix's cached per-voice references: the same array as the
    definition computed from the input, on every stream, for every voice set."""
    hop, nF = 256, 6
    x = LC.gpu_input(hop, nF)
    for V in HC.VOICE_SETS:
        ref, bnd = HC.reference(V, hop, nF)
        want = HR.harmonize_batch(x, HC.ratios(V, hop, nF), HC.gains(V), HC.DRY, HC.F, hop)
        assert np.array_equal(ref, want), V
        assert np.all(np.isfinite(ref)) and np.all(bnd >= 4.0 * (HC.F // hop) * 2.0 ** -24)


def test_every_voice_set_sees_the_special_gains():
    for V in HC.VOICE_SETS:
        g = HC.gains(V)
        assert g.shape == (HC.S, V)
        assert np.isnan(g).any() and (g == 0.0).any() and (g < 0.0).any() and (g == 4.0).any(), V
        assert len({tuple(np.nan_to_num(r, nan=9.0)) for r in g}) == HC.S                # they differ between streams
    assert set(HC.DRY) == {0.0, 1.0, 0.5}


@pytest.mark.parametrize("mutant", HR.MUTANTS)
def test_each_mutant_lies_beyond_the_gpu_bound_on_its_case(mutant):
    V, hop, nF = HC.TEETH_CASES[mutant]
    x = LC.gpu_input(hop, nF)
    ref, bnd = HC.reference(V, hop, nF)
    bad = HR.harmonize_batch(x, HC.ratios(V, hop, nF), HC.gains(V), HC.DRY, HC.F, hop, mutant)
    dist = np.abs(bad - ref).max(axis=1) / bnd
    print(f"PVHARM teeth {mutant}: distance / bound per stream {np.round(dist, 1)}")
    assert dist.max() >= HC.TEETH, (mutant, dist)
    if mutant == "shared_theta":
        # the streams with partials ("voice", "glide") are the ones that must see it
        for name in ("voice", "glide"):
            assert dist[LC.GPU_STREAMS.index(name)] >= HC.TEETH, (name, dist)


def test_the_streaming_form_is_the_one_shot_delayed():
    """by_block (every voice block by block, the dry part delayed by the latency) equals the definition on the whole signal with the
    blocks' ratios spread to frames, delayed by F - gcd(N, hop); N = 100 at hop 128 is the case the GPU test takes."""
    N, hop = 100, 128
    nb = 30
    x = LC.SIGNALS["voice"](N * nb, seed=5)
    tab = LC.ratio_of(np.random.default_rng(7).uniform(-13.0, 13.0, (nb, 2)))
    y = HR.by_block(x, N, hop, tab, [1.0, -0.5], 0.5)
    L = HC.F - 4
    rf = HC.per_frame(tab[:, None, :], N, hop, len(x))[0]
    one = HR.harmonize(x, rf, [1.0, -0.5], 0.5, HC.F, hop)
    assert np.all(y[:L] == 0.0)
    assert np.abs(y[L:] - one[:len(x) - L]).max() <= 1e-12
