"""The conditioning gate of the 2048-point phase-vocoder matrix (tests/pv2k_cases.py), on the CPU: on every case and stream the
restatement's two forms -- tests/stft_reference.py (radians, numpy's functions) and pv_cases.roundtrip_turns (turns, the kernels' form) --
agree to GATE_TOL = 1e-9 of max(1, max |ref|).  A pointwise comparison of the kernel with the restatement means something only on such
inputs (a phase difference on a wrap tie moves a bin's frequency by O bins for good); this test keeps the list honest if someone edits
it.  Measured on this list: worst 1.5e-12."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv2k_cases as K  # noqa: E402


def test_the_list_is_the_product_of_hops_intervals_and_lengths():
    assert len(K.ONE_SHOT_CASES) == 72 and len(set(K.ONE_SHOT_CASES)) == 72
    assert {c.hop for c in K.ONE_SHOT_CASES} == {128, 256, 512, 1024}
    for hop in K.HOPS:
        Ts = sorted({c.T for c in K.ONE_SHOT_CASES if c.hop == hop})
        assert len(Ts) == 6 and Ts[0] == K.F and Ts[1] == K.F + hop - 1
        assert sorted(K.n_frames(T, hop) % 4 for T in Ts[2:]) == [0, 1, 2, 3]
        assert {12.0, -12.0} < {c.semitones for c in K.ONE_SHOT_CASES if c.hop == hop}
    assert max(c.T for c in K.ONE_SHOT_CASES) == 2048 + 18 * 1024 + 3             # (the largest case: 5 x 20.5 K samples)


@pytest.mark.parametrize("hop", K.HOPS)
def test_the_two_forms_of_the_reference_agree_on_every_case(hop):
    worst = 0.0
    for case in (c for c in K.ONE_SHOT_CASES if c.hop == hop):
        x = K.one_shot_input(case)
        assert x.shape == (5, case.T) and x.dtype == np.float32
        a = K.one_shot_reference(case, x, "radians")
        b = K.one_shot_reference(case, x, "turns")
        for s in range(x.shape[0]):
            scale = max(1.0, float(np.abs(a[s]).max()))
            d = float(np.abs(a[s] - b[s]).max()) / scale
            worst = max(worst, d)
            assert d <= K.GATE_TOL, (K.one_shot_id(case), s, d)
    print(f"PV2K gate hop{hop}: worst {worst:.3e} of {K.GATE_TOL:g}")
