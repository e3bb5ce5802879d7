"""Quality of the peak-locked phase-vocoder stage with sub-bin region offsets against the integer-offset locked stage and the plain one, on
the CPU, from the three NumPy definitions (tests/pv_lockf_reference.py, tests/pv_lock_reference.py, tests/stft_reference.py): mean level
and envelope ripple (mean and std / mean of the analytic-signal magnitude, 2048 samples trimmed at each end) of stationary 0.5-amplitude
tones at 44.1 kHz, 1024 / 256, and the output rms of a 151 Hz 12-harmonic voice.  tests/test_pv_lockf_reference_cpu.py asserts the
inequalities on the ten tone / interval pairs; the voice's rms is recorded, not asserted.

    python tools/pv_lockf_quality.py > profiles/pv_lockf_quality.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import pv_lock_cases as LC  # noqa: E402
import pv_lock_reference as LR  # noqa: E402
import pv_lockf_reference as FR  # noqa: E402
import stft_reference  # noqa: E402


def main():
    print("Sub-bin against integer-offset peak locking and the plain phase-vocoder stage, NumPy definitions (tests/pv_lockf_reference.py,")
    print("tests/pv_lock_reference.py, tests/stft_reference.py), CPU.  0.5-amplitude tones, 44.1 kHz, 1024-point frames, hop 256, %d samples;" % LC.QUALITY_T)
    print("level = mean of the analytic-signal magnitude with %d samples trimmed at each end, ripple = its std / mean." % LC.QUALITY_TRIM)
    print("Written by tools/pv_lockf_quality.py.")
    print()
    print("%-10s %9s | %7s %8s %8s | %8s %8s %8s | %s" % ("tone Hz", "semitones", "level", "", "", "ripple", "", "", "deficit sub-bin / integer"))
    print("%-10s %9s | %7s %8s %8s | %8s %8s %8s |" % ("", "", "plain", "integer", "sub-bin", "plain", "integer", "sub-bin"))
    for freq in LC.QUALITY_TONES:
        x = LC.quality_tone(freq)
        for st in LC.QUALITY_SEMITONES:
            r = LC.ratio_of(st)
            rp, ap = LC.ripple(stft_reference.stft_roundtrip(x, LC.F, 256, ratio=r))
            ri, ai = LC.ripple(LR.locked_roundtrip(x, r, LC.F, 256))
            rf, af = LC.ripple(FR.lockf_roundtrip(x, r, LC.F, 256))
            print("%-10.1f %+9.2f | %7.3f %8.3f %8.3f | %7.2f%% %7.2f%% %7.2f%% | %.3f" % (freq, st, ap, ai, af, 100 * rp, 100 * ri, 100 * rf,
                                                                                          abs(0.5 - af) / abs(0.5 - ai)))
    print()
    v = LC.quality_voice()
    sl = slice(LC.QUALITY_TRIM, -LC.QUALITY_TRIM)
    rms = lambda y: float(np.sqrt(np.mean(np.asarray(y, np.float64)[sl] ** 2)))
    print("151 Hz 12-harmonic voice (amplitudes 0.3 / h), input rms %.3f:" % rms(v))
    for st in (7.0, -5.0, 12.0, -12.0):
        r = LC.ratio_of(st)
        print("  %+6.2f semitones: output rms plain %.3f, integer %.3f, sub-bin %.3f" % (st, rms(stft_reference.stft_roundtrip(v, LC.F, 256, ratio=r)),
                                                                                      rms(LR.locked_roundtrip(v, r, LC.F, 256)), rms(FR.lockf_roundtrip(v, r, LC.F, 256))))
    print()
    print("The sub-bin stage keeps the level the integer offset loses (a region's lobe now sits at the frequency its angle turns at), at a ripple")
    print("that stays below the plain stage's on every pair but is above the integer stage's on most: the six-tap interpolation is not exact.")


if __name__ == "__main__":
    main()
