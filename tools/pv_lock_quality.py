"""Quality of the peak-locked phase-vocoder stage against the plain one, on the CPU, from the two NumPy definitions
(tests/pv_lock_reference.py, tests/stft_reference.py): envelope ripple (std / mean of the analytic-signal magnitude, 2048 samples trimmed
at each end) and mean amplitude of stationary 0.5-amplitude tones at 44.1 kHz, 1024 / 256, and the output rms of a 151 Hz 12-harmonic
voice.  tests/test_pv_lock_reference_cpu.py asserts the ripple inequality; amplitude and rms are recorded, not asserted.

    python tools/pv_lock_quality.py > profiles/pv_lock_quality.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import pv_lock_cases as LC  # noqa: E402
import pv_lock_reference as LR  # noqa: E402
import stft_reference  # noqa: E402


def main():
    print("Peak-locked against plain phase-vocoder stage, NumPy definitions (tests/pv_lock_reference.py, tests/stft_reference.py), CPU.")
    print("0.5-amplitude tones, 44.1 kHz, 1024-point frames, hop 256, %d samples; ripple = std / mean of the analytic-signal magnitude with" % LC.QUALITY_T)
    print("%d samples trimmed at each end, amplitude = its mean.  Written by tools/pv_lock_quality.py." % LC.QUALITY_TRIM)
    print()
    print("%-10s %9s %14s %14s %8s %12s %12s" % ("tone Hz", "semitones", "ripple plain", "ripple locked", "ratio", "amp plain", "amp locked"))
    for freq in LC.QUALITY_TONES:
        x = LC.quality_tone(freq)
        for st in LC.QUALITY_SEMITONES:
            r = LC.ratio_of(st)
            rp, ap = LC.ripple(stft_reference.stft_roundtrip(x, LC.F, 256, ratio=r))
            rl, al = LC.ripple(LR.locked_roundtrip(x, r, LC.F, 256))
            print("%-10.1f %+9.2f %13.2f%% %13.2f%% %8.3f %12.3f %12.3f" % (freq, st, 100 * rp, 100 * rl, rl / rp, ap, al))
    print()
    v = LC.quality_voice()
    sl = slice(LC.QUALITY_TRIM, -LC.QUALITY_TRIM)
    rms = lambda y: float(np.sqrt(np.mean(np.asarray(y, np.float64)[sl] ** 2)))
    print("151 Hz 12-harmonic voice (amplitudes 0.3 / h), input rms %.3f:" % rms(v))
    for st in (7.0, -5.0, 12.0, -12.0):
        r = LC.ratio_of(st)
        print("  %+6.2f semitones: output rms plain %.3f, locked %.3f" % (st, rms(stft_reference.stft_roundtrip(v, LC.F, 256, ratio=r)),
                                                                           rms(LR.locked_roundtrip(v, r, LC.F, 256))))
    print()
    print("At -12 semitones the integer offset halves every peak's bin: the locked stage loses level on the low tone where the plain one keeps")
    print("it (fractional-bin interpolation of the offset is out of scope).")


if __name__ == "__main__":
    main()
