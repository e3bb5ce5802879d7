"""Quality of the peak-locked time stretch against the plain one, on the CPU, from the two NumPy definitions
(tests/pv_stretch_lock_reference.py, tests/pv_stretch_reference.py): envelope ripple (pv_lock_cases.ripple: std / mean of the
analytic-signal magnitude, 2048 samples trimmed at each end), mean amplitude and the spectral maximum of stationary 0.5-amplitude tones at
44.1 kHz, 1024 / 256, under a stretch with a pitch shift on top, and the output rms of a 151 Hz 12-harmonic voice.
tests/test_pv_stretch_lock_reference_cpu.py asserts the ripple inequality and the frequency on the ten pairs it names; the rest is
recorded, not asserted.

    python tools/pv_stretch_lock_quality.py > profiles/pv_stretch_lock_quality.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import pv_lock_cases as LC  # noqa: E402
import pv_stretch_lock_cases as K  # noqa: E402
import pv_stretch_lock_reference as SLR  # noqa: E402
import pv_stretch_reference as SR  # noqa: E402

PAIRS = ((2.0, 7.0), (0.5, -5.0), (0.25, 0.0), (1.5, 0.0), (0.5, 0.0), (4.0, 0.0), (2.0, -12.0), (0.8, 12.0), (1.0, 7.0))


def main():
    print("Peak-locked against plain time stretch, NumPy definitions (tests/pv_stretch_lock_reference.py, tests/pv_stretch_reference.py), CPU.")
    print("0.5-amplitude tones, 44.1 kHz, 1024-point frames, hop 256, %d output samples; ripple = std / mean of the analytic-signal magnitude" % K.QUALITY_T)
    print("with %d samples trimmed at each end, level = its mean, peak = the spectral maximum against tone x ratio." % LC.QUALITY_TRIM)
    print("Written by tools/pv_stretch_lock_quality.py.")
    print()
    print("%-9s %8s %9s %20s %20s %8s %10s" % ("tone Hz", "stretch", "semitones", "plain level/ripple", "locked level/ripple", "ratio", "peak - f r"))
    for freq in K.QUALITY_TONES:
        for a, v in PAIRS:
            x, pos, T = K.quality_setup(freq, a)
            r = K.ratio_of(v)
            rp, ap = LC.ripple(SLR.plain_stretch(x, pos, T, r, K.F, K.QUALITY_HOP))
            yl = SLR.stretch_locked_roundtrip(x, pos, T, r, K.F, K.QUALITY_HOP)
            rl, al = LC.ripple(yl)
            print("%-9.1f %8.2f %+9.2f %12.3f /%6.2f%% %12.3f /%6.2f%% %8.3f %+9.3f Hz" % (freq, a, v, ap, 100 * rp, al, 100 * rl, rl / rp, K.peak_frequency(yl) - freq * r))
    print()
    sl = slice(LC.QUALITY_TRIM, -LC.QUALITY_TRIM)
    rms = lambda y: float(np.sqrt(np.mean(np.asarray(y, np.float64)[sl] ** 2)))        # noqa: E731
    nF = (K.QUALITY_T - K.F) // K.QUALITY_HOP + 1
    print("151 Hz 12-harmonic voice (amplitudes 0.3 / h):")
    for a, v in ((2.0, 7.0), (0.5, -5.0), (0.25, 0.0), (1.5, 0.0)):
        n_in = K.F + int(np.floor((nF - 1) * K.QUALITY_HOP / a)) + 1
        x = LC.voice(n_in, 0, 151.0, 12)
        pos = SR.stretch_positions(nF, K.QUALITY_HOP, a, n_in, K.F).astype(np.int64)
        r = K.ratio_of(v)
        print("  stretch %4.2f, %+6.2f semitones: input rms %.3f, output rms plain %.3f, locked %.3f" % (
            a, v, rms(x), rms(SLR.plain_stretch(x, pos, K.QUALITY_T, r, K.F, K.QUALITY_HOP)),
            rms(SLR.stretch_locked_roundtrip(x, pos, K.QUALITY_T, r, K.F, K.QUALITY_HOP))))
    print()
    print("At stretch 0.25 the analysis advance is a whole frame (D = F): the plain stage's unwrap has no margin left and its output collapses;")
    print("the locked stage turns a peak's region by the peak's own frequency and keeps the tone.  At -12 semitones the integer offset halves")
    print("every peak's bin, as in the locked pitch shift (fractional-bin interpolation of the offset is out of scope).")


if __name__ == "__main__":
    main()
