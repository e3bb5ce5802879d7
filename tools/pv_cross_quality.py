"""How far the cross-synthesis moves the carrier's spectral envelope onto the voice's, on the CPU, from the NumPy definition
(tests/pv_cross_reference.py): the rms distance in dB, over the bins up to 8 kHz, between the time-averaged smoothed log envelope
(pv_formant_reference.envelope, lifter 32, averaged over the frames) of the output and of the voice, beside the same distance for the
untouched carrier.  The voice is tests/pv_cross_cases.py's: 12 harmonics of 151 Hz under three formant resonances; the carriers are a 110 Hz
sawtooth and white noise.  44.1 kHz, 1024-point frames, hop 256.  Both envelopes have their mean removed: a level difference is not a
difference of shape.  Recorded, not asserted.

    python tools/pv_cross_quality.py > profiles/pv_cross_quality.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import pv_cross_cases as XC  # noqa: E402
import pv_cross_reference as XR  # noqa: E402
import pv_formant_reference as FR  # noqa: E402
import stft_reference as R  # noqa: E402

F, HOP, NC, T = 1024, 256, 32, 1024 + 160 * 256
TOP = int(8000.0 / XC.FS * F)                         # bins compared: up to 8 kHz
TO_DB = 20.0 / np.log(10.0)


def mean_envelope(x):
    """The smoothed log envelope averaged over the frames of x, in dB, mean removed, bins 0 .. TOP."""
    w = R.window(F)
    nF = (len(x) - F) // HOP + 1
    e = np.mean([FR.envelope(np.abs(np.fft.rfft(x[f * HOP:f * HOP + F] * w)), F, NC) for f in range(2, nF - 2)], axis=0)[:TOP + 1] * TO_DB
    return e - e.mean()


def distance(a, b):
    return float(np.sqrt(np.mean((mean_envelope(a) - mean_envelope(b)) ** 2)))


def main():
    print("Cross-synthesis, NumPy definition (tests/pv_cross_reference.py), CPU: rms distance in dB between the time-averaged spectral envelopes")
    print("(lifter %d, bins up to 8 kHz, means removed) of the output and of the voice, beside the untouched carrier's.  44.1 kHz, %d-point frames," % (NC, F))
    print("hop %d, %d samples; voice: 12 harmonics of 151 Hz under resonances at 700, 1200 and 2600 Hz.  Written by tools/pv_cross_quality.py." % (HOP, T))
    print()
    voice = XC.voice(T).astype(np.float32)
    carriers = (("110 Hz sawtooth", XC.saw(T).astype(np.float32)),
                ("white noise, rms 0.1", (0.1 * np.random.default_rng(5).standard_normal(T)).astype(np.float32)))
    print("%-22s %6s %7s %22s %22s" % ("carrier", "depth", "lifter", "carrier to voice, dB", "output to voice, dB"))
    for name, c in carriers:
        before = distance(c, voice)
        for depth, nc in ((1.0, 32), (0.5, 32), (1.0, 8), (1.0, 64)):
            y = XR.cross_synth(voice, c, F, HOP, depth, nc)
            print("%-22s %6.2f %7d %22.1f %22.1f" % (name, depth, nc, before, distance(y, voice)))
    print()
    print("At depth 1 the output's envelope is the voice's up to what the frames' own harmonics leave in a 32-sample lifter; depth 0.5 about halves the")
    print("distance in dB, as the definition says (the gain is exp(depth (ev - ec))).")


if __name__ == "__main__":
    main()
