"""What the transient-preserving stretch does to an attack, measured on the NumPy definitions alone (tests/pv_transient_reference.py,
tests/pv_stretch_lock_reference.py; no GPU):

    python tools/pv_transient_quality.py [--out profiles/pv_transient_quality.txt]

Signals: decaying noise bursts and plucked harmonic notes (tests/pv_transient_cases.py), three onsets 10 987 samples apart and off the
frame grid, 1024-point frames.  For stretch 0.5, 0.75, 1.5, 2 and hops 128, 256, 512, without a pitch shift and with +7 semitones:
  * the onsets the flux rule finds at the default threshold against the true ones (in grid frames, (t - F / 2) / hop);
  * per onset, the relative rms distance of the 600 output samples around it from the input's, and the rms of the 30 ms before it over
    the 14 ms after it (pre-echo), with the scheme and with the locked stretch as it is.  The scheme's attack lands at a known output
    sample; the locked stretch's has no exact landing point, so it gets the best of every lag within a hop of its nominal one.
Then the choice of the default threshold: for each candidate, in how many of the six signals (two kinds, three hops) the rule finds exactly
one onset per attack (within the span's half width max(F / (2 hop), 1) of the true frame: the flux peaks when the attack enters the
window's middle half) and none elsewhere, and the spread of flux / mass at the attacks and at every other local maximum."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pv_transient_cases as TC  # noqa: E402
import pv_transient_reference as TR  # noqa: E402

CANDIDATES = (0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5)


def threshold_table(emit):
    """For the choice of the default: separation of flux / mass between the attacks and every other local maximum, over the six signals."""
    at_onsets, elsewhere = [], []
    exact = {thr: 0 for thr in CANDIDATES}
    cases = [(s, hop) for s in TC.ATTACKS for hop in TC.QUALITY_HOPS]
    for sig, hop in cases:
        x, onsets = TC.quality_input(TC.QualityCase(sig, 1.0, hop))
        flux, mass = TR.onset_flux(x, TC.F, hop)
        true = [(t0 - TC.F // 2) / hop for t0 in onsets]
        tol = float(TR.default_span(TC.F, hop))
        every = np.nonzero(TR.pick_onsets(flux, mass, 0.0))[0]                           # every local maximum above 0
        for g in every:
            share = flux[g] / mass[g]
            (at_onsets if min(abs(g - t) for t in true) <= tol else elsewhere).append(share)
        for thr in CANDIDATES:
            found = np.nonzero(TR.pick_onsets(flux, mass, thr))[0]
            ok = len(found) == len(true) and all(abs(g - t) <= tol for g, t in zip(found, true))
            exact[thr] += int(ok)
    emit(f"flux / mass at the local maxima of the flux, {len(cases)} signals (bursts and plucks at hops 128, 256, 512, three attacks each):")
    emit(f"  at the attacks (within the span):   min {min(at_onsets):.3f}  max {max(at_onsets):.3f}  ({len(at_onsets)} maxima)")
    emit(f"  every other local maximum:          min {min(elsewhere):.3g}  max {max(elsewhere):.3f}  ({len(elsewhere)} maxima)")
    for thr in CANDIDATES:
        emit(f"  thr {thr:<5g} exactly one onset per attack and none elsewhere in {exact[thr]} of {len(cases)} signals")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("transient-preserving locked time stretch on the NumPy definitions (tools/pv_transient_quality.py): 1024-point frames, "
         f"threshold {TC.THR}, span max(F / (2 hop), 1)")
    emit("distance: relative rms distance of the 600 output samples around the attack from the input's; pre/post: rms of the 30 ms before the attack over the 14 ms after")
    for semis in (0.0, 7.0):
        emit("")
        emit(f"pitch shift {semis:+g} semitones" + ("" if semis == 0 else " on top (only the positions help here: the frames of a span are still rotated apart)"))
        emit(f"  {'case':<22s} {'onsets found (true)':<44s} {'distance: scheme':>34s} {'locked today':>28s} {'pre/post: scheme':>30s} {'locked today':>26s}")
        for c in TC.QUALITY_CASES:
            q = TC.quality(c, semis)
            rows = q["rows"]
            found = " ".join(str(g) for g in q["found"]) + " (" + " ".join(f"{t:.1f}" for t in q["true"]) + ")"

            def span(key, fmt):
                v = [r[key] for r in rows]
                return f"{format(min(v), fmt)} .. {format(max(v), fmt)}"
            emit(f"  {TC.quality_id(c):<22s} {found:<44s} {span('new', '.3g'):>34s} {span('old', '.3g'):>28s} {span('new_pre', '.3g'):>30s} {span('old_pre', '.3g'):>26s}"
                 + ("" if all(r["accepted"] for r in rows) else "   (an attack without a span)"))
    emit("")
    threshold_table(emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
