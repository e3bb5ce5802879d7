#!/usr/bin/env python3
"""Diagnostic: the formant-preserving phase-vocoder kernels beside the ratio-curve kernels they were copied from.

    [VP_AMD_LIB=...] python tools/pv_formant_bench.py [--reps 7] [--lifter 32] [--out profiles/pv_formant_bench.txt]

One process, the legs alternating (tools/pv_bench.py's windows: every repetition is a window of calls that ends in a device synchronise):
  one-shot, 256 streams x 65 536 samples, 1024 points / hop 256: vp_stft_pitch_shift_curve and vp_stft_pitch_shift_formant on the SAME
  "steps" table (formants preserved, and formants moved per stream);
  streaming, 256 streams, 16 blocks of 1024 per call, hop 256: vp_pv_process_blocks_curve_device and vp_pv_process_blocks_formant_device
  on the same table.
Printed: mean, min and max of the repetitions' rates in frames/s, the formant kernel's mean over the curve kernel's from the same run, and
both kernels' resource listings.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pv_bench import alternate, report, resource_listing  # noqa: E402


def formant_legs(reps, lifter, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, semitones_to_ratios
    S, T, F, hop = 256, 65536, 1024, 256
    rng = np.random.default_rng(9)
    x = torch.randn(S, T, device="cuda", dtype=torch.float32) * 0.1
    y = torch.empty_like(x)
    moved = torch.from_numpy(semitones_to_ratios(rng.uniform(-12.0, 12.0, S))).cuda()
    kept = torch.ones(S, dtype=torch.float64, device="cuda")                 # (device tables in every leg: no upload inside a timed window)
    st = StftRoundTrip(S, T, F, hop)
    nF = st.n_frames
    steps = torch.from_numpy(semitones_to_ratios(rng.uniform(-12.0, 12.0, (S, nF)))).cuda()
    base = "curve, steps (parent kernel)"
    legs = {base: lambda: st.pitch_shift_curve(x, y, d_ratio=steps),
            "formant preserved, steps": lambda: st.pitch_shift_formant(x, y, d_ratio=steps, d_formant=kept, lifter=lifter),
            "formant moved per stream": lambda: st.pitch_shift_formant(x, y, d_ratio=steps, d_formant=moved, lifter=lifter)}
    report(f"one-shot, {S} streams x {T} samples, F = {F}, hop = {hop}, lifter = {lifter}", alternate(legs, reps, 50), S * nF, base, emit)
    st.close()
    N, K = 1024, 16
    ps_c, ps_f = PhaseVocoderStream(S, N, hop=hop), PhaseVocoderStream(S, N, hop=hop)
    xb = torch.randn(K, S, N, device="cuda", dtype=torch.float32) * 0.1
    yb = torch.empty_like(xb)
    steps = torch.from_numpy(semitones_to_ratios(rng.uniform(-12.0, 12.0, (K, S)))).cuda()
    legs = {base: lambda: ps_c.process_device(xb, yb, n_blocks=K, d_ratio=steps),
            "formant preserved, steps": lambda: ps_f.process_device(xb, yb, n_blocks=K, d_ratio=steps, d_formant=kept, lifter=lifter),
            "formant moved per stream": lambda: ps_f.process_device(xb, yb, n_blocks=K, d_ratio=steps, d_formant=moved, lifter=lifter)}
    report(f"streaming, {S} streams, {K} blocks of {N} per call, hop = {hop}, lifter = {lifter}", alternate(legs, reps, 200), S * K * N // hop, base, emit)
    ps_c.close()
    ps_f.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lifter", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    formant_legs(max(5, a.reps), a.lifter, emit)
    resource_listing(emit, ("vp_k_stft_pv_curve", "vp_k_stft_pv_formant", "vp_k_pv_stream_curve", "vp_k_pv_stream_formant"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
