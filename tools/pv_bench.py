#!/usr/bin/env python3
"""Diagnostic: the phase-vocoder stage (vp_stft_pitch_shift) at the bench's shape, a few intervals.

    [VP_AMD_LIB=...] python tools/pv_bench.py
    [VP_AMD_LIB=...] python tools/pv_bench.py --curve [--reps 7] [--out profiles/pv_curve_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --stretch [--reps 7] [--out profiles/pv_stretch_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --track [--reps 7] [--out profiles/pv_track_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --track-stream [--reps 7] [--out profiles/pv_track_stream_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --locked [--reps 7] [--out profiles/pv_lock_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --stretch-locked [--reps 7] [--out profiles/pv_stretch_lock_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --transient [--reps 7] [--out profiles/pv_transient_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --locked-subbin [--reps 7] [--out profiles/pv_lockf_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --cross [--reps 7] [--out profiles/pv_cross_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --harm [--reps 7] [--out profiles/pv_harm_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --harmkey [--reps 7] [--out profiles/pv_harmkey_bench.txt]
    [VP_AMD_LIB=...] python tools/pv_bench.py --track-fine [--reps 7] [--out profiles/pv_track_fine_bench.txt]

--curve: the ratio-curve builds against their fixed-interval parents, in ONE process with the legs alternating (fixed, constant curve,
"steps" curve, fixed, ...): 256 streams x 65 536 samples at 1024 points / hop 256 and 2048 points / hop 512 (vp_stft_pitch_shift against
vp_stft_pitch_shift_curve), then streaming, 16 blocks of 1024 per call, plain against curve.  Every repetition is a window of calls that
ends in a device synchronise; mean, min and max of the repetitions' rates are printed, and the constant curve's mean over the fixed
interval's from the same run.

--stretch: the time-stretch builds (vp_stft_time_stretch) beside their fixed-grid parents, in the same process and the same alternation:
256 streams, 65 536 output samples, 1024 points / hop 256 and 2048 points / hop 512; the parent at +7 semitones, then the stretch kernel at
+7 with the tables of stretch 1 (the identity table f hop: the parent's work), 0.5 and 2.  The identity table's mean over the parent's
from the same run is the comparison; the kernels' resource listings follow.

--track: the pitch tracker (vp_stft_track_pitch, kernel vp_k_yin_track), vp_stft_pitch_shift_curve alone on the tracker's table and
vp_stft_autotune (the two on one stream), alternating in one process: 256 streams x 65 536 samples of voiced signals (a harmonic tone with
vibrato per stream, every fourth stream noise) at 44.1 kHz, 1024 points / hop 256 and 2048 points / hop 512.  Printed: each leg's frames/s,
the tracker's beside the curve kernel's, and autotune's time per call against the sum of its parts'.

--track-stream: the streaming tracker (vp_pv_tracker_process_blocks_device, kernels vp_k_yin_track_stream and vp_k_track_follow) beside the
batch tracker, alternating in one process: 256 streams at 44.1 kHz, 1024 points, the same signals.  The batch tracker runs at --track's shape
(65 536 samples, hop 256: the yardstick) and at the streaming call's number of decisions (16 frames per stream, hop 512); the streaming
tracker takes 16 blocks of 1024 per call and, as its own line, one block per call.  Then the streaming autotune
(vp_pv_autotune_blocks_device) against the tracker call and the curve call that make it up.  Every repetition is a window of about a tenth of a second of calls.  Printed: decisions/s per leg and autotune's
time per call against the sum of its parts'.

--locked: the peak-locked builds (vp_stft_pitch_shift_locked, vp_pv_process_blocks_locked_device) beside the curve kernels they were
copied from, alternating in one process on the SAME "steps" table: one-shot, 256 streams x 65 536 samples, 1024 points / hop 256, on noise
and on voiced signals (the stage's mask searches depend on how far apart the peaks are); then streaming, 16 blocks of 1024 per call.  The
locked kernel's mean over the curve kernel's from the same run is the comparison; the kernels' resource listings follow.

--locked-subbin: the peak-locked builds with sub-bin region offsets (vp_stft_pitch_shift_locked_subbin,
vp_pv_process_blocks_locked_subbin_device) beside the integer-offset locked kernels they were copied from, alternating in one process on the
SAME "steps" table: one-shot, 256 streams x 65 536 samples, 1024 points / hop 256, on noise and on voiced signals; then streaming, 16 blocks
of 1024 per call, on both.  The sub-bin kernel's mean over the integer kernel's from the same run is the comparison; the kernels' resource
listings follow.

--stretch-locked: the locked time stretch (vp_stft_time_stretch_locked) beside both of its parents, alternating in one process: 256
streams, 65 536 output samples, 1024 points / hop 256, on noise and on voiced signals, every call at +7 semitones.  The locked pitch shift
(vp_k_stft_pv_lock) and the new kernel at the identity table f hop on the same input: the ratio is the cost of the positions alone.  Then
the plain time stretch (vp_k_stft_pv_stretch) and the new kernel at stretch 0.5 and 2, each pair on the same input and table.  The kernels'
resource listings follow.

--transient: the transient-preserving stretch's two kernels, alternating in one process: 256 streams x 65 536 samples, 1024 points /
hop 256, on noise and on voiced signals.  The onset flux (vp_stft_onset_flux) alone, in input frames per second; the reset kernel
(vp_stft_time_stretch_locked_reset) on an ALL-ZERO table beside vp_stft_time_stretch_locked on the same input, ratio table (+7) and
positions f hop: the ratio is the cost of the flag byte and the turn's select.  The kernels' resource listings follow.

--cross: the cross-synthesis (vp_stft_cross_synth, vp_xs_process_blocks_device) beside the kernels it is made of, alternating in one
process: 256 streams x 65 536 samples, 1024 points / hop 256, voiced voices over sawtooth carriers.  The plain double-precision round trip
of the carrier (two transforms per frame), the formant kernel on the voice (four, and the phase-vocoder stage), the cross-synthesis (seven),
and the streaming cross-synthesis, 16 blocks of 1024 per call.  The cross-synthesis's mean over the round trip's and over the formant
kernel's from the same run are the comparisons; the kernels' resource listings follow.

--harm: the harmonizer (vp_stft_harmonize, vp_hz_process_blocks_device) beside the composition it replaces, alternating in one process:
256 streams x 65 536 samples, 1024 points / hop 256, three voices (+4, +7, -5 semitones) plus the dry signal, on noise and on voiced input.
The legs: the harmonizer; three vp_stft_pitch_shift_locked calls, one double-precision vp_stft_roundtrip and the mix as one fused torch
expression on the device (a matrix-vector product over the stacked parts: one read of each, one write); one locked call alone.  Rates are input frames per second (a frame counts once however many voices it gets).
Streaming, 16 blocks of 1024 per call: the streaming harmonizer against three locked streaming handles plus the mix (the composition's dry
part is the undelayed input there: a caller's delay line is not timed).  The kernels' resource listings follow.

--harmkey: the key-aware voices (vp_stft_track_harmony, vp_stft_harmonize_key, vp_hz_autoharm_blocks_device) beside their parts and
beside the composition a caller had before them, alternating in one process: 256 streams x 65 536 samples at 44.1 kHz, 1024 points /
hop 256, three voices at degrees (2, 4, -3) of keys 0 .. 12 in turn, on voiced signals and on noise.  One-shot legs: vp_stft_track_pitch;
vp_stft_track_harmony at V = 3 (the ratio over the tracker is the voice stage's cost); vp_stft_harmonize along that table;
vp_stft_harmonize_key (against the sum of its two calls); three autotune(locked=True) calls and the mix (the composition: parallel
harmony from three trackers).  Streaming, 16 blocks of 1024 per call: vp_hz_autoharm_blocks_device against the tracker's voices call
plus the harmonizer call on handles of their own.  Every table a leg takes is on the device before the clock starts.

--track-fine: the fine trackers (VP_TRACK_FINE) beside the integer ones, alternating in one process on one handle whose mode is switched
between the legs: vp_stft_track_pitch at 256 streams x 65 536 samples, 1024 points / hop 256 (kernels vp_k_yin_track and
vp_k_yin_track_fine), and vp_pv_tracker_process_blocks_device at 16 blocks of 1024 per call with full windows.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fixed_intervals():
    import torch
    from vocoderproject_amd import StftRoundTrip
    S, T, F, hop = 256, 65536, 1024, 256
    x = torch.randn(S, T, device="cuda", dtype=torch.float32) * 0.1
    y = torch.empty_like(x)
    st = StftRoundTrip(S, T, F, hop)
    frames = S * ((T - F) // hop + 1)
    for semis in (7.0, 12.0, -5.0):
        for _ in range(3):
            st.pitch_shift(x, y, semis)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 20
        for _ in range(n):
            st.pitch_shift(x, y, semis)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        print(f"{semis:+5.1f} semitones: {frames / dt / 1e6:7.1f} M frames/s  {dt * 1e6:8.1f} us per call")
    st.close()


def alternate(legs, reps, calls, warmup=3):
    """legs: {name: callable enqueueing one call}.  Returns {name: [seconds per call, one per repetition]}, the legs taking turns.
    calls: calls per repetition, one number or one per leg ({name: n}: short calls need more of them to fill a window)."""
    import torch
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = calls[name] if isinstance(calls, dict) else calls
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / n)
    return out


def report(title, times, frames, base, emit):
    emit(title)
    rate = {k: [frames / t / 1e6 for t in v] for k, v in times.items()}
    for k, r in rate.items():
        mean = sum(r) / len(r)
        emit(f"  {k:<28s} {mean:8.1f} M frames/s  (min {min(r):.1f}, max {max(r):.1f}, {len(r)} repetitions)"
             + ("" if k == base else f"  {mean / (sum(rate[base]) / len(rate[base])):.3f} x {base}"))


def curve_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, semitones_to_ratios
    S, T = 256, 65536
    rng = np.random.default_rng(9)
    x = torch.randn(S, T, device="cuda", dtype=torch.float32) * 0.1
    y = torch.empty_like(x)
    for F, hop in ((1024, 256), (2048, 512)):
        st = StftRoundTrip(S, T, F, hop)
        nF = st.n_frames
        const = torch.from_numpy(np.full((S, nF), semitones_to_ratios([7.0])[0])).cuda()
        steps = torch.from_numpy(semitones_to_ratios(rng.uniform(-12.0, 12.0, (S, nF)))).cuda()
        legs = {"fixed +7 (parent kernel)": lambda: st.pitch_shift(x, y, 7.0),
                "curve, constant +7": lambda: st.pitch_shift_curve(x, y, d_ratio=const),
                "curve, steps": lambda: st.pitch_shift_curve(x, y, d_ratio=steps)}
        report(f"one-shot, {S} streams x {T} samples, F = {F}, hop = {hop}", alternate(legs, reps, 100), S * nF, "fixed +7 (parent kernel)", emit)
        st.close()
    N, K, hop = 1024, 16, 256
    ps = PhaseVocoderStream(S, N, hop=hop)
    ps.set_semitones(7.0)
    xb = torch.randn(K, S, N, device="cuda", dtype=torch.float32) * 0.1
    yb = torch.empty_like(xb)
    const = torch.from_numpy(np.full((K, S), semitones_to_ratios([7.0])[0])).cuda()
    steps = torch.from_numpy(semitones_to_ratios(rng.uniform(-12.0, 12.0, (K, S)))).cuda()
    legs = {"plain +7 (parent kernel)": lambda: ps.process_device(xb, yb, n_blocks=K),
            "curve, constant +7": lambda: ps.process_device(xb, yb, n_blocks=K, d_ratio=const),
            "curve, steps": lambda: ps.process_device(xb, yb, n_blocks=K, d_ratio=steps)}
    report(f"streaming, {S} streams, {K} blocks of {N} per call, hop = {hop}", alternate(legs, reps, 300), S * K * N // hop, "plain +7 (parent kernel)", emit)
    ps.close()


def locked_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, semitones_to_ratios
    S, T, F, hop, fs = 256, 65536, 1024, 256, 44100.0
    rng = np.random.default_rng(9)
    st = StftRoundTrip(S, T, F, hop)
    nF = st.n_frames
    steps = torch.from_numpy(semitones_to_ratios(rng.uniform(-12.0, 12.0, (S, nF)))).cuda()
    base = "curve, steps (parent kernel)"
    for what, x in (("noise", torch.randn(S, T, device="cuda", dtype=torch.float32) * 0.1), ("voiced signals", torch.from_numpy(voiced_rows(S, T, fs)).cuda())):
        y = torch.empty_like(x)
        legs = {base: lambda x=x, y=y: st.pitch_shift_curve(x, y, d_ratio=steps),
                "locked, steps": lambda x=x, y=y: st.pitch_shift_locked(x, y, d_ratio=steps)}
        report(f"one-shot, {S} streams x {T} samples of {what}, F = {F}, hop = {hop}", alternate(legs, reps, 100), S * nF, base, emit)
    st.close()
    N, K = 1024, 16
    a, b = PhaseVocoderStream(S, N, hop=hop), PhaseVocoderStream(S, N, hop=hop)
    xb = torch.randn(K, S, N, device="cuda", dtype=torch.float32) * 0.1
    yb = torch.empty_like(xb)
    steps = torch.from_numpy(semitones_to_ratios(rng.uniform(-12.0, 12.0, (K, S)))).cuda()
    legs = {base: lambda: a.process_device(xb, yb, n_blocks=K, d_ratio=steps),
            "locked, steps": lambda: b.process_device(xb, yb, n_blocks=K, d_ratio=steps, locked=True)}
    report(f"streaming, {S} streams, {K} blocks of {N} per call of noise, hop = {hop}", alternate(legs, reps, 300), S * K * N // hop, base, emit)
    a.close()
    b.close()


def locked_subbin_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, semitones_to_ratios
    S, T, F, hop, fs = 256, 65536, 1024, 256, 44100.0
    rng = np.random.default_rng(9)
    st = StftRoundTrip(S, T, F, hop)
    nF = st.n_frames
    steps = torch.from_numpy(semitones_to_ratios(rng.uniform(-12.0, 12.0, (S, nF)))).cuda()
    base, new = "locked, steps (parent kernel)", "locked sub-bin, steps"
    inputs = (("noise", torch.randn(S, T, device="cuda", dtype=torch.float32) * 0.1), ("voiced signals", torch.from_numpy(voiced_rows(S, T, fs)).cuda()))
    for what, x in inputs:
        y = torch.empty_like(x)
        legs = {base: lambda x=x, y=y: st.pitch_shift_locked(x, y, d_ratio=steps),
                new: lambda x=x, y=y: st.pitch_shift_locked(x, y, d_ratio=steps, subbin=True)}
        report(f"one-shot, {S} streams x {T} samples of {what}, F = {F}, hop = {hop}", alternate(legs, reps, 100), S * nF, base, emit)
    st.close()
    N, K = 1024, 16
    a, b = PhaseVocoderStream(S, N, hop=hop), PhaseVocoderStream(S, N, hop=hop)
    steps = torch.from_numpy(semitones_to_ratios(rng.uniform(-12.0, 12.0, (K, S)))).cuda()
    for what, x in inputs:
        xb = x[:, :K * N].reshape(S, K, N).transpose(0, 1).contiguous()
        yb = torch.empty_like(xb)
        legs = {base: lambda xb=xb, yb=yb: a.process_device(xb, yb, n_blocks=K, d_ratio=steps, locked=True),
                new: lambda xb=xb, yb=yb: b.process_device(xb, yb, n_blocks=K, d_ratio=steps, locked=True, subbin=True)}
        report(f"streaming, {S} streams, {K} blocks of {N} per call of {what}, hop = {hop}", alternate(legs, reps, 300), S * K * N // hop, base, emit)
    a.close()
    b.close()


def stretch_locked_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios, stretch_positions
    S, T, F, hop, fs = 256, 65536, 1024, 256, 44100.0
    st = StftRoundTrip(S, T, F, hop)
    nF = st.n_frames
    y = torch.empty(S, T, device="cuda", dtype=torch.float32)
    ratio = torch.from_numpy(np.full((S, nF), semitones_to_ratios([7.0])[0])).cuda()
    parent = "locked +7 (parent kernel)"
    n_max = int(T / 0.5) + F
    for what, rows in (("noise", torch.randn(S, n_max, device="cuda", dtype=torch.float32) * 0.1), ("voiced signals", torch.from_numpy(voiced_rows(S, n_max, fs)).cuda())):
        legs = {}
        for a in (1.0, 0.5, 2.0):
            n_in = T if a == 1.0 else int(T / a) + F                        # (stretch 1: the parent's input, row for row)
            x = rows[:, :n_in].contiguous()
            pos = torch.from_numpy(np.tile(stretch_positions(nF, hop, a, n_in, F), (S, 1))).cuda()
            if a == 1.0:
                assert np.array_equal(pos[0].cpu().numpy(), np.arange(nF) * hop)
                legs[parent] = lambda x=x: st.pitch_shift_locked(x, y, d_ratio=ratio)
                legs["stretch locked 1, +7 (identity table)"] = lambda x=x, pos=pos: st.time_stretch_locked(x, y, d_pos=pos, d_ratio=ratio)
            else:
                legs[f"plain stretch {a:g}, +7"] = lambda x=x, pos=pos: st.time_stretch(x, y, d_pos=pos, semitones=7.0)
                legs[f"stretch locked {a:g}, +7"] = lambda x=x, pos=pos: st.time_stretch_locked(x, y, d_pos=pos, d_ratio=ratio)
        times = alternate(legs, reps, 100)
        report(f"locked time stretch, {S} streams x {T} output samples of {what}, F = {F}, hop = {hop}", times, S * nF, parent, emit)
        mean = {k: sum(v) / len(v) for k, v in times.items()}
        for a in (0.5, 2.0):
            emit(f"  stretch locked {a:g} = {mean[f'plain stretch {a:g}, +7'] / mean[f'stretch locked {a:g}, +7']:.3f} x plain stretch {a:g} (frames/s, the same run)")
    st.close()


def transient_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import StftRoundTrip, semitones_to_ratios
    S, T, F, hop, fs = 256, 65536, 1024, 256, 44100.0
    st = StftRoundTrip(S, T, F, hop)
    nF = st.n_frames
    y = torch.empty(S, T, device="cuda", dtype=torch.float32)
    ratio = torch.from_numpy(np.full((S, nF), semitones_to_ratios([7.0])[0])).cuda()
    pos = torch.from_numpy(np.tile(np.arange(nF, dtype=np.int32) * hop, (S, 1))).cuda()
    zero = torch.zeros((S, nF), dtype=torch.uint8, device="cuda")
    flux, mass = torch.empty((S, nF), dtype=torch.float64, device="cuda"), torch.empty((S, nF), dtype=torch.float64, device="cuda")
    parent, new, fl = "stretch locked, +7 (parent kernel)", "stretch locked reset, all-zero table", "onset flux"
    for what, x in (("noise", torch.randn(S, T, device="cuda", dtype=torch.float32) * 0.1), ("voiced signals", torch.from_numpy(voiced_rows(S, T, fs)).cuda())):
        legs = {parent: lambda x=x: st.time_stretch_locked(x, y, d_pos=pos, d_ratio=ratio),
                new: lambda x=x: st.time_stretch_locked(x, y, d_pos=pos, d_ratio=ratio, d_reset=zero),
                fl: lambda x=x: st.onset_flux(x, flux, mass)}
        report(f"transient-preserving stretch, {S} streams x {T} samples of {what}, F = {F}, hop = {hop} (n_in = T: {nF} frames per stream in every leg)",
               alternate(legs, reps, {parent: 100, new: 100, fl: 400}), S * nF, parent, emit)
    st.close()


def stretch_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import StftRoundTrip, stretch_positions
    S, T = 256, 65536
    parent = "fixed +7 (parent kernel)"
    for F, hop in ((1024, 256), (2048, 512)):
        st = StftRoundTrip(S, T, F, hop)
        nF = st.n_frames
        y = torch.empty(S, T, device="cuda", dtype=torch.float32)
        legs = {}
        for a in (1.0, 0.5, 2.0):
            n_in = T if a == 1.0 else int(T / a) + F                        # (stretch 1: the parent's input, row for row)
            x = torch.randn(S, n_in, device="cuda", dtype=torch.float32) * 0.1
            pos = torch.from_numpy(np.tile(stretch_positions(nF, hop, a, n_in, F), (S, 1))).cuda()
            if a == 1.0:
                assert np.array_equal(pos[0].cpu().numpy(), np.arange(nF) * hop)
                legs[parent] = lambda x=x: st.pitch_shift(x, y, 7.0)
            legs[f"stretch {a:g}, +7" + (" (identity table)" if a == 1.0 else "")] = lambda x=x, pos=pos: st.time_stretch(x, y, d_pos=pos, semitones=7.0)
        report(f"time stretch, {S} streams x {T} output samples, F = {F}, hop = {hop}", alternate(legs, reps, 100), S * nF, parent, emit)
        st.close()


def track_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import StftRoundTrip
    S, T, fs = 256, 65536, 44100.0
    x = torch.from_numpy(voiced_rows(S, T, fs)).cuda()
    y = torch.empty_like(x)
    keys = torch.from_numpy((np.arange(S) % 13).astype(np.int32)).cuda()
    for F, hop in ((1024, 256), (2048, 512)):
        st = StftRoundTrip(S, T, F, hop)
        nF = st.n_frames
        period, table = st.track_pitch(x, fs, keys=keys)
        torch.cuda.synchronize()
        voiced = float((period > 0).float().mean())
        legs = {"tracker": lambda: st.track_pitch(x, fs, keys=keys),
                "curve on the tracker's table": lambda: st.pitch_shift_curve(x, y, d_ratio=table),
                "autotune": lambda: st.autotune(x, y, fs, keys=keys)}
        times = alternate(legs, reps, 20)
        report(f"pitch tracker, {S} streams x {T} samples at {fs:g} Hz, F = {F}, hop = {hop}, {100.0 * voiced:.0f} % of the frames voiced",
               times, S * nF, "curve on the tracker's table", emit)
        mean = {k: sum(v) / len(v) for k, v in times.items()}
        curve = mean["curve on the tracker's table"]
        parts = mean["tracker"] + curve
        emit(f"  per call: tracker {mean['tracker'] * 1e3:.3f} ms + curve {curve * 1e3:.3f} ms = {parts * 1e3:.3f} ms; "
             f"autotune {mean['autotune'] * 1e3:.3f} ms = {mean['autotune'] / parts:.3f} x the sum")
        st.close()


def voiced_rows(S, T, fs, seed=11):
    """--track's signals: a harmonic tone with vibrato per stream, every fourth stream noise; float32 [S][T]."""
    import numpy as np
    rng = np.random.default_rng(seed)
    t = np.arange(T) / fs
    rows = []
    for s in range(S):
        if s % 4 == 3:
            rows.append(0.1 * rng.standard_normal(T))
            continue
        f0 = rng.uniform(110.0, 440.0) * 2.0 ** (0.3 / 12.0 * np.sin(2.0 * np.pi * rng.uniform(3.0, 7.0) * t))
        ph = 2.0 * np.pi * np.cumsum(f0) / fs
        rows.append(0.3 * np.sin(ph) + 0.15 * np.sin(2.0 * ph + 1.0) + 0.08 * np.sin(3.0 * ph + 2.0))
    return np.stack(rows).astype(np.float32)


def track_stream_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, StreamingPitchTracker
    S, T, fs, F, N, K = 256, 65536, 44100.0, 1024, 1024, 16
    rows = voiced_rows(S, T, fs)
    x = torch.from_numpy(rows).cuda()
    keys = torch.from_numpy((np.arange(S) % 13).astype(np.int32)).cuda()
    # the batch tracker: the yardstick's shape, and the streaming call's number of decisions (K frames per stream)
    st = StftRoundTrip(S, T, F, 256)
    Tk = F + (K - 1) * 512 + 441
    stk = StftRoundTrip(S, Tk, F, 512)
    xk = x[:, :Tk].contiguous()
    assert stk.n_frames == K
    # the streaming tracker: two blocks of history first (W = 1465 samples), then every decision has a full window
    blocks = torch.from_numpy(np.ascontiguousarray(rows[:, :(K + 2) * N].reshape(S, K + 2, N).transpose(1, 0, 2))).cuda()
    trk, trk1 = StreamingPitchTracker(S, N, fs, F), StreamingPitchTracker(S, N, fs, F)
    for t in (trk, trk1):
        t.process_device(blocks[:2], n_blocks=2, keys=keys)
    slab, one = blocks[2:].contiguous(), blocks[2:3].contiguous()
    period, _ = trk.process_device(slab, n_blocks=K, keys=keys)
    torch.cuda.synchronize()
    voiced = float((period > 0).float().mean())
    legs = {"batch, 65 536 samples, hop 256": lambda: st.track_pitch(x, fs, keys=keys),
            f"batch, {K} frames per stream": lambda: stk.track_pitch(xk, fs, keys=keys),
            f"streaming, {K} blocks per call": lambda: trk.process_device(slab, n_blocks=K, keys=keys),
            "streaming, 1 block per call": lambda: trk1.process_device(one, n_blocks=1, keys=keys)}
    decisions = {"batch, 65 536 samples, hop 256": S * st.n_frames, f"batch, {K} frames per stream": S * K, f"streaming, {K} blocks per call": S * K,
                 "streaming, 1 block per call": S}
    calls = dict(zip(legs, (40, 500, 500, 2000)))                            # (windows of about a tenth of a second each)
    times = alternate(legs, reps, calls)
    emit(f"streaming pitch tracker, {S} streams at {fs:g} Hz, F = {F}, blocks of {N}, {100.0 * voiced:.0f} % of the decisions voiced")
    rate = {k: [decisions[k] / t / 1e6 for t in v] for k, v in times.items()}
    mean = {k: sum(r) / len(r) for k, r in rate.items()}
    for k, r in rate.items():
        emit(f"  {k:<32s} {mean[k]:8.2f} M decisions/s  (min {min(r):.2f}, max {max(r):.2f}, {len(r)} repetitions)  "
             f"{sum(times[k]) / len(times[k]) * 1e6:8.1f} us per call")
    emit(f"  streaming, {K} blocks per call = {mean[f'streaming, {K} blocks per call'] / mean['batch, 65 536 samples, hop 256']:.3f} x the batch tracker at its "
         f"bench shape, {mean[f'streaming, {K} blocks per call'] / mean[f'batch, {K} frames per stream']:.3f} x the batch tracker at {K} frames per stream")
    for h in (st, stk, trk, trk1):
        h.close()
    # autotune against its parts: separate handle pairs, the same slab
    y = torch.empty_like(slab)
    pv_a, pv_b, trk_a, trk_b = PhaseVocoderStream(S, N), PhaseVocoderStream(S, N), StreamingPitchTracker(S, N, fs, F), StreamingPitchTracker(S, N, fs, F)
    for t in (trk_a, trk_b):
        t.process_device(blocks[:2], n_blocks=2, keys=keys)
    _, table = trk_a.process_device(slab, n_blocks=K, keys=keys)
    legs = {"tracker": lambda: trk_a.process_device(slab, n_blocks=K, keys=keys),
            "curve on the tracker's table": lambda: pv_a.process_device(slab, y, n_blocks=K, d_ratio=table),
            "autotune": lambda: pv_b.autotune_device(trk_b, slab, y, n_blocks=K, keys=keys)}
    times = alternate(legs, reps, 300)
    m = {k: sum(v) / len(v) for k, v in times.items()}
    parts = m["tracker"] + m["curve on the tracker's table"]
    emit(f"streaming autotune, {S} streams, {K} blocks of {N} per call, hop = 256")
    emit(f"  per call: tracker {m['tracker'] * 1e3:.3f} ms + curve {m['curve on the tracker' + chr(39) + 's table'] * 1e3:.3f} ms = {parts * 1e3:.3f} ms; "
         f"autotune {m['autotune'] * 1e3:.3f} ms = {m['autotune'] / parts:.3f} x the sum")
    for h in (pv_a, pv_b, trk_a, trk_b):
        h.close()


def track_fine_legs(reps, emit):
    """The fine trackers beside the integer ones, the mode switched on one handle between the legs (the switch is a host-side store)."""
    import numpy as np
    import torch
    from vocoderproject_amd import StftRoundTrip, StreamingPitchTracker
    S, T, fs, F, hop, N, K = 256, 65536, 44100.0, 1024, 256, 1024, 16
    rows = voiced_rows(S, T, fs)
    x = torch.from_numpy(rows).cuda()
    keys = torch.from_numpy((np.arange(S) % 13).astype(np.int32)).cuda()
    st = StftRoundTrip(S, T, F, hop)
    period, _ = st.track_pitch(x, fs, keys=keys)
    torch.cuda.synchronize()
    voiced = float((period > 0).float().mean())

    def batch(fine):
        st.set_track_mode(fine)
        st.track_pitch(x, fs, keys=keys)
    times = alternate({"vp_k_yin_track": lambda: batch(False), "vp_k_yin_track_fine": lambda: batch(True)}, reps, 20)
    report(f"fine pitch tracker, {S} streams x {T} samples at {fs:g} Hz, F = {F}, hop = {hop}, {100.0 * voiced:.0f} % of the frames voiced",
           times, S * st.n_frames, "vp_k_yin_track", emit)
    m = {k: sum(v) / len(v) for k, v in times.items()}
    emit(f"  per call: integer {m['vp_k_yin_track'] * 1e3:.3f} ms, fine {m['vp_k_yin_track_fine'] * 1e3:.3f} ms; fine / integer, frames per second: "
         f"{m['vp_k_yin_track'] / m['vp_k_yin_track_fine']:.3f}")
    st.close()
    blocks = torch.from_numpy(np.ascontiguousarray(rows[:, :(K + 2) * N].reshape(S, K + 2, N).transpose(1, 0, 2))).cuda()
    trk = StreamingPitchTracker(S, N, fs, F)
    trk.process_device(blocks[:2], n_blocks=2, keys=keys)                    # two blocks of history: every decision has a full window
    slab = blocks[2:].contiguous()

    def stream(fine):
        trk.set_fine(fine)
        trk.process_device(slab, n_blocks=K, keys=keys)
    times = alternate({"integer": lambda: stream(False), "fine": lambda: stream(True)}, reps, 500)
    m = {k: sum(v) / len(v) for k, v in times.items()}
    emit(f"streaming fine tracker, {S} streams, {K} blocks of {N} per call (tracker and follow kernel)")
    for k, v in times.items():
        r = [S * K / t / 1e6 for t in v]
        emit(f"  {k:<28s} {sum(r) / len(r):8.2f} M decisions/s  (min {min(r):.2f}, max {max(r):.2f}, {len(r)} repetitions)  {m[k] * 1e6:8.1f} us per call")
    emit(f"  fine / integer, decisions per second: {m['integer'] / m['fine']:.3f}")
    trk.close()


def saw_rows(S, T, fs, seed=12):
    """--cross's carriers: one sawtooth per stream, 55 .. 220 Hz; float32 [S][T]."""
    import numpy as np
    rng = np.random.default_rng(seed)
    ph = np.arange(T)[None, :] * (rng.uniform(55.0, 220.0, (S, 1)) / fs)
    return (0.4 * (2.0 * (ph - np.floor(ph)) - 1.0)).astype(np.float32)


def cross_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import CrossSynthStream, StftRoundTrip
    S, T, F, hop, fs = 256, 65536, 1024, 256, 44100.0
    v = torch.from_numpy(voiced_rows(S, T, fs)).cuda()
    c = torch.from_numpy(saw_rows(S, T, fs)).cuda()
    y = torch.empty_like(c)
    st = StftRoundTrip(S, T, F, hop)
    nF = st.n_frames
    ones = torch.from_numpy(np.ones((S, nF))).cuda()
    depth = torch.from_numpy(np.ones(S)).cuda()
    base = "round trip of the carrier, f64"
    legs = {base: lambda: st(c, y),
            "formant kernel, ratio 1": lambda: st.pitch_shift_formant(v, y, d_ratio=ones, d_formant=depth),
            "cross-synthesis": lambda: st.cross_synth(v, c, y, d_depth=depth)}
    times = alternate(legs, reps, 60)
    report(f"one-shot, {S} streams x {T} samples of voiced voices over sawtooth carriers, F = {F}, hop = {hop}", times, S * nF, base, emit)
    mean = {k: sum(t) / len(t) for k, t in times.items()}
    emit(f"  cross-synthesis = {mean['formant kernel, ratio 1'] / mean['cross-synthesis']:.3f} x the formant kernel (frames/s, the same run)")
    st.close()
    N, K = 1024, 16
    xs = CrossSynthStream(S, N, hop=hop)

    def slab(x):
        return x[:, :K * N].reshape(S, K, N).permute(1, 0, 2).contiguous()
    vb, cb = slab(v), slab(c)
    yb = torch.empty_like(cb)
    legs = {"streaming cross-synthesis": lambda: xs.process_device(vb, cb, yb, n_blocks=K, d_depth=depth)}
    stimes = alternate(legs, reps, 300)
    r = [S * K * N // hop / t / 1e6 for t in stimes["streaming cross-synthesis"]]
    emit(f"streaming, {S} streams, {K} blocks of {N} per call, hop = {hop}")
    emit(f"  {'streaming cross-synthesis':<28s} {sum(r) / len(r):8.1f} M frames/s  (min {min(r):.1f}, max {max(r):.1f}, {len(r)} repetitions)  "
         f"{sum(r) / len(r) / (S * nF / mean['cross-synthesis'] / 1e6):.3f} x the one-shot cross-synthesis")
    xs.close()


def harm_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import HarmonizerStream, PhaseVocoderStream, StftRoundTrip, semitones_to_ratios
    S, T, F, hop, fs, V = 256, 65536, 1024, 256, 44100.0, 3
    semis = np.array([4.0, 7.0, -5.0])
    gains, dry = (1.0, 0.7, 0.7), 1.0
    st = StftRoundTrip(S, T, F, hop)
    nF = st.n_frames
    ratio = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(semitones_to_ratios(semis)[None, :, None], (S, V, nF)))).cuda()
    per = [ratio[:, v, :].contiguous() for v in range(V)]
    d_gain = torch.from_numpy(np.tile(np.array(gains), (S, 1))).cuda()
    d_dry = torch.from_numpy(np.full(S, dry)).cuda()
    new, base, one = "harmonizer, 3 voices + dry", "3 locked + round trip + mix", "one locked call"
    inputs = (("noise", torch.randn(S, T, device="cuda", dtype=torch.float32) * 0.1), ("voiced signals", torch.from_numpy(voiced_rows(S, T, fs)).cuda()))
    w = torch.tensor([list(gains) + [dry]], dtype=torch.float32, device="cuda")
    for what, x in inputs:
        y = torch.empty_like(x)
        parts = torch.empty((V + 1, S, T), dtype=torch.float32, device="cuda")

        def composed(x=x, y=y, parts=parts):
            for v in range(V):
                st.pitch_shift_locked(x, parts[v], d_ratio=per[v])
            st(x, parts[V])
            torch.mm(w, parts.view(V + 1, -1), out=y.view(1, -1))          # the mix: one pass over the four parts, one write
        legs = {new: lambda x=x, y=y: st.harmonize(x, y, d_ratio=ratio, gains=d_gain, dry=d_dry),
                base: composed,
                one: lambda x=x, y=y: st.pitch_shift_locked(x, y, d_ratio=per[0])}
        report(f"one-shot, {S} streams x {T} samples of {what}, F = {F}, hop = {hop}", alternate(legs, reps, 40), S * nF, base, emit)
    st.close()
    N, K = 1024, 16
    hz = HarmonizerStream(S, N, V, hop=hop)
    ps = [PhaseVocoderStream(S, N, hop=hop) for _ in range(V)]
    tab = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(semitones_to_ratios(semis), (K, S, V)))).cuda()
    tabs = [tab[:, :, v].contiguous() for v in range(V)]
    for what, x in inputs:
        xb = x[:, :K * N].reshape(S, K, N).transpose(0, 1).contiguous()
        yb = torch.empty_like(xb)
        parts = torch.empty((V + 1, K, S, N), dtype=torch.float32, device="cuda")
        parts[V].copy_(xb)                                     # (the dry part: the input as it is)

        def composed(xb=xb, yb=yb, parts=parts):
            for v in range(V):
                ps[v].process_device(xb, parts[v], n_blocks=K, d_ratio=tabs[v], locked=True)
            torch.mm(w, parts.view(V + 1, -1), out=yb.view(1, -1))
        legs = {"streaming harmonizer": lambda xb=xb, yb=yb: hz.process_device(xb, yb, n_blocks=K, d_ratio=tab, gains=d_gain, dry=d_dry),
                "3 locked streams + mix": composed}
        report(f"streaming, {S} streams, {K} blocks of {N} per call of {what}, hop = {hop}", alternate(legs, reps, 150), S * K * N // hop,
               "3 locked streams + mix", emit)
    hz.close()
    for p in ps:
        p.close()


def harmkey_legs(reps, emit):
    import numpy as np
    import torch
    from vocoderproject_amd import HarmonizerStream, StftRoundTrip, StreamingPitchTracker
    S, T, F, hop, fs, V = 256, 65536, 1024, 256, 44100.0, 3
    gains, dry = (1.0, 0.7, 0.7), 1.0
    st = StftRoundTrip(S, T, F, hop)
    nF = st.n_frames
    keys = torch.from_numpy((np.arange(S) % 13).astype(np.int32)).cuda()
    deg = torch.from_numpy(np.tile(np.array([2, 4, -3], np.int32), (S, 1))).cuda()
    unv = torch.from_numpy(np.tile(2.0 ** (np.array([4.0, 7.0, -5.0]) / 12.0), (S, 1))).cuda()
    d_gain = torch.from_numpy(np.tile(np.array(gains), (S, 1))).cuda()
    d_dry = torch.from_numpy(np.full(S, dry)).cuda()
    w = torch.tensor([list(gains) + [dry]], dtype=torch.float32, device="cuda")
    inputs = (("voiced signals", torch.from_numpy(voiced_rows(S, T, fs)).cuda()), ("noise", torch.randn(S, T, device="cuda", dtype=torch.float32) * 0.1))
    trk, harm, table, both, old = "track_pitch", "track_harmony, V = 3", "harmonize on its table", "harmonize_key", "3 autotune(locked) + mix"
    for what, x in inputs:
        y = torch.empty_like(x)
        parts = torch.empty((V + 1, S, T), dtype=torch.float32, device="cuda")
        parts[V].copy_(x)                                      # (the composition's dry part: the input as it is)
        period, ratio = st.track_harmony(x, fs, deg, keys=keys, unvoiced=unv)
        torch.cuda.synchronize()
        voiced = float((period > 0).float().mean())

        def composed(x=x, y=y, parts=parts):
            for v in range(V):
                st.autotune(x, parts[v], fs, keys=keys, locked=True)
            torch.mm(w, parts.view(V + 1, -1), out=y.view(1, -1))
        legs = {trk: lambda x=x: st.track_pitch(x, fs, keys=keys),
                harm: lambda x=x: st.track_harmony(x, fs, deg, keys=keys, unvoiced=unv),
                table: lambda x=x, y=y, ratio=ratio: st.harmonize(x, y, d_ratio=ratio, gains=d_gain, dry=d_dry),
                both: lambda x=x, y=y: st.harmonize(x, y, degrees=deg, sample_rate=fs, keys=keys, unvoiced=unv, gains=d_gain, dry=d_dry),
                old: composed}
        times = alternate(legs, reps, 20)
        report(f"one-shot, {S} streams x {T} samples of {what} at {fs:g} Hz, F = {F}, hop = {hop}, {100.0 * voiced:.0f} % of the frames voiced",
               times, S * nF, trk, emit)
        m = {k: sum(v) / len(v) for k, v in times.items()}
        emit(f"  track_harmony / track_pitch, frames per second: {m[trk] / m[harm]:.3f}")
        emit(f"  per call: track_harmony {m[harm] * 1e3:.3f} ms + harmonize {m[table] * 1e3:.3f} ms = {(m[harm] + m[table]) * 1e3:.3f} ms; "
             f"harmonize_key {m[both] * 1e3:.3f} ms = {m[both] / (m[harm] + m[table]):.3f} x the sum; "
             f"3 autotune(locked) + mix {m[old] * 1e3:.3f} ms = {m[old] / m[both]:.2f} x harmonize_key")
    st.close()
    N, K = 1024, 16
    for what, x in inputs:
        blocks = x[:, :(K + 2) * N].reshape(S, K + 2, N).transpose(0, 1).contiguous()
        hz_a, hz_b, trk_a, trk_b = HarmonizerStream(S, N, V, hop=hop), HarmonizerStream(S, N, V, hop=hop), StreamingPitchTracker(S, N, fs, F), StreamingPitchTracker(S, N, fs, F)
        for t in (trk_a, trk_b):                               # two blocks of history first: every timed decision has a full window
            t.process_voices_device(blocks[:2], deg, n_blocks=2, keys=keys, unvoiced=unv)
        slab = blocks[2:].contiguous()
        yb = torch.empty_like(slab)
        _, tab = trk_a.process_voices_device(slab, deg, n_blocks=K, keys=keys, unvoiced=unv)
        legs = {"tracker, voices": lambda slab=slab: trk_a.process_voices_device(slab, deg, n_blocks=K, keys=keys, unvoiced=unv),
                "harmonizer on its table": lambda slab=slab, yb=yb, tab=tab: hz_a.process_device(slab, yb, n_blocks=K, d_ratio=tab, gains=d_gain, dry=d_dry),
                "autoharm": lambda slab=slab, yb=yb: hz_b.autoharm_device(trk_b, slab, yb, deg, n_blocks=K, keys=keys, unvoiced=unv, gains=d_gain, dry=d_dry)}
        times = alternate(legs, reps, 150)
        m = {k: sum(v) / len(v) for k, v in times.items()}
        parts_t = m["tracker, voices"] + m["harmonizer on its table"]
        emit(f"streaming, {S} streams, {K} blocks of {N} per call of {what}, hop = {hop}")
        emit(f"  per call: tracker {m['tracker, voices'] * 1e3:.3f} ms + harmonizer {m['harmonizer on its table'] * 1e3:.3f} ms = {parts_t * 1e3:.3f} ms; "
             f"autoharm {m['autoharm'] * 1e3:.3f} ms = {m['autoharm'] / parts_t:.3f} x the sum "
             f"({S * K * N // hop / m['autoharm'] / 1e6:.1f} M frames/s)")
        for h in (hz_a, hz_b, trk_a, trk_b):
            h.close()


def resource_listing(emit, kernels=("vp_k_stft_fused<true, false>", "vp_k_stft_pv_stretch", "vp_k_stft_pv2k", "vp_k_stft_pv2k_stretch")):
    try:
        import kernel_resources
        from vocoderproject_amd import processor
        res = kernel_resources.kernel_resources(processor.LIB_PATH)
    except Exception as e:                                                  # (no llvm tools next to the runtime)
        emit(f"kernel resources: not available ({type(e).__name__})")
        return
    emit("kernel resources (tools/kernel_resources.py):")
    for k in kernels:
        emit(f"  {k:<30s} {res.get(k)}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--curve", action="store_true", help="the ratio-curve legs instead of the fixed intervals")
    ap.add_argument("--stretch", action="store_true", help="the time-stretch legs instead of the fixed intervals")
    ap.add_argument("--track", action="store_true", help="the pitch-tracker legs instead of the fixed intervals")
    ap.add_argument("--track-stream", action="store_true", help="the streaming-tracker legs instead of the fixed intervals")
    ap.add_argument("--track-fine", action="store_true", help="the fine trackers beside the integer ones instead of the fixed intervals")
    ap.add_argument("--locked", action="store_true", help="the peak-locked legs instead of the fixed intervals")
    ap.add_argument("--locked-subbin", action="store_true", help="the sub-bin peak-locked legs instead of the fixed intervals")
    ap.add_argument("--stretch-locked", action="store_true", help="the locked time-stretch legs instead of the fixed intervals")
    ap.add_argument("--transient", action="store_true", help="the onset-flux and reset-kernel legs instead of the fixed intervals")
    ap.add_argument("--cross", action="store_true", help="the cross-synthesis legs instead of the fixed intervals")
    ap.add_argument("--harm", action="store_true", help="the harmonizer legs instead of the fixed intervals")
    ap.add_argument("--harmkey", action="store_true", help="the key-aware voices' legs instead of the fixed intervals")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="--curve / --stretch / --track: also write the report to this file")
    a = ap.parse_args()
    if not a.curve and not a.stretch and not a.track and not a.track_stream and not a.locked and not a.locked_subbin and not a.stretch_locked and not a.transient and not a.cross and not a.harm and not a.harmkey and not a.track_fine:
        return fixed_intervals()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    if a.curve:
        curve_legs(max(5, a.reps), emit)
    if a.stretch:
        stretch_legs(max(5, a.reps), emit)
        resource_listing(emit)
    if a.track:
        track_legs(max(5, a.reps), emit)
        resource_listing(emit, ("vp_k_yin_track", "vp_k_stft_pv_curve", "vp_k_stft_pv2k_curve"))
    if a.track_stream:
        track_stream_legs(max(5, a.reps), emit)
        resource_listing(emit, ("vp_k_yin_track", "vp_k_yin_track_stream", "vp_k_track_follow", "vp_k_track_reset", "vp_k_pv_stream_curve"))
    if a.track_fine:
        track_fine_legs(max(5, a.reps), emit)
        resource_listing(emit, ("vp_k_yin_track", "vp_k_yin_track_fine", "vp_k_yin_track_stream", "vp_k_yin_track_stream_fine"))
    if a.locked:
        locked_legs(max(5, a.reps), emit)
        resource_listing(emit, ("vp_k_stft_pv_curve", "vp_k_stft_pv_lock", "vp_k_pv_stream_curve", "vp_k_pv_stream_lock"))
    if a.locked_subbin:
        locked_subbin_legs(max(5, a.reps), emit)
        resource_listing(emit, ("vp_k_stft_pv_lock", "vp_k_stft_pv_lockf", "vp_k_pv_stream_lock", "vp_k_pv_stream_lockf"))
    if a.stretch_locked:
        stretch_locked_legs(max(5, a.reps), emit)
        resource_listing(emit, ("vp_k_stft_pv_lock", "vp_k_stft_pv_stretch", "vp_k_stft_pv_stretch_lock"))
    if a.transient:
        transient_legs(max(5, a.reps), emit)
        resource_listing(emit, ("vp_k_stft_pv_stretch_lock", "vp_k_stft_pv_stretch_lock_reset", "vp_k_stft_onset_flux"))
    if a.cross:
        cross_legs(max(5, a.reps), emit)
        resource_listing(emit, ("vp_k_stft_fused<false, false>", "vp_k_stft_pv_formant", "vp_k_stft_cross", "vp_k_xs_stream"))
    if a.harm:
        harm_legs(max(5, a.reps), emit)
        resource_listing(emit, ("vp_k_stft_pv_lock", "vp_k_stft_harm", "vp_k_pv_stream_lock", "vp_k_hz_stream"))
    if a.harmkey:
        harmkey_legs(max(5, a.reps), emit)
        resource_listing(emit, ("vp_k_yin_track", "vp_k_yin_track_voices", "vp_k_yin_track_stream", "vp_k_yin_track_voices_stream", "vp_k_track_follow",
                                "vp_k_track_follow_voices", "vp_k_stft_harm", "vp_k_hz_stream"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
