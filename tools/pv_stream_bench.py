#!/usr/bin/env python3
"""The streaming phase vocoder (vp_pv_*, vp_k_pv_stream) against the one-shot vp_stft_pitch_shift, in one process.

    python tools/pv_stream_bench.py [--out profiles/pv_stream_bench.json] [--calls 200]

Reports frames/s at 256 streams, hop 256, blocks of 256 and 1024 samples, with 1 and 16 blocks per call, and the one-shot figure at
256 streams x 65 536 samples; bytes per call (input + output + state read and written).  The kernel trace is a run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -o pv -- python tools/pv_stream_bench.py --trace
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, HOP, F = 256, 256, 1024
REC_BYTES = (2 * 513 + 2) * 8 + 2 * 1024 * 4          # one stream's state (vp_stft.h VP_PV_REC_BYTES)


def bytes_per_call(N, blocks):
    return S * (2 * blocks * N * 4 + 2 * REC_BYTES)


def stream_rate(N, blocks, calls, warm=10):
    import torch
    from vocoderproject_amd import PhaseVocoderStream
    ps = PhaseVocoderStream(S, N, hop=HOP)
    ps.set_semitones(7)
    x = torch.randn(blocks, S, N, device="cuda", dtype=torch.float32) * 0.1
    y = torch.empty_like(x)
    for _ in range(warm):
        ps.process_device(x, y, n_blocks=blocks)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        ps.process_device(x, y, n_blocks=blocks)
    e1.record()
    torch.cuda.synchronize()
    dt = e0.elapsed_time(e1) / 1e3 / calls
    frames = S * blocks * N / HOP
    ps.close()
    return dict(N=N, blocks_per_call=blocks, us_per_call=dt * 1e6, frames_per_s=frames / dt, bytes_per_call=bytes_per_call(N, blocks),
                GB_per_s=bytes_per_call(N, blocks) / dt / 1e9)


def one_shot_rate(calls, T=65536):
    import torch
    from vocoderproject_amd import StftRoundTrip
    x = torch.randn(S, T, device="cuda", dtype=torch.float32) * 0.1
    y = torch.empty_like(x)
    st = StftRoundTrip(S, T, F, HOP)
    for _ in range(3):
        st.pitch_shift(x, y, 7.0)
    torch.cuda.synchronize()
    n = max(3, calls // 20)
    t0 = time.perf_counter()
    for _ in range(n):
        st.pitch_shift(x, y, 7.0)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    frames = S * ((T - F) // HOP + 1)
    st.close()
    return dict(S=S, T=T, us_per_call=dt * 1e6, frames_per_s=frames / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="a short run for the kernel trace (no figures)")
    a = ap.parse_args()
    import torch  # noqa: F401
    if a.trace:
        for N in (256, 1024):
            for b in (1, 16):
                stream_rate(N, b, 20, warm=2)
        one_shot_rate(20)
        return 0
    res = dict(streams=S, hop=HOP, frame=F, stream=[], one_shot=one_shot_rate(a.calls))
    for N in (256, 1024):
        for b in (1, 16):
            res["stream"].append(stream_rate(N, b, a.calls if b == 1 else max(20, a.calls // 8)))
    ref = res["one_shot"]["frames_per_s"]
    for r in res["stream"]:
        r["vs_one_shot"] = r["frames_per_s"] / ref
    print(f"one-shot vp_stft_pitch_shift, {S} x {res['one_shot']['T']}: {ref / 1e6:7.1f} M frames/s")
    for r in res["stream"]:
        print(f"stream N={r['N']:5d} x{r['blocks_per_call']:3d} blocks/call: {r['frames_per_s'] / 1e6:7.1f} M frames/s "
              f"({r['vs_one_shot']:.2f}x one-shot)  {r['us_per_call']:8.1f} us/call  {r['bytes_per_call'] / 1e6:6.2f} MB/call "
              f"{r['GB_per_s']:7.1f} GB/s")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
