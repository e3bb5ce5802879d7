#!/usr/bin/env python3
"""What the channel-pointer entry points cost beside the packed ones, in one process, the variants interleaved.

    python tools/channels_bench.py [--calls 2000] [--repeats 7] [--out profiles/channels_bench.json]

Legs:
  headline   256 mono streams, N = 1024, pitch corrector only, VP_IIR_FAST (the bench.py headline), 1 and 8 blocks per call:
             vp_process_block[s]_mono_device on the packed voice slab / vp_process_block[s]_channels_device with n_in = 1
  both       1024 streams, both processes, VP_IIR_FAST, n_in = 3, one block per call
Variants of a leg: `packed` (the slab is already there: nothing to move), `channels` (device tables of separately allocated rows),
`stack` (the same rows packed by hand with one torch.stack -- plus the block-major permute for several blocks -- then the packed
call; its output stays packed, i.e. it is charged nothing for the way back).  Every variant has a handle of its own; a repeat times
`--calls` calls of each variant in turn between device events, and the figures are the median over the repeats with their spread.
A library without the channel entry points (VP_AMD_LIB pointing at an older build) reports the packed variant alone: that is how the
packed figures of two builds are compared.

The kernel trace is a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/channels_bench.py --trace
    python tools/channels_bench.py --summarise-trace <dir>       # the vp_k_* kernels per launch shape (a leg each)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, HOP = 44100.0, 256
UNIQUE = 16                                   # distinct blocks of input a leg cycles through


class Leg:
    def __init__(self, name, S, N, blocks, mono, pitch, voc):
        self.name, self.S, self.N, self.B, self.mono, self.pitch, self.voc = name, S, N, blocks, mono, pitch, voc
        self.n_in = 1 if mono else 3

    def frames(self):
        return self.S * self.B * self.N / HOP

    def handle(self):
        from vocoderproject_amd import BatchVocoderProcessor
        p = BatchVocoderProcessor(pitchBool=self.pitch, vocBool=self.voc)
        p.prepareToPlay(FS, self.N, self.S)
        p.set_iir_mode("fast")
        p.set_yin_mode("xcorr")
        if self.B > 1:
            p.reserve_blocks(self.B)
        return p

    def build(self, have_channels):
        """-> {variant: callable(i)} issuing call number i"""
        import torch
        from vocoderproject_amd import BatchVocoderProcessor
        from vocoderproject_amd.synth import make_streams
        S, N, B, n_in = self.S, self.N, self.B, self.n_in
        x = make_streams(S, N * UNIQUE, device="cuda")[:, :n_in]                      # [S][n_in][U N]
        slabs = x.reshape(S, n_in, UNIQUE, N).permute(2, 0, 1, 3).contiguous()         # [U][S][n_in][N]
        if self.mono:
            slabs = slabs[:, :, 0].contiguous()                                         # [U][S][N]
        y = torch.empty((B, S, 2, N), dtype=torch.float32, device="cuda")
        self.handles = []
        variants = {}

        def packed_call(p, slab):
            if self.mono:
                (p.process_mono_device(slab[0], y[0]) if B == 1 else p.process_blocks_mono_device(slab, y))
            else:
                (p.process_device(slab[0], y[0]) if B == 1 else p.process_blocks_device(slab, y))

        p0 = self.handle()
        self.handles.append(p0)
        variants["packed"] = lambda i: packed_call(p0, slabs[(i * B) % UNIQUE:(i * B) % UNIQUE + B])
        # rows: one allocation per (stream, channel), UNIQUE * N samples; a call reads B blocks from a rotating offset through tables
        # built once per offset
        rows = [x[s, ch].clone() for s in range(S) for ch in range(n_in)]
        out_rows = [torch.empty(B * N, dtype=torch.float32, device="cuda") for _ in range(S * 2)]
        offsets = sorted({(i * B) % UNIQUE for i in range(UNIQUE)})
        if have_channels:
            p1 = self.handle()
            self.handles.append(p1)
            t_out = BatchVocoderProcessor.channel_table(out_rows)
            t_in = {o: BatchVocoderProcessor.channel_table([r[o * N:(o + B) * N] for r in rows]) for o in offsets}
            variants["channels"] = lambda i: p1.process_channels_device(t_in[(i * B) % UNIQUE], n_in, t_out, 2, n_blocks=B)
        p2 = self.handle()
        self.handles.append(p2)
        views = {o: [r[o * N:(o + B) * N] for r in rows] for o in offsets}
        stacked = torch.empty((S * n_in, B * N), dtype=torch.float32, device="cuda")

        def stack_call(i):
            torch.stack(views[(i * B) % UNIQUE], out=stacked)
            slab = stacked.view(S, n_in, B, N).permute(2, 0, 1, 3)
            slab = slab.contiguous() if B > 1 else slab.reshape(1, S, n_in, N)
            packed_call(p2, slab[:, :, 0] if self.mono else slab)
        variants["stack"] = stack_call
        return variants

    def close(self):
        for p in self.handles:
            p.close()


LEGS = [Leg("headline_1_block", 256, 1024, 1, True, 1, 0), Leg("headline_8_blocks", 256, 1024, 8, True, 1, 0),
        Leg("both_1024_streams", 1024, 1024, 1, False, 1, 1)]


def time_calls(fn, calls, i0):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i0 + i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / calls


def summarise_trace(d):
    """Average duration of every vp_k_* kernel of a rocprofv3 kernel trace, per grid (the legs launch different grids)."""
    import csv
    import glob
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            if not name.startswith("vp_k"):
                continue
            key = (name, r.get("Grid_Size_X", "?"), r.get("Grid_Size_Y", "?"), r.get("Workgroup_Size_X", "?"))
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, gx, gy, wx), ts in sorted(rows.items()):
        print(f"{name:40s} grid {gx:>8s} x {gy:>3s} (workgroup {wx:>4s})  calls {len(ts):5d}  avg {statistics.mean(ts):8.2f} us  "
              f"min {min(ts):8.2f}  max {max(ts):8.2f}")
    return 0 if rows else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000, help="single-block calls per timed window (several blocks per call: divided by them)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="a short run for the kernel trace (no figures)")
    ap.add_argument("--summarise-trace", default=None, metavar="DIR", help="print the per-kernel times of a rocprofv3 output directory")
    a = ap.parse_args()
    if a.summarise_trace:
        return summarise_trace(a.summarise_trace)
    import torch
    from vocoderproject_amd.processor import load_library
    if not torch.cuda.is_available():
        print("no GPU: nothing to measure (this tool has no CPU fallback)", file=sys.stderr)
        return 1
    have = hasattr(load_library(), "vp_process_block_channels_device")
    res = dict(channel_entry_points=have, calls=a.calls, repeats=a.repeats, legs=[])
    for leg in LEGS:
        variants = leg.build(have)
        calls = 20 if a.trace else max(20, a.calls // leg.B)
        for fn in variants.values():                                                  # warm-up: every variant, every offset
            for i in range(2 * UNIQUE):
                fn(i)
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for r in range(1 if a.trace else a.repeats):
            for k, fn in variants.items():                                            # interleaved: the variants share whatever else the box does
                times[k].append(time_calls(fn, calls, r * calls))
        row = dict(leg=leg.name, streams=leg.S, N=leg.N, blocks_per_call=leg.B, n_in=leg.n_in, variants={})
        for k, ts in times.items():
            med = statistics.median(ts)
            row["variants"][k] = dict(us_per_call=med * 1e6, us_min=min(ts) * 1e6, us_max=max(ts) * 1e6, frames_per_s=leg.frames() / med,
                                      spread=(max(ts) - min(ts)) / med)
        base = row["variants"]["packed"]["us_per_call"]
        for k, v in row["variants"].items():
            v["vs_packed"] = v["us_per_call"] / base
        res["legs"].append(row)
        leg.close()
        if not a.trace:
            for k, v in row["variants"].items():
                print(f"{leg.name:18s} {k:9s} {v['frames_per_s'] / 1e6:8.2f} M frames/s  {v['us_per_call']:8.1f} us/call "
                      f"(min {v['us_min']:.1f}, max {v['us_max']:.1f}, spread {100 * v['spread']:.1f} %)  {v['vs_packed']:.3f}x packed", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
