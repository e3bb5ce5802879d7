"""Offline (file-to-file) front end: the caller one step either side of the hot path.

The reference's notebook renders whole recordings -- `pitch_corrector(x, ...)` and `vocode(x, y, ...)`
(Notebook/"Pitch Corrector and Vocoder.ipynb" cells 9 and 25) on signals read with `wavio.read(...).data[:, 0] / 32767`
(cells 3, 15, 22) and returns an output as long as, and aligned with, its input.  This module does the same with the
plugin's own path (the MI355X kernels behind the C ABI) for a whole BATCH of recordings at once: every recording is one
stream of one `BatchVocoderProcessor`, the batch is padded to a common length, pushed through `processBlock()` block by
block (several blocks per call where the library offers it), and the plugin's latency (`setLatencySamples`,
PluginProcessor.cpp:175,183) is taken off the front so that output sample t belongs to input sample t.

There is no CPU path here either: without a GPU the processor raises.

    python -m vocoderproject_amd.offline pitch  take1.wav take2.wav --out-dir tuned/ [--key 12] [--shift +3]
    python -m vocoderproject_amd.offline vocode voice.wav --carrier synth.wav --out-dir out/
    python -m vocoderproject_amd.offline pvshift a.wav b.wav --shift 7 --out-dir out/     (streaming phase vocoder)
    python -m vocoderproject_amd.offline pvshift a.wav --glide -12:12 --out-dir out/      (... along a glide, one interval per block)
    python -m vocoderproject_amd.offline stretch a.wav b.wav --stretch 1.5 [--shift 3] [--locked] --out-dir out/   (time stretch, one-shot phase vocoder)
    python -m vocoderproject_amd.offline stretch a.wav --stretch 2 --locked --transients [THR] [--span K] --out-dir out/   (attacks kept: no stretch across an onset, phases restart at it)
    python -m vocoderproject_amd.offline pvshift a.wav --shift -12 --locked --subbin --out-dir out/   (peak locking with sub-bin region offsets)
    python -m vocoderproject_amd.offline pvtune a.wav b.wav --key 0 --out-dir out/ [--track-csv] [--fine]   (pitch tracker + phase-vocoder correction; --fine: sub-sample periods)
    python -m vocoderproject_amd.offline pvtune a.wav --stream [--block 256 --hold 8 --glide 0.5] --out-dir out/   (... block by block: the streaming tracker)
    python -m vocoderproject_amd.offline pvcross voice.wav [more.wav] --carrier synth.wav [--depth D] [--lifter N] [--stream --block N] [--hop H] --out-dir out/   (STFT cross-synthesis)
    python -m vocoderproject_amd.offline harmonize a.wav [b.wav] --voices 4,7,-5 [--gains 1,1,0.7] [--dry 1] [--stream --block N] [--hop H] --out-dir out/   (peak-locked harmonizer)
    python -m vocoderproject_amd.offline harmonize a.wav [b.wav] --degrees 2,4,-3 --key 0 [--gains ..] [--dry 1] [--stream --block N --hold 8 --glide 0.5] [--track-csv] --out-dir out/   (voices at degrees of the key)
"""
import argparse
import os
import sys
import wave

import numpy as np

PCM_SCALE = 32767.0          # the notebook's convention: int16 / 32767.0 (cell 3)


# ---- WAV files (stdlib `wave`: integer PCM, 8/16/24/32 bit) -------------------------------------------------------------

def read_wav(path):
    """-> (sample_rate, float32 [channels][T]) scaled like the notebook does: int16 / 32767 (other widths likewise by
    their own full scale)."""
    with wave.open(path, "rb") as w:
        nch, width, fs, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if width == 1:
        a = (np.frombuffer(raw, np.uint8).astype(np.float64) - 128.0) / 127.0
    elif width == 2:
        a = np.frombuffer(raw, "<i2").astype(np.float64) / PCM_SCALE
    elif width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        a = v.astype(np.float64) / float((1 << 23) - 1)
    elif width == 4:
        a = np.frombuffer(raw, "<i4").astype(np.float64) / float((1 << 31) - 1)
    else:
        raise ValueError(f"{path}: unsupported sample width {width}")
    a = a.reshape(-1, nch).T
    return int(fs), np.ascontiguousarray(a, np.float32)


def write_wav(path, fs, y, width=2):
    """y: float [channels][T] or [T]; clipped to full scale; 16-bit (default) or 24-bit PCM."""
    y = np.asarray(y, np.float64)
    if y.ndim == 1:
        y = y[None]
    full = {2: PCM_SCALE, 3: float((1 << 23) - 1)}[width]
    v = np.rint(np.clip(y, -1.0, 1.0) * full).astype(np.int32).T          # [T][ch]
    if width == 2:
        raw = v.astype("<i2").tobytes()
    else:
        u = (v & 0xFFFFFF).astype(np.uint32).reshape(-1)
        raw = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    with wave.open(path, "wb") as w:
        w.setnchannels(y.shape[0])
        w.setsampwidth(width)
        w.setframerate(int(fs))
        w.writeframes(raw)


# ---- batching -----------------------------------------------------------------------------------------------------------

def pack_batch(voices, carriers, N, latency):
    """Recordings of different lengths -> one [S][3][T] float32 batch, T a multiple of N that leaves room for the
    plugin's latency behind the longest recording.  carriers[s] may be None (no side chain: zeros, like the null
    pointer of MyBuffer.cpp:93-102), mono [T] (copied to both side-chain channels) or stereo [2][T]."""
    S = len(voices)
    if S == 0:
        raise ValueError("no recordings")
    lens = [int(np.asarray(v).shape[-1]) for v in voices]
    T = max(lens) + int(latency)
    T = ((T + N - 1) // N) * N
    x = np.zeros((S, 3, T), np.float32)
    for s in range(S):
        v = np.asarray(voices[s], np.float32)
        if v.ndim != 1:
            raise ValueError(f"voice {s}: expected a mono signal, got shape {v.shape}")
        x[s, 0, :lens[s]] = v
        c = None if carriers is None else carriers[s]
        if c is not None:
            c = np.asarray(c, np.float32)
            if c.ndim == 1:
                c = np.stack([c, c])
            if c.ndim != 2 or c.shape[0] != 2:
                raise ValueError(f"carrier {s}: expected [T] or [2][T], got shape {c.shape}")
            n = min(c.shape[1], T)
            x[s, 1:3, :n] = c[:, :n]
    return x, lens


def unpack_batch(y, lens, latency):
    """[S][2][T] -> list of [2][len_s]: the plugin's latency taken off the front (output t <-> input t)."""
    return [np.ascontiguousarray(y[s, :, latency:latency + lens[s]]) for s in range(len(lens))]


def render(voices, carriers, fs, *, pitch=True, vocoder=False, params=None, stream_params=None, shift=None,
           N=1024, blocks_per_call=8, device=0, iir_mode="exact", yin_mode="direct", processor=None):
    """Push a batch of recordings through the plugin path.  voices: list of mono float arrays (one stream each);
    carriers: None or a list (entries None / mono / stereo).  params: plugin parameter ids -> values for all streams;
    stream_params: optional list of dicts, one per stream; shift: None, one number, or a list of numbers / None per
    stream (fixed interval in semitones, vp_set_pitch_shift).  Returns a list of float32 [2][len] outputs aligned with
    the inputs.  `processor` (tests): an object with the BatchVocoderProcessor interface to use instead of a new one."""
    S = len(voices)
    if processor is None:
        from . import BatchVocoderProcessor
        kw = dict(params or {})
        kw.update(pitchBool=int(bool(pitch)), vocBool=int(bool(vocoder)))
        processor = BatchVocoderProcessor(device=device, **kw)
    p = processor
    p.prepareToPlay(float(fs), int(N), S)
    p.set_iir_mode(iir_mode)
    p.set_yin_mode(yin_mode)
    for s, sp in enumerate(stream_params or []):
        for k, v in (sp or {}).items():
            p.setStreamParameter(s, k, v)
    if shift is not None:
        per = shift if isinstance(shift, (list, tuple)) else [shift] * S
        if len(per) != S:
            raise ValueError("shift: one value per stream expected")
        for s, v in enumerate(per):
            if v is not None:
                p.setPitchShift(float(v), on=True, stream=s)
    lat = p.latency
    x, lens = pack_batch(voices, carriers, int(N), lat)
    T = x.shape[2]
    nb = T // N
    y = np.empty((S, 2, T), np.float32)
    B = max(1, int(blocks_per_call))
    b = 0
    while b < nb:
        k = min(B, nb - b)
        if k > 1 and hasattr(p, "process_blocks"):
            xb = np.ascontiguousarray(x[:, :, b * N:(b + k) * N].reshape(S, 3, k, N).transpose(2, 0, 1, 3))   # [k][S][3][N]
            yb = p.process_blocks(xb)                                                                       # [k][S][2][N]
            y[:, :, b * N:(b + k) * N] = yb.transpose(1, 2, 0, 3).reshape(S, 2, k * N)
        else:
            for j in range(k):
                y[:, :, (b + j) * N:(b + j + 1) * N] = p.process(np.ascontiguousarray(x[:, :, (b + j) * N:(b + j + 1) * N]))
        b += k
    return unpack_batch(y, lens, lat)


def pitch_corrector(voices, fs, key=12, **kw):
    """The notebook's `pitch_corrector(x, ...)` (cell 9) for a batch: mono in, corrected mono out (the plugin writes the
    same signal to both output channels; channel 0 is returned)."""
    params = dict(kw.pop("params", None) or {})
    params.setdefault("keyPitch", int(key))
    return [o[0] for o in render(voices, None, fs, pitch=True, vocoder=False, params=params, **kw)]


def vocode(voices, carriers, fs, order_lpc=40, order_synth=5, **kw):
    """The notebook's `vocode(x, y, window, window_len, hop, order_lpc)` (cell 25) for a batch: voice + carrier in,
    cross-synthesis out ([2][len] per stream: left/right)."""
    params = dict(kw.pop("params", None) or {})
    params.setdefault("lpcVoice", int(order_lpc))
    params.setdefault("lpcSynth", int(order_synth))
    return render(voices, carriers, fs, pitch=False, vocoder=True, params=params, **kw)


# ---- the phase-vocoder flows: validate, size, pack, call, unpack ------------------------------------------------------------------

def _batch_size(voices):
    if len(voices) == 0:
        raise ValueError("no recordings")
    return len(voices)


def _per_recording(value, S, name, conv=float, lo=None, hi=None, range_msg=None):
    """One value or one per recording (list, tuple or array) -> a list of S values through `conv`, each within [lo, hi] (a NaN is
    outside) where a range is given."""
    many = isinstance(value, (list, tuple)) or (isinstance(value, np.ndarray) and value.ndim > 0)
    per = [conv(v) for v in value] if many else [conv(value)] * S
    if len(per) != S:
        raise ValueError(f"{name}: one value per recording expected")
    if range_msg is not None and not all(lo <= v <= hi for v in per):
        raise ValueError(range_msg)
    return per


def _lengths(voices):
    return [int(np.asarray(v).shape[-1]) for v in voices]


def _pack_mono(voices, lens, T):
    """Mono recordings of lengths `lens` -> one zeroed float32 [S][T] with each recording at the front of its row."""
    x = np.zeros((len(voices), int(T)), np.float32)
    for s, v in enumerate(voices):
        v = np.asarray(v, np.float32)
        if v.ndim != 1:
            raise ValueError(f"voice {s}: expected a mono signal, got shape {v.shape}")
        x[s, :lens[s]] = v
    return x


def _both_channels(y, lens, offset=0):
    """[S][T] -> float32 [2][len_s] per recording from sample `offset` on: the signal on both channels, the layout the pitch flow writes."""
    return [np.ascontiguousarray(np.stack([y[s, offset:offset + n]] * 2)) for s, n in enumerate(lens)]


def _check_lifter(lifter):
    if not 4 <= int(lifter) <= 64:
        raise ValueError("lifter: 4 to 64 samples expected")


def _check_formant(formant, lifter):
    if formant is None:
        return
    if not -12.0 <= float(formant) <= 12.0:
        raise ValueError("formant: an interval within +-12 semitones expected")
    _check_lifter(lifter)


def _overlapped(n, hop, F=1024):
    """The length of a one-shot batch whose first n samples all lie under the full overlap of F-point frames."""
    return F + -(-int(n) // hop) * hop


def _check_locked(locked, formant, F=1024):
    if locked and formant is not None:
        raise ValueError("--locked and --formant exclude each other: formant correction on top of peak locking is not built")
    if locked and int(F) != 1024:
        raise ValueError("--locked: 1024-point frames expected (the peak-locked kernels are not built for 2048)")


def _check_subbin(subbin, locked):
    if subbin and not locked:
        raise ValueError("--subbin: valid only together with --locked (the sub-bin region offsets are a variant of the peak-locked call)")


def _mode_kw(formant, lifter, locked, formant_name="formant", subbin=False):
    """What a call receives beyond the plain call's arguments: nothing, the formant pair, locked=True, subbin=True (only when set)."""
    kw = {} if formant is None else {formant_name: float(formant), "lifter": int(lifter)}
    if locked:
        kw["locked"] = True
    if subbin:
        kw["subbin"] = True
    return kw


SHIFT_RANGE = (-12.0, 12.0, "shift: intervals within +-12 semitones expected")


def _stream(processor, S, N, hop, device, cls=None, **kw):
    """`processor` (the tests' double) or a new streaming processor: a PhaseVocoderStream, or `cls` with what else its constructor takes."""
    if processor is not None:
        return processor
    if cls is None:
        from . import PhaseVocoderStream as cls
    return cls(S, int(N), hop=int(hop), device=device, **kw)


def pv_shift(voices, shift, N=1024, hop=256, device=0, processor=None):
    """A batch of recordings through the streaming phase vocoder (PhaseVocoderStream: one stream per recording), block by block,
    its latency taken off the front.  shift: one interval in semitones or one per recording.  Returns float32 [2][len] per
    recording (the shifted signal on both channels: the layout the pitch flow writes).  `processor` (tests): an object with the
    PhaseVocoderStream interface (set_semitones, latency, process) to use instead of a new one."""
    S = _batch_size(voices)
    p = _stream(processor, S, N, hop, device)
    for s, v in enumerate(_per_recording(shift, S, "shift")):
        p.set_semitones(v, stream=s)
    lat = int(p.latency)
    lens = _lengths(voices)
    T = -(-(max(lens) + lat) // N) * N
    x = _pack_mono(voices, lens, T)
    y = np.concatenate([p.process(np.ascontiguousarray(x[:, b:b + N])) for b in range(0, T, N)], axis=1)
    return _both_channels(y, lens, lat)


def glide_curve(lens, start, end, N, n_blocks):
    """Semitones per block and recording, float64 [n_blocks][S]: a linear glide from `start` to `end` over each recording's own blocks
    (block b of a recording of n blocks: start + (end - start) b / (n - 1)), `end` behind its last block."""
    c = np.empty((int(n_blocks), len(lens)))
    for s, n in enumerate(lens):
        nb = max(1, -(-int(n) // int(N)))
        t = np.minimum(np.arange(int(n_blocks)) / max(nb - 1, 1), 1.0)
        c[:, s] = float(start) + (float(end) - float(start)) * t
    return c


def pv_glide(voices, start, end, N=1024, hop=256, device=0, blocks_per_call=16, processor=None, formant=None, lifter=32, locked=False,
             subbin=False):
    """pv_shift with a glide: every recording's interval moves linearly from `start` to `end` semitones over its length, one value per
    block, through the streaming phase vocoder's ratio-curve call (PhaseVocoderStream.run(curve=...): several blocks per call, each
    with its own interval).  Returns float32 [2][len] per recording.  `processor` (tests): an object with latency and
    run(x, blocks_per_call, curve) to use instead of a new PhaseVocoderStream.  formant (semitones; None: the call above, unchanged): the
    formant-preserving call instead -- the spectral envelope moves by `formant` semitones (0: it stays) whatever the pitch does, with a
    cepstral lifter of `lifter` samples; run then also receives formant_semitones and lifter.  locked: the peak-locked call instead
    (run then also receives locked=True); not together with formant.  subbin (with locked only): the locked call with sub-bin region
    offsets (run then also receives subbin=True)."""
    S = _batch_size(voices)
    if not (-12.0 <= float(start) <= 12.0 and -12.0 <= float(end) <= 12.0):
        raise ValueError("glide: intervals within +-12 semitones expected")
    _check_formant(formant, lifter)
    _check_locked(locked, formant)
    _check_subbin(subbin, locked)
    p = _stream(processor, S, N, hop, device)
    lens = _lengths(voices)
    x = _pack_mono(voices, lens, max(lens))
    curve = glide_curve(lens, start, end, N, -(-(max(lens) + int(p.latency)) // int(N)))
    # (run's output is aligned with its input: the latency is off)
    y = p.run(x, blocks_per_call=int(blocks_per_call), curve=curve, **_mode_kw(formant, lifter, locked, "formant_semitones", subbin))
    return _both_channels(y, lens)


def pv_shift_locked(voices, shift, N=1024, hop=256, device=0, blocks_per_call=16, processor=None, subbin=False):
    """pv_shift through the PEAK-LOCKED call: every recording by its own fixed interval (one value or one per recording), streamed block
    by block through PhaseVocoderStream.run(curve=..., locked=True) -- a constant curve.  Returns float32 [2][len] per recording.
    `processor` (tests): an object with latency and run(x, blocks_per_call, curve, locked) to use instead of a new PhaseVocoderStream.
    subbin: the locked call with sub-bin region offsets (run then also receives subbin=True)."""
    S = _batch_size(voices)
    per = _per_recording(shift, S, "shift", float, *SHIFT_RANGE)
    p = _stream(processor, S, N, hop, device)
    lens = _lengths(voices)
    y = p.run(_pack_mono(voices, lens, max(lens)), blocks_per_call=int(blocks_per_call), curve=np.array([per]), **_mode_kw(None, 0, True, subbin=subbin))
    return _both_channels(y, lens)


def _one_shot(x, T, F, hop, device, call):
    """With a StftRoundTrip of x's rows, n_samples T and this geometry: x float32 [S][n_in] goes up, call(st, d_in, d_out) runs, the device
    is synchronised, d_out float32 [S][T] comes down and the handle is closed.  -> (d_out's array, what `call` returned)."""
    import torch
    from . import StftRoundTrip
    dev = torch.device("cuda", device)
    st = StftRoundTrip(x.shape[0], int(T), int(F), int(hop), device=device)
    try:
        d_in = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
        d_out = torch.empty((x.shape[0], int(T)), dtype=torch.float32, device=dev)
        res = call(st, d_in, d_out)
        torch.cuda.synchronize(dev)
        return d_out.cpu().numpy(), res
    finally:
        st.close()


class _FormantShiftRunner:
    """StftRoundTrip.pitch_shift_formant from host arrays: x float32 [S][T], semitones [S] -> float32 [S][T]."""

    def __init__(self, hop, device):
        self.hop, self.device = int(hop), device

    def run(self, x, semitones, formant, lifter):
        def call(st, d_in, d_out):
            st.pitch_shift_formant(d_in, d_out, semitones=np.asarray(semitones, np.float64).reshape(-1, 1) * np.ones((1, st.n_frames)),
                                   formant_semitones=float(formant), lifter=int(lifter))
        return _one_shot(x, x.shape[1], 1024, self.hop, self.device, call)[0]


def pv_shift_formant(voices, shift, formant=0.0, lifter=32, N=1024, hop=256, device=0, stream=False, blocks_per_call=16, processor=None):
    """pv_shift with the spectral envelope kept apart from the pitch: the pitch moves by `shift` semitones (one value or one per recording),
    the formants by `formant` (0: they stay where they were), through a cepstral envelope with a lifter of `lifter` samples (4 .. 64).
    Batch (default): the one-shot call StftRoundTrip.pitch_shift_formant on the recordings padded to a common length under the full
    overlap of 1024-point frames; stream: block by block through PhaseVocoderStream.run(curve=..., formant_semitones=...), as pv_glide
    runs.  Returns float32 [2][len] per recording.  `processor` (tests): an object with run(x, semitones, formant, lifter) (batch) or
    latency and run(x, blocks_per_call, curve, formant_semitones, lifter) (stream) to use instead of the GPU."""
    S = _batch_size(voices)
    per = _per_recording(shift, S, "shift", float, *SHIFT_RANGE)
    _check_formant(formant, lifter)
    hop = int(hop)
    lens = _lengths(voices)
    if stream:
        p = _stream(processor, S, N, hop, device)
        y = p.run(_pack_mono(voices, lens, max(lens)), blocks_per_call=int(blocks_per_call), curve=np.array([per]), formant_semitones=float(formant),
                  lifter=int(lifter))
    else:
        x = _pack_mono(voices, lens, _overlapped(max(lens), hop))
        p = processor if processor is not None else _FormantShiftRunner(hop, device)
        y = p.run(x, per, float(formant), int(lifter))
    return _both_channels(y, lens)


class _StretchRunner:
    """StftRoundTrip.time_stretch (locked: time_stretch_locked) from host arrays: x float32 [S][n_in], pos int32 [S][n_frames] -> float32
    [S][T]."""

    def __init__(self, F, hop, device):
        self.F, self.hop, self.device = int(F), int(hop), device

    def run(self, x, pos, T, semitones, locked=False, reset=None):
        def call(st, d_in, d_out):
            if reset is not None:
                import torch
                st.time_stretch_locked(d_in, d_out, positions=pos, semitones=float(semitones), d_reset=torch.from_numpy(np.ascontiguousarray(reset, dtype=np.uint8)).to(d_in.device))
            else:
                (st.time_stretch_locked if locked else st.time_stretch)(d_in, d_out, positions=pos, semitones=float(semitones))
        return _one_shot(x, T, self.F, self.hop, self.device, call)[0]

    def flux(self, x):
        """StftRoundTrip.onset_flux from the host array x float32 [S][n_in] -> (flux, mass) float64 [S][nG]."""
        import torch
        from .processor import StftRoundTrip
        x = np.ascontiguousarray(x, dtype=np.float32)
        st = StftRoundTrip(x.shape[0], self.F + self.hop, self.F, self.hop, self.device)
        try:
            d_flux, d_mass = st.onset_flux(torch.from_numpy(x).to(torch.device("cuda", self.device)))
            return d_flux.cpu().numpy(), d_mass.cpu().numpy()
        finally:
            st.close()


def transient_tables(flux, mass, lens, per, nF, hop, F, thr, span):
    """The position and reset tables of a batch, int32 and uint8 [S][nF]: recording s is picked and planned against ITS OWN length --
    the first (max(lens[s], F) - F) // hop + 1 frames of its row of the padded batch's flux and mass tables, its own stretch per[s]."""
    from .processor import pick_onsets, stretch_positions_transient
    pos, reset = np.zeros((len(lens), nF), np.int32), np.zeros((len(lens), nF), np.uint8)
    for s, (n, a) in enumerate(zip(lens, per)):
        n = max(int(n), F)
        nG = (n - F) // hop + 1
        pos[s], reset[s] = stretch_positions_transient(pick_onsets(flux[s][:nG], mass[s][:nG], thr), nF, hop, a, n, F, span)
    return pos, reset


def pv_stretch(voices, stretch, shift=0.0, F=1024, hop=256, device=0, processor=None, locked=False, transients=None, span=None):
    """A batch of recordings through the one-shot phase vocoder's time stretch (StftRoundTrip.time_stretch: one stream per recording).
    stretch: output duration / input duration in [0.25, 4], one value or one per recording; shift: the pitch shift on top, semitones.
    The recordings are padded to a common input length, each has its own position table (pos[f] = floor(f hop / stretch), held at its
    own last frame), the outputs share one length and each is trimmed to ceil(len stretch) samples.  Returns float32 [2][ceil(len
    stretch)] per recording (the signal on both channels).  `processor` (tests): an object with run(x, pos, T, semitones) to use instead
    of the GPU.  locked: the peak-locked time stretch instead (StftRoundTrip.time_stretch_locked; 1024-point frames); run then also
    receives locked=True.
    transients=thr (with locked only; thr in [0, 1]): the transient-preserving stretch -- the batch's onset flux (processor.flux(x) ->
    flux, mass [S][nG]), then per recording, against its own length, pick_onsets(thr) and stretch_positions_transient(span): a span of
    2 span + 1 frames around every onset is read without stretch and its first frame restarts the phases; run then also receives
    reset=uint8 [S][n_frames].  span: 1 .. 8, None = max(F / (2 hop), 1).  A recording without onsets takes the two-anchor line."""
    S = _batch_size(voices)
    per = _per_recording(stretch, S, "stretch", float, 0.25, 4.0, "stretch: factors within [0.25, 4] expected")
    if transients is not None:
        if not locked:
            raise ValueError("transients: valid only together with locked (the phase reset is a variant of the peak-locked time stretch)")
        if not 0.0 <= float(transients) <= 1.0:
            raise ValueError("transients: a threshold within [0, 1] expected")
        if span is not None and not 1 <= int(span) <= 8:
            raise ValueError("span: 1 to 8 frames expected")
    elif span is not None:
        raise ValueError("span: valid only together with transients")
    if not -12.0 <= float(shift) <= 12.0:
        raise ValueError("shift: an interval within +-12 semitones expected")
    F, hop = int(F), int(hop)
    _check_locked(locked, None, F)
    lens = _lengths(voices)
    outs = [int(np.ceil(n * a)) for n, a in zip(lens, per)]
    x = _pack_mono(voices, lens, max(max(lens), F))
    T = _overlapped(max(outs), hop, F)
    nF = (T - F) // hop + 1
    # (the formula of vp_stretch_positions, against each recording's own length: behind its end a recording repeats its last frame)
    pos = np.stack([np.minimum(np.floor(np.arange(nF, dtype=np.int64) * hop / a), max(n, F) - F) for n, a in zip(lens, per)]).astype(np.int32)
    p = processor if processor is not None else _StretchRunner(F, hop, device)
    if transients is not None:
        flux, mass = p.flux(x)
        pos, reset = transient_tables(flux, mass, lens, per, nF, hop, F, float(transients), None if span is None else int(span))
        return _both_channels(p.run(x, pos, T, float(shift), locked=True, reset=reset), outs)
    y = p.run(x, pos, T, float(shift), **_mode_kw(None, 0, locked))
    return _both_channels(y, outs)


class _AutotuneRunner:
    """StftRoundTrip.autotune from host arrays: x float32 [S][T], keys [S] -> (y float32 [S][T], period int32 [S][nF], ratio float64 [S][nF])."""

    def __init__(self, F, hop, device):
        self.F, self.hop, self.device, self.fine = int(F), int(hop), device, False

    def set_fine(self, fine):
        """The fine tracker (StftRoundTrip.set_track_mode); run then also returns the refined periods float64 [S][nF]."""
        self.fine = bool(fine)

    def run(self, x, fs, keys, formant=None, lifter=32, locked=False, subbin=False):
        def call(st, d_in, d_out):
            if self.fine:
                st.set_track_mode(True)
            res = st.autotune(d_in, d_out, float(fs), keys=[int(k) for k in keys], formant_semitones=formant, lifter=int(lifter),
                              **_mode_kw(None, 0, locked, subbin=subbin))
            return res + (st.track_pitch(d_in, float(fs), keys=[int(k) for k in keys], with_fine_period=True)[2],) if self.fine else res
        y, tables = _one_shot(x, x.shape[1], self.F, self.hop, self.device, call)
        return (y,) + tuple(t.cpu().numpy() for t in tables)


def tune_length(max_len, fs, F, hop):
    """Common row length of a pvtune batch: every sample of the longest recording under the full overlap of frames, and never shorter than
    the tracker's window of F + ceil(fs / 100) samples."""
    F, hop = int(F), int(hop)
    return max(_overlapped(max_len, hop, F), F + int(np.ceil(float(fs) / 100.0)))


def _check_tune(voices, fs, key, formant, lifter):
    """What both pvtune flows check first -> the keys, one per recording."""
    keys = _per_recording(key, _batch_size(voices), "key", int, 0, 12, "key: 0..12 expected (12 = chromatic)")
    if not 8000.0 <= float(fs) <= 51200.0:
        raise ValueError("pvtune: sample rates from 8000 to 51200 Hz are served")
    _check_formant(formant, lifter)
    return keys


def _tune(p, voices, lens, T, fs, keys, kw, offset, with_track, fine=False):
    """Both pvtune flows from the packed call on: p.run(x, fs, keys, **kw) -> the recordings from sample `offset` on, with the track or not.
    fine: p.set_fine(True) first; run then returns the refined periods as a fourth item, and so does the track."""
    if fine:
        p.set_fine(True)
    y, *track = p.run(_pack_mono(voices, lens, T), float(fs), keys, **kw)
    if len(track) != (3 if fine else 2):
        raise ValueError("pvtune: the processor's run returned %d tables where %d were expected" % (len(track), 3 if fine else 2))
    outs = _both_channels(y, lens, offset)
    return (outs,) + tuple(track) if with_track else outs


def pv_autotune(voices, fs, key=12, F=1024, hop=256, device=0, processor=None, with_track=False, formant=None, lifter=32, locked=False,
                subbin=False, fine=False):
    """A batch of recordings through the pitch tracker and the one-shot phase vocoder (StftRoundTrip.autotune: one stream per recording):
    every frame is moved onto the nearest note of its recording's key.  key: Notes::key 0..12 (12 = chromatic), one value or one per
    recording.  The recordings are zero-padded to a common length (tune_length).  Returns float32 [2][len] per recording (the corrected
    signal on both channels); with_track: also period int32 [S][nF] and ratio float64 [S][nF] of the padded batch.  `processor` (tests): an
    object with run(x, fs, keys) to use instead of the GPU.  formant (semitones; None: the correction above, unchanged): the correction
    keeps the spectral envelope apart from the pitch (StftRoundTrip.autotune(formant_semitones=...); 1024-point frames) -- 0 leaves the
    singer's formants where they were; lifter: the cepstral lifter, 4 .. 64 samples; run then also receives formant and lifter.
    locked: the correction runs through the peak-locked call (StftRoundTrip.autotune(locked=True); 1024-point frames, not together with
    formant); run then also receives locked=True.  subbin (with locked only): the locked call with sub-bin region offsets; run then also
    receives subbin=True.  fine: the fine tracker (StftRoundTrip.set_track_mode: the period refined below one sample, the note looked up
    on the refined pitch); the processor's set_fine(True) is called first, and with_track also returns the refined periods float64 [S][nF]."""
    keys = _check_tune(voices, fs, key, formant, lifter)
    if formant is not None and int(F) != 1024:
        raise ValueError("pvtune --formant: 1024-point frames expected (the formant kernels are not built for 2048)")
    _check_locked(locked, formant, F)
    _check_subbin(subbin, locked)
    lens = _lengths(voices)
    p = processor if processor is not None else _AutotuneRunner(F, hop, device)
    return _tune(p, voices, lens, tune_length(max(lens), fs, F, hop), fs, keys, _mode_kw(formant, lifter, locked, subbin=subbin), 0, with_track, fine)


class _StreamTuneRunner:
    """PhaseVocoderStream.autotune_device from host arrays: x float32 [S][n N], keys [S] -> (y float32 [S][n N] with the shifter's latency
    still in front, period int32 [n][S], ratio float64 [n][S])."""

    def __init__(self, N, hop, F, hold, glide, device, blocks_per_call=16):
        self.N, self.hop, self.F, self.hold, self.glide, self.device, self.k = int(N), int(hop), int(F), int(hold), float(glide), device, int(blocks_per_call)
        self.fine = False

    def set_fine(self, fine):
        """The fine tracker (StreamingPitchTracker.set_fine); run then goes through the composed call's two parts, whose bits it has, and
        also returns the raw decisions' refined periods float64 [n][S]."""
        self.fine = bool(fine)

    def _fine_call(self, pv, trk, d_in, d_out, n, keys, formant, lifter, lk):
        period, ratio, fine = trk.process_device(d_in, n_blocks=n, keys=keys, with_fine_period=True)
        pv.process_device(d_in, d_out, n_blocks=n, d_ratio=ratio, **({} if formant is None else {"formant_semitones": formant, "lifter": lifter}), **lk)
        return period, ratio, fine

    def run(self, x, fs, keys, formant=None, lifter=32, locked=False, subbin=False):
        import torch
        from . import PhaseVocoderStream, StreamingPitchTracker
        lk = _mode_kw(None, 0, locked, subbin=subbin)
        S, N = x.shape[0], self.N
        nb = x.shape[1] // N
        dev = torch.device("cuda", self.device)
        pv = PhaseVocoderStream(S, N, hop=self.hop, device=self.device)
        trk = StreamingPitchTracker(S, N, float(fs), frame_len=self.F, hold_blocks=self.hold, glide=self.glide, device=self.device)
        try:
            d_in = torch.from_numpy(np.ascontiguousarray(x.reshape(S, nb, N).transpose(1, 0, 2), np.float32)).to(dev)
            d_out = torch.empty_like(d_in)
            if self.fine:
                trk.set_fine(True)
                tables = [self._fine_call(pv, trk, d_in[b:b + self.k], d_out[b:b + self.k], min(self.k, nb - b), [int(k) for k in keys], formant, int(lifter), lk)
                          for b in range(0, nb, self.k)]
            else:
                tables = [pv.autotune_device(trk, d_in[b:b + self.k], d_out[b:b + self.k], n_blocks=min(self.k, nb - b), keys=[int(k) for k in keys],
                                             formant_semitones=formant, lifter=int(lifter), **lk)
                          for b in range(0, nb, self.k)]
            torch.cuda.synchronize(dev)
            y = d_out.cpu().numpy().transpose(1, 0, 2).reshape(S, nb * N)
            return (np.ascontiguousarray(y),) + tuple(torch.cat([t[i] for t in tables]).cpu().numpy() for i in range(len(tables[0])))
        finally:
            trk.close()
            pv.close()


def stream_tune_length(max_len, N, hop):
    """(padded length, latency) of a streamed pvtune batch: whole blocks that hold the longest recording and the shifter's latency of
    1024 - gcd(N, hop) samples behind it."""
    import math
    lat = 1024 - math.gcd(int(N), int(hop))
    return -(-(int(max_len) + lat) // int(N)) * int(N), lat


def pv_autotune_stream(voices, fs, key=12, N=1024, hop=256, F=1024, hold=0, glide=1.0, device=0, processor=None, with_track=False, formant=None,
                       lifter=32, locked=False, subbin=False, fine=False):
    """pv_autotune block by block, as a live caller would run it: the streaming tracker (StreamingPitchTracker, analysis length F) decides
    one ratio per block of N samples from the audio received so far, holds the last voiced ratio for `hold` unvoiced blocks and moves the
    fraction `glide` of the way to its target per block; the streaming phase vocoder (1024-point frames) shifts along that table.  The
    recordings are zero-padded to whole blocks that also hold the shifter's latency, which is taken off the front.  Returns float32
    [2][len] per recording; with_track: also period int32 [n_blocks][S] and ratio float64 [n_blocks][S] of the padded batch.  A decision
    costs the same at every N: N = 64 costs 16 times as much per second of audio as N = 1024.  `processor` (tests): an object with
    run(x, fs, keys) to use instead of the GPU.  formant, lifter, locked, subbin: as pv_autotune's (the shifter's frames are 1024 points
    whatever F).  fine: as pv_autotune's (StreamingPitchTracker.set_fine); with_track then also returns the raw decisions' refined
    periods float64 [n_blocks][S], which the follow stage neither holds nor glides."""
    keys = _check_tune(voices, fs, key, formant, lifter)
    _check_locked(locked, formant)
    _check_subbin(subbin, locked)
    if int(N) < 1 or int(F) not in (1024, 2048):
        raise ValueError("pvtune --stream: a block of at least one sample and a tracker frame of 1024 or 2048 expected")
    if not (0 <= int(hold) <= 1 << 20 and 0.0 < float(glide) <= 1.0):
        raise ValueError("pvtune --stream: 0 <= hold <= 2^20 blocks and 0 < glide <= 1 expected")
    lens = _lengths(voices)
    T, lat = stream_tune_length(max(lens), N, hop)
    p = processor if processor is not None else _StreamTuneRunner(N, hop, F, hold, glide, device)
    return _tune(p, voices, lens, T, fs, keys, _mode_kw(formant, lifter, locked, subbin=subbin), lat, with_track, fine)


class _CrossRunner:
    """StftRoundTrip.cross_synth from host arrays: voice, carrier float32 [S][T], depth [S] -> float32 [S][T]."""

    def __init__(self, F, hop, device):
        self.F, self.hop, self.device = int(F), int(hop), device

    def run(self, v, c, depth, lifter):
        import torch
        d_c = torch.from_numpy(np.ascontiguousarray(c, np.float32)).to(torch.device("cuda", self.device))

        def call(st, d_in, d_out):
            st.cross_synth(d_in, d_c, d_out, depth=depth, lifter=int(lifter))
        return _one_shot(v, v.shape[1], self.F, self.hop, self.device, call)[0]


def _pack_carriers(carriers, S, lens, T):
    """One carrier for every voice or one per voice -> float32 [S][T]: row s is the carrier cut to voice s's length, silence behind."""
    many = isinstance(carriers, (list, tuple))
    cs = list(carriers) if many else [carriers]
    if len(cs) == 1:
        cs = cs * S
    if len(cs) != S:
        raise ValueError("carrier: one for all voices or one per voice expected")
    c = np.zeros((S, int(T)), np.float32)
    for s, a in enumerate(cs):
        a = np.asarray(a, np.float32)
        if a.ndim != 1:
            raise ValueError(f"carrier {s}: expected a mono signal, got shape {a.shape}")
        n = min(a.size, lens[s])
        c[s, :n] = a[:n]
    return c


def pv_cross(voices, carriers, depth=1.0, lifter=32, F=1024, hop=256, N=1024, stream=False, blocks_per_call=16, device=0, processor=None):
    """STFT cross-synthesis of a batch (one stream per voice): every voice's spectral envelope on its carrier.  carriers: one mono signal for
    all voices or a list with one per voice; a carrier shorter than its voice is padded with silence, a longer one is cut to the voice.
    depth: 0 (the carrier unchanged) .. 1 (the voice's envelope in full), one value or one per voice; lifter: the cepstral lifter, 4 .. 64
    samples.  Batch (default): the one-shot call StftRoundTrip.cross_synth on the recordings padded to a common length under the full
    overlap of 1024-point frames; stream: block by block through CrossSynthStream.run, its latency taken off.  Returns float32 [2][len]
    per voice (the signal on both channels).  `processor` (tests): an object with run(voice, carrier, depth, lifter) (batch) or
    run(voice, carrier, blocks_per_call, depth, lifter) (stream) to use instead of the GPU."""
    S = _batch_size(voices)
    per = _per_recording(depth, S, "depth", float, 0.0, 1.0, "depth: values within [0, 1] expected")
    _check_lifter(lifter)
    if int(F) != 1024:
        raise ValueError("pvcross: 1024-point frames expected (the cross-synthesis kernels are not built for 2048)")
    hop = int(hop)
    lens = _lengths(voices)
    T = max(lens) if stream else _overlapped(max(lens), hop)
    v = _pack_mono(voices, lens, T)
    c = _pack_carriers(carriers, S, lens, T)
    if stream:
        from . import CrossSynthStream
        y = _stream(processor, S, N, hop, device, CrossSynthStream).run(v, c, blocks_per_call=int(blocks_per_call), depth=per, lifter=int(lifter))
    else:
        p = processor if processor is not None else _CrossRunner(F, hop, device)
        y = p.run(v, c, per, int(lifter))
    return _both_channels(y, lens)


class _HarmRunner:
    """StftRoundTrip.harmonize from host arrays: x float32 [S][T], semitones [S][V][n_frames], gains [S][V], dry [S] -> float32 [S][T]."""

    def __init__(self, F, hop, device):
        self.F, self.hop, self.device = int(F), int(hop), device

    def run(self, x, semitones, gains, dry):
        def call(st, d_in, d_out):
            st.harmonize(d_in, d_out, semitones=semitones, gains=gains, dry=dry)
        return _one_shot(x, x.shape[1], self.F, self.hop, self.device, call)[0]


HARM_MAX_VOICES = 4


def pv_harmonize(voices, intervals, gains=None, dry=1.0, F=1024, hop=256, N=1024, stream=False, blocks_per_call=16, device=0, processor=None):
    """The phase-vocoder harmonizer on a batch (one stream per recording): beside every recording, `dry` times itself, V = 1 .. 4
    peak-locked copies shifted by `intervals` semitones (each within +-12) and mixed by `gains` (V values within [-4, 4]; None: 1 each).
    dry: one value or one per recording, within [-4, 4].  Batch (default): the one-shot call StftRoundTrip.harmonize on the recordings
    padded to a common length under the full overlap of 1024-point frames; stream: block by block through HarmonizerStream.run, its
    latency taken off.  Returns float32 [2][len] per recording (the signal on both channels).  `processor` (tests): an object with
    run(x, semitones [S][V][n_frames], gains [S][V], dry [S]) (batch) or latency and run(x, semitones [n_blocks][S][V], blocks_per_call,
    gains, dry) (stream) to use instead of the GPU."""
    S = _batch_size(voices)
    many = isinstance(intervals, (list, tuple)) or (isinstance(intervals, np.ndarray) and intervals.ndim == 1)
    iv = [float(v) for v in intervals] if many else []
    if not 1 <= len(iv) <= HARM_MAX_VOICES:
        raise ValueError("voices: 1 to 4 intervals expected")
    if not all(-12.0 <= v <= 12.0 for v in iv):
        raise ValueError("voices: intervals within +-12 semitones expected")
    V = len(iv)
    g = [1.0] * V if gains is None else [float(v) for v in gains]
    if len(g) != V:
        raise ValueError("gains: one gain per voice expected")
    if not all(-4.0 <= v <= 4.0 for v in g):
        raise ValueError("gains: values within [-4, 4] expected")
    per = _per_recording(dry, S, "dry", float, -4.0, 4.0, "dry: values within [-4, 4] expected")
    if int(F) != 1024:
        raise ValueError("harmonize: 1024-point frames expected (the harmonizer kernels are not built for 2048)")
    hop, N = int(hop), int(N)
    lens = _lengths(voices)
    gtab = np.tile(np.array(g, np.float64), (S, 1))
    if stream:
        x = _pack_mono(voices, lens, max(lens))
        from . import HarmonizerStream
        processor = _stream(processor, S, N, hop, device, HarmonizerStream, n_voices=V)
        nb = -(-(max(lens) + int(processor.latency)) // N)
        st = np.tile(np.array(iv, np.float64), (nb, S, 1))
        y = processor.run(x, semitones=st, blocks_per_call=int(blocks_per_call), gains=gtab, dry=per)
    else:
        T = _overlapped(max(lens), hop)
        x = _pack_mono(voices, lens, T)
        nF = (T - 1024) // hop + 1
        st = np.tile(np.array(iv, np.float64)[None, :, None], (S, 1, nF))
        p = processor if processor is not None else _HarmRunner(F, hop, device)
        y = p.run(x, st, gtab, per)
    return _both_channels(y, lens)


class _HarmKeyRunner:
    """StftRoundTrip.harmonize(degrees=...) from host arrays: x float32 [S][T], keys [S], degrees [S][V], gains [S][V], dry [S] ->
    (float32 [S][T], period int32 [S][nF], ratio float64 [S][V][nF])."""

    def __init__(self, hop, device):
        self.hop, self.device, self.fine = int(hop), device, False

    def set_fine(self, fine):
        """The fine tracker (StftRoundTrip.set_track_mode); run then also returns the refined periods float64 [S][nF]."""
        self.fine = bool(fine)

    def run(self, x, fs, keys, degrees, gains, dry):
        def call(st, d_in, d_out):
            if self.fine:
                st.set_track_mode(True)
            res = st.harmonize(d_in, d_out, degrees=degrees, sample_rate=float(fs), keys=[int(k) for k in keys], gains=gains, dry=dry)
            return res + (st.track_pitch(d_in, float(fs), keys=[int(k) for k in keys], with_fine_period=True)[2],) if self.fine else res
        y, tables = _one_shot(x, x.shape[1], 1024, self.hop, self.device, call)
        return (y,) + tuple(t.cpu().numpy() for t in tables)


class _StreamHarmKeyRunner:
    """HarmonizerStream.autoharm_device from host arrays: x float32 [S][n N] -> (y float32 [S][n N] with the harmonizer's latency still in
    front, period int32 [n][S], ratio float64 [n][S][V])."""

    def __init__(self, N, hop, hold, glide, device, blocks_per_call=16):
        self.N, self.hop, self.hold, self.glide, self.device, self.k = int(N), int(hop), int(hold), float(glide), device, int(blocks_per_call)
        self.fine = False

    def set_fine(self, fine):
        """The fine tracker (StreamingPitchTracker.set_fine); run then also returns the raw decisions' refined periods float64 [n][S], from
        a twin tracker fed the same blocks through process_device(with_fine_period=True)."""
        self.fine = bool(fine)

    def run(self, x, fs, keys, degrees, gains, dry):
        import torch
        from . import HarmonizerStream, StreamingPitchTracker
        S, N = x.shape[0], self.N
        nb = x.shape[1] // N
        dev = torch.device("cuda", self.device)
        hz = HarmonizerStream(S, N, degrees.shape[1], hop=self.hop, device=self.device)
        trk = StreamingPitchTracker(S, N, float(fs), hold_blocks=self.hold, glide=self.glide, device=self.device)
        twin = None
        try:
            d_in = torch.from_numpy(np.ascontiguousarray(x.reshape(S, nb, N).transpose(1, 0, 2), np.float32)).to(dev)
            d_out = torch.empty_like(d_in)
            if self.fine:
                twin = StreamingPitchTracker(S, N, float(fs), device=self.device)
                trk.set_fine(True)
            tables = [hz.autoharm_device(trk, d_in[b:b + self.k], d_out[b:b + self.k], degrees, n_blocks=min(self.k, nb - b), keys=[int(k) for k in keys],
                                         gains=gains, dry=dry) for b in range(0, nb, self.k)]
            fine = [twin.process_device(d_in[b:b + self.k], n_blocks=min(self.k, nb - b), keys=[int(k) for k in keys], with_fine_period=True)[2]
                    for b in range(0, nb, self.k)] if self.fine else None
            torch.cuda.synchronize(dev)
            y = d_out.cpu().numpy().transpose(1, 0, 2).reshape(S, nb * N)
            out = (np.ascontiguousarray(y), torch.cat([p for p, _ in tables]).cpu().numpy(), torch.cat([r for _, r in tables]).cpu().numpy())
            return out + (torch.cat(fine).cpu().numpy(),) if self.fine else out
        finally:
            if twin is not None:
                twin.close()
            trk.close()
            hz.close()


def pv_harmonize_key(voices, fs, degrees, key=12, gains=None, dry=1.0, hop=256, N=1024, stream=False, hold=0, glide=1.0, device=0, processor=None,
                     with_track=False, fine=False):
    """The KEY-AWARE harmonizer on a batch (one stream per recording): beside every recording, `dry` times itself, V = 1 .. 4 peak-locked
    voices at `degrees` (integers within +-12) steps of the key's note table from the note the pitch tracker chose -- scale degrees in a
    scale key (2 is a third above, 4 a fifth), semitones in the chromatic key 12.  Unvoiced frames take each voice's nominal interval.
    key: 0..12, one value or one per recording; gains, dry: as pv_harmonize's.  Batch (default): StftRoundTrip.harmonize(degrees=...) on the
    recordings padded as pv_autotune pads them; stream: block by block through HarmonizerStream.autoharm_device with a
    StreamingPitchTracker (hold, glide: its follow stage), the harmonizer's latency taken off.  Returns float32 [2][len] per recording;
    with_track: also period and ratio of the padded batch ([S][nF] and [S][V][nF]; stream: [n_blocks][S] and [n_blocks][S][V]).
    `processor` (tests): an object with run(x, fs, keys, degrees [S][V], gains [S][V], dry [S]) -> (y, period, ratio) instead of the GPU.
    fine: the fine tracker (the period refined below one sample; every voice's note index and ratio come from the refined pitch); the
    processor's set_fine(True) is called first, its run returns the refined periods ([S][nF]; stream: [n_blocks][S]) as a fourth item,
    and so does with_track."""
    S = _batch_size(voices)
    many = isinstance(degrees, (list, tuple)) or (isinstance(degrees, np.ndarray) and degrees.ndim == 1)
    dg = list(degrees) if many else []
    if not 1 <= len(dg) <= HARM_MAX_VOICES or not all(float(v) == int(v) for v in dg):
        raise ValueError("degrees: 1 to 4 integers expected")
    if not all(-12 <= int(v) <= 12 for v in dg):
        raise ValueError("degrees: steps within +-12 expected")
    V = len(dg)
    g = [1.0] * V if gains is None else [float(v) for v in gains]
    if len(g) != V:
        raise ValueError("gains: one gain per voice expected")
    if not all(-4.0 <= v <= 4.0 for v in g):
        raise ValueError("gains: values within [-4, 4] expected")
    per = _per_recording(dry, S, "dry", float, -4.0, 4.0, "dry: values within [-4, 4] expected")
    keys = _per_recording(key, S, "key", int, 0, 12, "key: 0..12 expected (12 = chromatic)")
    if not 8000.0 <= float(fs) <= 51200.0:
        raise ValueError("harmonize --degrees: sample rates from 8000 to 51200 Hz are served")
    if stream and not (int(N) >= 1 and 0 <= int(hold) <= 1 << 20 and 0.0 < float(glide) <= 1.0):
        raise ValueError("harmonize --stream: a block of at least one sample, 0 <= hold <= 2^20 blocks and 0 < glide <= 1 expected")
    lens = _lengths(voices)
    dtab, gtab = np.tile(np.array([int(v) for v in dg], np.int32), (S, 1)), np.tile(np.array(g, np.float64), (S, 1))
    if stream:
        T, lat = stream_tune_length(max(lens), N, hop)
        p = processor if processor is not None else _StreamHarmKeyRunner(N, hop, hold, glide, device)
    else:
        T, lat = tune_length(max(lens), fs, 1024, hop), 0
        p = processor if processor is not None else _HarmKeyRunner(hop, device)
    if fine:
        p.set_fine(True)
    y, *track = p.run(_pack_mono(voices, lens, T), float(fs), keys, dtab, gtab, per)
    if len(track) != (3 if fine else 2):
        raise ValueError("harmonize --degrees: the processor's run returned %d tables where %d were expected" % (len(track), 3 if fine else 2))
    outs = _both_channels(y, lens, lat)
    return (outs,) + tuple(track) if with_track else outs


def write_track_csv(path, fs, hop, period, ratio, n_samples=None, period_fine=None):
    """One recording's track: a line per frame with its start time in seconds, the period in samples (0 = unvoiced) and the correction in
    semitones (12 log2 ratio); n_samples: only the frames that start inside the recording.  period_fine (the fine tracker): a fourth
    column, the refined period in samples."""
    with open(path, "w") as f:
        f.write("time_s,period,semitones\n" if period_fine is None else "time_s,period,semitones,period_fine\n")
        for i, (p, r) in enumerate(zip(period, ratio)):
            if n_samples is not None and i * int(hop) >= int(n_samples) and i > 0:
                break
            f.write("%.6f,%d,%.6f" % (i * int(hop) / float(fs), int(p), 12.0 * np.log2(float(r))))
            f.write("\n" if period_fine is None else ",%.6f\n" % float(period_fine[i]))


# ---- command line ---------------------------------------------------------------------------------------------------------

def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m vocoderproject_amd.offline", description=__doc__.split("\n\n")[0])
    ap.add_argument("flow", choices=["pitch", "vocode", "both", "pvshift", "stretch", "pvtune", "pvcross", "harmonize"])
    ap.add_argument("inputs", nargs="+", help="voice recordings (WAV; channel 0 is used, like the notebook)")
    ap.add_argument("--carrier", action="append", default=None,
                    help="side-chain recording(s) for vocode/both, carrier(s) for pvcross (channel 0): one for all voices or one per voice")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--key", type=int, default=12, help="keyPitch 0..12 (12 = chromatic, the plugin's default)")
    ap.add_argument("--shift", type=float, default=None, help="fixed interval in semitones instead of the key correction")
    ap.add_argument("--glide", default=None, metavar="A:B",
                    help="pvshift: a linear glide from A to B semitones over each recording, one value per block, instead of --shift; "
                         "pvtune --stream: one number in (0, 1], the fraction of the way to its target the ratio moves per block (default 1)")
    ap.add_argument("--stream", action="store_true", help="pvtune: block by block through the streaming tracker and phase vocoder (--block, --hold, --glide); "
                                                          "pvshift --formant: block by block instead of the one-shot call")
    ap.add_argument("--formant", type=float, nargs="?", const=0.0, default=None, metavar="ST",
                    help="pvshift, pvtune: keep the spectral envelope apart from the pitch and move the formants by ST semitones "
                         "(no value: 0, they stay where they were).  The value is optional, so put the flag BEHIND the input files or "
                         "in front of another option: `--formant a.wav` would read a.wav as the interval")
    ap.add_argument("--locked", action="store_true",
                    help="pvshift (--shift or --glide), pvtune [--stream], stretch: the peak-locked phase vocoder -- a spectral peak's whole region moves "
                         "and turns as one, so tones keep their level (1024-point frames; not together with --formant)")
    ap.add_argument("--subbin", action="store_true",
                    help="pvshift, pvtune [--stream], together with --locked: a peak's region moves by the real-valued offset of its interpolated "
                         "centre and the spectrum is interpolated (six taps), so shifted tones keep their level at every interval")
    ap.add_argument("--depth", type=float, default=1.0, help="pvcross: 0 (the carrier unchanged) to 1 (the voice's spectral envelope in full)")
    ap.add_argument("--lifter", type=int, default=32, help="--formant, pvcross: length of the cepstral lifter in samples, 4 to 64 (short: a smoother envelope)")
    ap.add_argument("--voices", default=None, metavar="ST[,ST..]",
                    help="harmonize: 1 to 4 intervals in semitones, each within +-12, comma-separated (a list that starts below zero as --voices=-5,4)")
    ap.add_argument("--degrees", default=None, metavar="D[,D..]",
                    help="harmonize, instead of --voices: 1 to 4 voices at integer steps of --key's note table from the tracked note, each within "
                         "+-12 (scale degrees in a scale key: 2 a third above, 4 a fifth; semitones in key 12); --stream, --hold, --glide and "
                         "--track-csv as pvtune's")
    ap.add_argument("--gains", default=None, metavar="G[,G..]", help="harmonize: one gain per voice within [-4, 4] (default: 1 each)")
    ap.add_argument("--dry", type=float, default=1.0, help="harmonize: gain of the unshifted signal beside the voices, within [-4, 4] (default 1)")
    ap.add_argument("--hold", type=int, default=0, help="pvtune --stream: unvoiced blocks over which the last voiced ratio is kept")
    ap.add_argument("--stretch", type=float, default=None, help="stretch: output duration / input duration, 0.25 to 4 (--shift: semitones on top)")
    ap.add_argument("--transients", type=float, nargs="?", const=0.2, default=None, metavar="THR",
                    help="stretch, together with --locked: keep attacks -- a frame whose spectral flux is a local maximum of at least THR of its "
                         "spectral mass (0 to 1; no value: 0.2) is an onset, the frames around it are read without stretch and the phases "
                         "restart there.  The value is optional, so put the flag BEHIND the input files or in front of another option")
    ap.add_argument("--span", type=int, default=None, metavar="K", help="--transients: frames kept either side of an onset, 1 to 8 (default: frame / (2 hop))")
    ap.add_argument("--frame", type=int, default=1024, help="stretch, pvtune: frame length (1024 or 2048)")
    ap.add_argument("--track-csv", action="store_true", help="pvtune: also write NAME_pvtune.csv per recording (time, period, correction in semitones per frame)")
    ap.add_argument("--fine", action="store_true",
                    help="pvtune [--stream], harmonize --degrees [--stream]: the fine pitch tracker -- the period refined below one sample by a "
                         "parabola through the difference function's minimum, the note looked up on the refined pitch; --track-csv gains a "
                         "fourth column, the refined period")
    ap.add_argument("--lpc-voice", type=int, default=40)
    ap.add_argument("--lpc-synth", type=int, default=5)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256, help="pvshift: hop of the 1024-point frames (64, 128, 256 or 512)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--fast", action="store_true", help="VP_IIR_FAST + certified cross-correlation YIN")
    # (a glide that starts below zero, "--glide -12:12", looks like an option to argparse: hand it over as --glide=-12:12)
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):
        if argv[i] == "--glide" and ":" in argv[i + 1]:
            argv[i:i + 2] = ["--glide=" + argv[i + 1]]
            break
    a = ap.parse_args(argv)
    if a.flow == "pvcross":
        for flag, given in (("--formant", a.formant is not None), ("--locked", a.locked), ("--subbin", a.subbin), ("--shift", a.shift is not None), ("--glide", a.glide is not None),
                            ("--stretch", a.stretch is not None)):
            if given:
                raise SystemExit(f"{flag}: pvcross does not take it (the cross-synthesis moves neither pitch nor time)")
    if a.flow == "harmonize":
        # (--degrees: the track and, streamed, the tracker's follow stage are pvtune's)
        tracked = ((("--glide", a.glide is not None and not a.stream), ("--hold", a.hold != 0 and not a.stream)) if a.degrees is not None else
                   (("--glide", a.glide is not None), ("--track-csv", a.track_csv), ("--hold", a.hold != 0)))
        for flag, given in (("--formant", a.formant is not None), ("--locked", a.locked), ("--subbin", a.subbin), ("--shift", a.shift is not None),
                            ("--stretch", a.stretch is not None), ("--carrier", a.carrier is not None)) + tracked:
            if given and a.degrees is not None:
                raise SystemExit(f"{flag}: harmonize --degrees does not take it (its voices are peak-locked copies at degrees of the key)")
            if given:
                raise SystemExit(f"{flag}: harmonize does not take it (its voices are peak-locked copies at the fixed intervals of --voices)")
        if a.voices is not None and a.degrees is not None:
            raise SystemExit("--voices and --degrees exclude each other: fixed intervals or degrees of the key")
        if a.voices is None and a.degrees is None:
            raise SystemExit("harmonize needs --voices ST[,ST..] or --degrees D[,D..]")
    elif a.voices is not None or a.gains is not None:
        raise SystemExit("--voices, --gains: harmonize takes them")
    elif a.degrees is not None:
        raise SystemExit("--degrees: harmonize takes it")
    if a.formant is not None and a.flow not in ("pvshift", "pvtune"):
        raise SystemExit("--formant: pvshift and pvtune take it")
    if a.locked and a.flow not in ("pvshift", "pvtune", "stretch"):
        raise SystemExit("--locked: pvshift, pvtune and stretch take it")
    if a.locked and a.formant is not None:
        raise SystemExit("--locked and --formant exclude each other: formant correction on top of peak locking is not built")
    if a.subbin and a.flow == "stretch":
        raise SystemExit("--subbin: stretch does not take it (the locked time stretch keeps integer offsets)")
    if a.subbin and a.flow not in ("pvshift", "pvtune"):
        raise SystemExit("--subbin: pvshift and pvtune take it")
    if a.subbin and not a.locked:
        raise SystemExit("--subbin: valid only together with --locked (the sub-bin region offsets are a variant of the peak-locked call)")
    if a.transients is not None and a.flow != "stretch":
        raise SystemExit("--transients: stretch takes it")
    if a.transients is not None and not a.locked:
        raise SystemExit("--transients: valid only together with --locked (the phase reset is a variant of the peak-locked time stretch)")
    if a.span is not None and a.transients is None:
        raise SystemExit("--span: valid only together with --transients")
    if a.fine and not (a.flow == "pvtune" or (a.flow == "harmonize" and a.degrees is not None)):
        raise SystemExit("--fine: pvtune and harmonize --degrees take it (the flows that track the pitch)")
    fkw = {} if a.formant is None else dict(formant=a.formant, lifter=a.lifter)
    if a.locked:
        fkw["locked"] = True
    if a.subbin:
        fkw["subbin"] = True
    if a.fine and a.flow == "pvtune":
        fkw["fine"] = True

    recs = [read_wav(f) for f in a.inputs]
    fs = recs[0][0]
    if any(r[0] != fs for r in recs):
        raise SystemExit("all recordings of a batch must share one sample rate (one prepareToPlay)")
    voices = [r[1][0] for r in recs]
    if a.flow == "pvcross":
        if not a.carrier:
            raise SystemExit("pvcross needs --carrier")
        cs = [read_wav(f) for f in a.carrier]
        if any(c[0] != fs for c in cs):
            raise SystemExit("carrier sample rate differs from the voices'")
        if len(cs) not in (1, len(voices)):
            raise SystemExit("--carrier: give one, or one per voice")
        try:
            outs = pv_cross(voices, [c[1][0] for c in cs], depth=a.depth, lifter=a.lifter, hop=a.hop, N=a.block, stream=a.stream, device=a.device)
        except ValueError as e:
            raise SystemExit(str(e))
        return _write_outputs(a, fs, outs)
    if a.flow == "harmonize" and a.degrees is not None:
        try:
            dg = [int(v) for v in a.degrees.split(",")]
            gains = None if a.gains is None else [float(v) for v in a.gains.split(",")]
            glide = 1.0 if a.glide is None else float(a.glide)
        except ValueError:
            raise SystemExit("--degrees: comma-separated integers expected; --gains: numbers; --glide: one number in (0, 1]")
        try:
            outs, period, ratio, *fine = pv_harmonize_key(voices, fs, dg, key=a.key, gains=gains, dry=a.dry, hop=a.hop, N=a.block, stream=a.stream,
                                                          hold=a.hold, glide=glide, device=a.device, with_track=True, **({"fine": True} if a.fine else {}))
        except ValueError as e:
            raise SystemExit(str(e))
        rc = _write_outputs(a, fs, outs)
        if a.track_csv:                                                            # one file per recording and voice: the voice's ratio per frame / block
            step = a.block if a.stream else a.hop
            for s, f in enumerate(a.inputs):
                for v in range(len(dg)):
                    out = os.path.join(a.out_dir, os.path.splitext(os.path.basename(f))[0] + f"_harmonize_v{v}.csv")
                    write_track_csv(out, fs, step, period[:, s] if a.stream else period[s], ratio[:, s, v] if a.stream else ratio[s, v],
                                    n_samples=voices[s].shape[-1], **({"period_fine": fine[0][:, s] if a.stream else fine[0][s]} if fine else {}))
                    print(out)
        return rc
    if a.flow == "harmonize":
        try:
            iv = [float(v) for v in a.voices.split(",")]
            gains = None if a.gains is None else [float(v) for v in a.gains.split(",")]
        except ValueError:
            raise SystemExit("--voices, --gains: comma-separated numbers expected")
        try:
            outs = pv_harmonize(voices, iv, gains=gains, dry=a.dry, hop=a.hop, N=a.block, stream=a.stream, device=a.device)
        except ValueError as e:
            raise SystemExit(str(e))
        return _write_outputs(a, fs, outs)
    if a.flow == "stretch":
        if a.stretch is None:
            raise SystemExit("stretch needs --stretch FACTOR")
        try:
            outs = pv_stretch(voices, a.stretch, shift=0.0 if a.shift is None else a.shift, F=a.frame, hop=a.hop, device=a.device,
                              **({"locked": True} if a.locked else {}), **({} if a.transients is None else {"transients": a.transients, "span": a.span}))
        except ValueError as e:
            raise SystemExit(str(e))
        return _write_outputs(a, fs, outs)
    if a.flow == "pvtune":
        try:
            if a.stream:
                try:
                    glide = 1.0 if a.glide is None else float(a.glide)
                except ValueError:
                    raise SystemExit("pvtune --stream --glide: one number in (0, 1] expected")
                outs, period, ratio, *fine = pv_autotune_stream(voices, fs, key=a.key, N=a.block, hop=a.hop, F=a.frame, hold=a.hold, glide=glide,
                                                                device=a.device, with_track=True, **fkw)
                period, ratio, step, fine = period.T, ratio.T, a.block, [t.T for t in fine]   # a row per block, at the block's start
            else:
                outs, period, ratio, *fine = pv_autotune(voices, fs, key=a.key, F=a.frame, hop=a.hop, device=a.device, with_track=True, **fkw)
                step = a.hop
        except ValueError as e:
            raise SystemExit(str(e))
        rc = _write_outputs(a, fs, outs)
        if a.track_csv:
            for s, f in enumerate(a.inputs):
                out = os.path.join(a.out_dir, os.path.splitext(os.path.basename(f))[0] + "_pvtune.csv")
                write_track_csv(out, fs, step, period[s], ratio[s], n_samples=voices[s].shape[-1], **({"period_fine": fine[0][s]} if fine else {}))
                print(out)
        return rc
    if a.flow == "pvshift":
        if (a.shift is None) == (a.glide is None):
            raise SystemExit("pvshift needs --shift or --glide A:B")
        if a.glide is not None:
            try:
                g0, g1 = (float(v) for v in a.glide.split(":"))
            except ValueError:
                raise SystemExit("--glide: A:B expected, two intervals in semitones")
            try:
                outs = pv_glide(voices, g0, g1, N=a.block, hop=a.hop, device=a.device, **fkw)     # (a glide is streamed: one interval per block)
            except ValueError as e:
                raise SystemExit(str(e))
        elif a.locked:
            try:
                outs = pv_shift_locked(voices, a.shift, N=a.block, hop=a.hop, device=a.device, **({"subbin": True} if a.subbin else {}))
            except ValueError as e:
                raise SystemExit(str(e))
        elif a.formant is not None:
            try:
                outs = pv_shift_formant(voices, a.shift, N=a.block, hop=a.hop, device=a.device, stream=a.stream, **fkw)
            except ValueError as e:
                raise SystemExit(str(e))
        else:
            outs = pv_shift(voices, a.shift, N=a.block, hop=a.hop, device=a.device)
        return _write_outputs(a, fs, outs)
    carriers = None
    if a.flow != "pitch":
        if not a.carrier:
            raise SystemExit("vocode/both need --carrier")
        cs = [read_wav(f) for f in a.carrier]
        if any(c[0] != fs for c in cs):
            raise SystemExit("carrier sample rate differs from the voices'")
        if len(cs) == 1:
            cs = cs * len(voices)
        if len(cs) != len(voices):
            raise SystemExit("--carrier: give one, or one per voice")
        carriers = [c[1][:2] if c[1].shape[0] >= 2 else c[1][0] for c in cs]
    params = dict(keyPitch=a.key, lpcVoice=a.lpc_voice, lpcSynth=a.lpc_synth)
    outs = render(voices, carriers, fs, pitch=a.flow != "vocode", vocoder=a.flow != "pitch", params=params, shift=a.shift,
                  N=a.block, device=a.device, iir_mode="fast" if a.fast else "exact", yin_mode="xcorr" if a.fast else "direct")
    return _write_outputs(a, fs, outs)


def _write_outputs(a, fs, outs):
    os.makedirs(a.out_dir, exist_ok=True)
    for f, y in zip(a.inputs, outs):
        out = os.path.join(a.out_dir, os.path.splitext(os.path.basename(f))[0] + f"_{a.flow}.wav")
        write_wav(out, fs, y)
        print(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
