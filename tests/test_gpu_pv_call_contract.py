"""The argument contract of every vp_stft_* / vp_pv_* processing and autotune entry (include/vp_amd.h), one table: for each entry every
pointer null in turn, every scalar out of its range in turn and the pairs of simultaneous errors whose winner callers can see -- the code
returned and the exact vp_stft_last_error text, or that the text did not change.  No case launches a kernel.  Afterwards one valid
call on the one-shot handle and on each stream the cases used (phase vocoder, cross-synthesis, harmonizer) equals the same call on fresh
handles, bit for bit: a refused call leaves nothing behind.
Below the table, the pending changes of the three streaming handles at the edges of VP_PV_MAX_UPDATES = 16 per launch: 15, 16, 17, 32 and
33 of them in front of one call reach none, one and two update-only launches with a one-entry and a full carried group."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

pytestmark = pytest.mark.gpu

INVALID, GEOMETRY = -1, -4                                    # include/vp_amd.h VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY
S, T, N, NB, V = 2, 4096, 64, 32, 2
NAN = float("nan")
KEEP = None                                                   # vp_stft_last_error keeps the text it had

LOCK_NULL = "locked: null input, output or ratio table"
LOCK_2K = "locked: 2048-point frames are not built (the peak-locked stage exists for 1024-point frames only)"
FORM_NULL = "formant: null input, output or ratio table"
FORM_LIFTER = "formant: lifter outside 4 .. 64 samples"
FORM_2K = "formant: 2048-point frames are not built (the envelope needs a wavefront's exchange buffer to hold the frame's 1025 bins; it holds 1024 doubles)"
SL_NULL = "stretch locked: null input, position table, output or ratio table"
SL_SHORT = "stretch locked: the input row is shorter than one frame"
SL_2K = "stretch locked: 2048-point frames are not built (the peak-locked stage exists for 1024-point frames only)"
SUB_NULL = "locked subbin: null input, output or ratio table"
SUB_2K = "locked subbin: 2048-point frames are not built (the peak-locked stage exists for 1024-point frames only)"
HARM_NULL = "harmonize: null input, output or ratio table"
HARM_VOICES = "harmonize: the number of voices is outside 1 .. 4"
HARM_2K = "harmonize: 2048-point frames are not built (the peak-locked stage exists for 1024-point frames only)"
CROSS_NULL = "cross: null voice, carrier or output"
CROSS_LIFTER = "cross: lifter outside 4 .. 64 samples"
CROSS_2K = "cross: 2048-point frames are not built (the envelope needs a wavefront's exchange buffer to hold the frame's 1025 bins; it holds 1024 doubles)"
TRK_NULL = "pitch tracker: null input"
TRK_OUT = "pitch tracker: period and ratio outputs are both null"
TRK_FS = "pitch tracker: sample rate outside 8000 .. 51200 Hz"
TRK_SHORT = "pitch tracker: rows of 1024 samples are shorter than frame_len + tauMax = 1465"
TUNE_NULL = "autotune: null output or ratio table (the table is result and scratch)"

# entry -> its arguments, by the names of the valid values below (p: one-shot handle; pv, trk, xs, hz: stream, tracker, cross-synthesis and
# harmonizer streams; s*: the streams' slabs; h*: the harmonizer's ratio tables; the cross-synthesis entries' voice is `in` / `sin`)
ENTRIES = {
    "vp_stft_roundtrip": ("p", "in", "out", "mag", "stream"),
    "vp_stft_pitch_shift": ("p", "in", "out", "semitones", "stream"),
    "vp_stft_pitch_shift_curve": ("p", "in", "out", "ratio", "stream"),
    "vp_stft_pitch_shift_locked": ("p", "in", "out", "ratio", "stream"),
    "vp_stft_pitch_shift_locked_subbin": ("p", "in", "out", "ratio", "stream"),
    "vp_stft_harmonize": ("p", "in", "out", "n_voices", "hratio", "gain", "dry", "stream"),
    "vp_stft_pitch_shift_formant": ("p", "in", "out", "ratio", "formant", "lifter", "stream"),
    "vp_stft_cross_synth": ("p", "in", "carrier", "out", "depth", "lifter", "stream"),
    "vp_stft_time_stretch": ("p", "in", "n_in", "pos", "out", "semitones", "stream"),
    "vp_stft_time_stretch_locked": ("p", "in", "n_in", "pos", "out", "ratio", "stream"),
    "vp_stft_track_pitch": ("p", "in", "fs", "key", "period", "ratio", "stream"),
    "vp_stft_autotune": ("p", "in", "out", "fs", "key", "period", "ratio", "stream"),
    "vp_stft_autotune_formant": ("p", "in", "out", "fs", "key", "period", "ratio", "formant", "lifter", "stream"),
    "vp_pv_process_blocks_device": ("pv", "sin", "sout", "n_blocks", "stream"),
    "vp_pv_process_blocks_curve_device": ("pv", "sin", "sout", "sratio", "n_blocks", "stream"),
    "vp_pv_process_blocks_locked_device": ("pv", "sin", "sout", "sratio", "n_blocks", "stream"),
    "vp_pv_process_blocks_locked_subbin_device": ("pv", "sin", "sout", "sratio", "n_blocks", "stream"),
    "vp_pv_process_blocks_formant_device": ("pv", "sin", "sout", "sratio", "formant", "lifter", "n_blocks", "stream"),
    "vp_xs_process_blocks_device": ("xs", "sin", "scarrier", "sout", "depth", "lifter", "n_blocks", "stream"),
    "vp_hz_process_blocks_device": ("hz", "sin", "sout", "shratio", "gain", "dry", "n_blocks", "stream"),
    "vp_pv_process_block": ("pv", "hin", "hout"),
    "vp_pv_tracker_process_blocks_device": ("trk", "sin", "key", "speriod", "sratio", "n_blocks", "stream"),
    "vp_pv_autotune_blocks_device": ("pv", "trk", "sin", "sout", "key", "speriod", "sratio", "n_blocks", "stream"),
    "vp_pv_autotune_blocks_formant_device": ("pv", "trk", "sin", "sout", "key", "speriod", "sratio", "formant", "lifter", "n_blocks", "stream"),
}

H2K, HSHORT, PV3 = "@h2k", "@hshort", "@pv3"                  # the 2048/512 handle, the T = 1024 handle, the stream of three


def nulls(entry, names, code=INVALID, msg=KEEP):
    return [(entry, {n: None}, code, msg) for n in names]


def each(entry, name, values, code=INVALID, msg=KEEP):
    return [(entry, {name: v}, code, msg) for v in values]


SEMIS, LIFTERS, RATES, BLOCKS = (12.5, -12.5, NAN), (3, 65), (7999.0, NAN), (0, (1 << 28) // N + 1)

CASES = (
    nulls("vp_stft_roundtrip", ("p", "in", "out"))
    + nulls("vp_stft_pitch_shift", ("p", "in", "out")) + each("vp_stft_pitch_shift", "semitones", SEMIS)
    + [("vp_stft_pitch_shift", {"in": None, "semitones": NAN}, INVALID, KEEP)]
    + nulls("vp_stft_pitch_shift_curve", ("p", "in", "out", "ratio"))
    # vp_stft_pitch_shift_locked: pointers, frame length
    + nulls("vp_stft_pitch_shift_locked", ("p",)) + nulls("vp_stft_pitch_shift_locked", ("in", "out", "ratio"), msg=LOCK_NULL)
    + [("vp_stft_pitch_shift_locked", {"p": H2K}, GEOMETRY, LOCK_2K), ("vp_stft_pitch_shift_locked", {"p": H2K, "ratio": None}, INVALID, LOCK_NULL)]
    # vp_stft_pitch_shift_formant: pointers, lifter, frame length
    + nulls("vp_stft_pitch_shift_formant", ("p",)) + nulls("vp_stft_pitch_shift_formant", ("in", "out", "ratio"), msg=FORM_NULL)
    + each("vp_stft_pitch_shift_formant", "lifter", LIFTERS, msg=FORM_LIFTER)
    + [("vp_stft_pitch_shift_formant", {"p": H2K}, GEOMETRY, FORM_2K), ("vp_stft_pitch_shift_formant", {"p": H2K, "formant": None}, GEOMETRY, FORM_2K),
       ("vp_stft_pitch_shift_formant", {"out": None, "lifter": 3}, INVALID, FORM_NULL), ("vp_stft_pitch_shift_formant", {"p": H2K, "lifter": 65}, INVALID, FORM_LIFTER),
       ("vp_stft_pitch_shift_formant", {"p": None, "lifter": 3}, INVALID, KEEP)]
    + nulls("vp_stft_time_stretch", ("p", "in", "pos", "out")) + each("vp_stft_time_stretch", "n_in", (1023,)) + each("vp_stft_time_stretch", "semitones", SEMIS)
    + [("vp_stft_time_stretch", {"p": H2K, "n_in": 2047}, INVALID, KEEP)]
    # vp_stft_time_stretch_locked: pointers, row length, frame length
    + nulls("vp_stft_time_stretch_locked", ("p",)) + nulls("vp_stft_time_stretch_locked", ("in", "pos", "out", "ratio"), msg=SL_NULL)
    + each("vp_stft_time_stretch_locked", "n_in", (1023, 0, -1), msg=SL_SHORT)
    + [("vp_stft_time_stretch_locked", {"p": H2K, "n_in": 2048}, GEOMETRY, SL_2K), ("vp_stft_time_stretch_locked", {"p": H2K, "n_in": 2047}, INVALID, SL_SHORT),
       ("vp_stft_time_stretch_locked", {"pos": None, "n_in": 1023}, INVALID, SL_NULL), ("vp_stft_time_stretch_locked", {"p": H2K, "n_in": 2048, "in": None}, INVALID, SL_NULL)]
    # vp_stft_track_pitch: handle, input, outputs, sample rate, row length
    + nulls("vp_stft_track_pitch", ("p",)) + nulls("vp_stft_track_pitch", ("in",), msg=TRK_NULL)
    + [("vp_stft_track_pitch", {"period": None, "ratio": None}, INVALID, TRK_OUT)] + each("vp_stft_track_pitch", "fs", RATES + (51201.0,), msg=TRK_FS)
    + [("vp_stft_track_pitch", {"p": HSHORT}, GEOMETRY, TRK_SHORT), ("vp_stft_track_pitch", {"p": HSHORT, "fs": 7999.0}, INVALID, TRK_FS),
       ("vp_stft_track_pitch", {"in": None, "period": None, "ratio": None, "fs": NAN}, INVALID, TRK_NULL),
       ("vp_stft_track_pitch", {"period": None, "ratio": None, "fs": NAN}, INVALID, TRK_OUT)]
)
for _e in ("vp_stft_autotune", "vp_stft_autotune_formant"):
    # output and ratio table first (with a handle), then the tracker's checks; the formant entry: then lifter and frame length
    CASES += (nulls(_e, ("p",)) + nulls(_e, ("out", "ratio"), msg=TUNE_NULL) + nulls(_e, ("in",), msg=TRK_NULL) + each(_e, "fs", RATES, msg=TRK_FS)
              + [(_e, {"p": HSHORT}, GEOMETRY, TRK_SHORT), (_e, {"p": None, "out": None}, INVALID, KEEP), (_e, {"out": None, "in": None}, INVALID, TUNE_NULL),
                 (_e, {"ratio": None, "period": None}, INVALID, TUNE_NULL), (_e, {"ratio": None, "fs": 7999.0}, INVALID, TUNE_NULL),
                 (_e, {"in": None, "fs": 7999.0}, INVALID, TRK_NULL), (_e, {"p": HSHORT, "out": None}, INVALID, TUNE_NULL)])
CASES += (
    each("vp_stft_autotune_formant", "lifter", LIFTERS, msg=FORM_LIFTER)
    + [("vp_stft_autotune_formant", {"p": H2K}, GEOMETRY, FORM_2K), ("vp_stft_autotune_formant", {"p": H2K, "lifter": 3}, INVALID, FORM_LIFTER),
       ("vp_stft_autotune_formant", {"fs": NAN, "lifter": 3}, INVALID, TRK_FS), ("vp_stft_autotune_formant", {"p": HSHORT, "lifter": 65}, GEOMETRY, TRK_SHORT),
       ("vp_stft_autotune_formant", {"out": None, "lifter": 3}, INVALID, TUNE_NULL), ("vp_stft_autotune_formant", {"in": None, "lifter": 3}, INVALID, TRK_NULL)]
    # the streaming entries keep no message: the code alone
    + nulls("vp_pv_process_blocks_device", ("pv", "sin", "sout")) + each("vp_pv_process_blocks_device", "n_blocks", BLOCKS)
)
for _e in ("vp_pv_process_blocks_curve_device", "vp_pv_process_blocks_locked_device", "vp_pv_process_blocks_locked_subbin_device",
           "vp_pv_process_blocks_formant_device"):
    CASES += nulls(_e, ("pv", "sin", "sout", "sratio")) + each(_e, "n_blocks", BLOCKS)
CASES += (
    each("vp_pv_process_blocks_formant_device", "lifter", LIFTERS)
    + [("vp_pv_process_blocks_formant_device", {"sin": None, "lifter": 3}, INVALID, KEEP), ("vp_pv_process_blocks_formant_device", {"n_blocks": 0, "lifter": 65}, INVALID, KEEP)]
    + nulls("vp_pv_process_block", ("pv", "hin", "hout"))
    + nulls("vp_pv_tracker_process_blocks_device", ("trk", "sin")) + each("vp_pv_tracker_process_blocks_device", "n_blocks", BLOCKS)
    + [("vp_pv_tracker_process_blocks_device", {"speriod": None, "sratio": None}, INVALID, KEEP)]
)
for _e in ("vp_pv_autotune_blocks_device", "vp_pv_autotune_blocks_formant_device"):
    # handle, output and ratio table (the formant entry: and the lifter), then the tracker's checks, then the pair's geometry
    CASES += (nulls(_e, ("pv", "trk", "sin", "sout", "sratio")) + each(_e, "n_blocks", BLOCKS)
              + [(_e, {"pv": PV3}, GEOMETRY, KEEP), (_e, {"pv": PV3, "n_blocks": 0}, INVALID, KEEP), (_e, {"pv": PV3, "sout": None}, INVALID, KEEP),
                 (_e, {"pv": PV3, "sin": None}, INVALID, KEEP), (_e, {"pv": PV3, "trk": None}, INVALID, KEEP)])
CASES += (each("vp_pv_autotune_blocks_formant_device", "lifter", LIFTERS)
          + [("vp_pv_autotune_blocks_formant_device", {"pv": PV3, "lifter": 3}, INVALID, KEEP), ("vp_pv_autotune_blocks_formant_device", {"trk": None, "lifter": 65}, INVALID, KEEP)])
CASES += (
    # vp_stft_pitch_shift_locked_subbin: the locked entry's rows under its own name
    nulls("vp_stft_pitch_shift_locked_subbin", ("p",)) + nulls("vp_stft_pitch_shift_locked_subbin", ("in", "out", "ratio"), msg=SUB_NULL)
    + [("vp_stft_pitch_shift_locked_subbin", {"p": H2K}, GEOMETRY, SUB_2K), ("vp_stft_pitch_shift_locked_subbin", {"p": H2K, "ratio": None}, INVALID, SUB_NULL)]
    # vp_stft_harmonize: pointers (the gain and dry tables may be null), voice count, frame length
    + nulls("vp_stft_harmonize", ("p",)) + nulls("vp_stft_harmonize", ("in", "out", "hratio"), msg=HARM_NULL)
    + each("vp_stft_harmonize", "n_voices", (0, 5, -1), msg=HARM_VOICES)
    + [("vp_stft_harmonize", {"p": H2K}, GEOMETRY, HARM_2K), ("vp_stft_harmonize", {"p": H2K, "gain": None, "dry": None}, GEOMETRY, HARM_2K),
       ("vp_stft_harmonize", {"in": None, "n_voices": 0}, INVALID, HARM_NULL), ("vp_stft_harmonize", {"p": H2K, "n_voices": 5}, INVALID, HARM_VOICES),
       ("vp_stft_harmonize", {"p": None, "n_voices": 0}, INVALID, KEEP)]
    # vp_stft_cross_synth: pointers (the depth table may be null), lifter, frame length
    + nulls("vp_stft_cross_synth", ("p",)) + nulls("vp_stft_cross_synth", ("in", "carrier", "out"), msg=CROSS_NULL)
    + each("vp_stft_cross_synth", "lifter", LIFTERS, msg=CROSS_LIFTER)
    + [("vp_stft_cross_synth", {"p": H2K}, GEOMETRY, CROSS_2K), ("vp_stft_cross_synth", {"p": H2K, "depth": None}, GEOMETRY, CROSS_2K),
       ("vp_stft_cross_synth", {"out": None, "lifter": 3}, INVALID, CROSS_NULL), ("vp_stft_cross_synth", {"p": H2K, "lifter": 65}, INVALID, CROSS_LIFTER),
       ("vp_stft_cross_synth", {"p": None, "lifter": 3}, INVALID, KEEP)]
    # the cross-synthesis and harmonizer streams: the code alone, like the other streaming entries
    + nulls("vp_xs_process_blocks_device", ("xs", "sin", "scarrier", "sout")) + each("vp_xs_process_blocks_device", "n_blocks", BLOCKS)
    + each("vp_xs_process_blocks_device", "lifter", LIFTERS)
    + [("vp_xs_process_blocks_device", {"scarrier": None, "lifter": 3}, INVALID, KEEP), ("vp_xs_process_blocks_device", {"depth": None, "n_blocks": 0}, INVALID, KEEP),
       ("vp_xs_process_blocks_device", {"depth": None, "lifter": 65}, INVALID, KEEP)]
    + nulls("vp_hz_process_blocks_device", ("hz", "sin", "sout", "shratio")) + each("vp_hz_process_blocks_device", "n_blocks", BLOCKS)
    + [("vp_hz_process_blocks_device", {"gain": None, "dry": None, "n_blocks": 0}, INVALID, KEEP),
       ("vp_hz_process_blocks_device", {"gain": None, "dry": None, "shratio": None}, INVALID, KEEP)]
)


def _curve_call(st, d_in, d_ratio):
    d_out = torch.full_like(d_in, NAN)
    st.pitch_shift_curve(d_in, d_out, d_ratio=d_ratio)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _stream_call(pv, d_in, d_ratio):
    d_out = torch.full_like(d_in, NAN)
    pv.process_device(d_in, d_out, n_blocks=NB, d_ratio=d_ratio)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _cross_call(xs, d_voice, d_carrier):
    d_out = torch.full_like(d_voice, NAN)
    xs.process_device(d_voice, d_carrier, d_out, n_blocks=NB, depth=None)      # (the library's NULL depth table)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _harm_call(hz, d_in, d_ratio):
    d_out = torch.full_like(d_in, NAN)
    hz.process_device(d_in, d_out, n_blocks=NB, d_ratio=d_ratio)               # (the library's NULL gain and dry tables)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def test_every_entry_refuses_every_wrong_argument_with_its_code_and_message_and_leaves_the_handles_as_they_were():
    from vocoderproject_amd import CrossSynthStream, HarmonizerStream, PhaseVocoderStream, StftRoundTrip, StreamingPitchTracker
    h1, h2k, hshort = StftRoundTrip(S, T, 1024, 256), StftRoundTrip(S, T, 2048, 512), StftRoundTrip(S, 1024, 1024, 256)
    pv, trk, pv3 = PhaseVocoderStream(S, N), StreamingPitchTracker(S, N, 44100.0), PhaseVocoderStream(3, N)
    xs, hz = CrossSynthStream(S, N), HarmonizerStream(S, N, V)
    L = h1.L
    rng = np.random.default_rng(7)
    d_in = torch.from_numpy(rng.normal(0, 0.2, (S, T)).astype(np.float32)).cuda()
    d_sin = torch.from_numpy(rng.normal(0, 0.2, (NB, S, N)).astype(np.float32)).cuda()
    d_ratio = torch.from_numpy(2.0 ** (rng.uniform(-12, 12, (S, h1.n_frames)) / 12)).cuda()
    d_sratio = torch.from_numpy(2.0 ** (rng.uniform(-12, 12, (NB, S)) / 12)).cuda()
    d_scarrier = torch.from_numpy(rng.normal(0, 0.2, (NB, S, N)).astype(np.float32)).cuda()
    d_shratio = torch.from_numpy(2.0 ** (rng.uniform(-12, 12, (NB, S, V)) / 12)).cuda()
    bufs = dict(out=torch.empty_like(d_in), pos=torch.zeros((S, h1.n_frames), dtype=torch.int32).cuda(), formant=torch.ones(S, dtype=torch.float64).cuda(),
                key=torch.zeros(S, dtype=torch.int32).cuda(), period=torch.zeros((S, h1.n_frames), dtype=torch.int32).cuda(),
                sout=torch.empty_like(d_sin), speriod=torch.zeros((NB, S), dtype=torch.int32).cuda(),
                carrier=torch.zeros_like(d_in), hratio=torch.ones((S, V, h1.n_frames), dtype=torch.float64).cuda(),
                gain=torch.ones((S, V), dtype=torch.float64).cuda(), dry=torch.ones(S, dtype=torch.float64).cuda(), depth=torch.ones(S, dtype=torch.float64).cuda())
    hin, hout = np.zeros((S, N), np.float32), np.zeros((S, N), np.float32)
    valid = {k: v.data_ptr() for k, v in bufs.items()}
    valid.update({"p": h1.h, "pv": pv.h, "trk": trk.h, "in": d_in.data_ptr(), "ratio": d_ratio.data_ptr(), "sin": d_sin.data_ptr(), "sratio": d_sratio.data_ptr(),
                  "mag": None, "semitones": 3.0, "n_in": T, "lifter": 32, "fs": 44100.0, "n_blocks": NB, "hin": hin.ctypes.data, "hout": hout.ctypes.data,
                  "xs": xs.h, "hz": hz.h, "scarrier": d_scarrier.data_ptr(), "shratio": d_shratio.data_ptr(), "n_voices": V,
                  "stream": C.c_void_p(torch.cuda.current_stream().cuda_stream)})
    named = {H2K: h2k.h, HSHORT: hshort.h, PV3: pv3.h}
    one_shot = {h.h.value: h for h in (h1, h2k, hshort)}
    torch.cuda.synchronize()
    assert {c[0] for c in CASES} == set(ENTRIES)
    for entry, wrong, code, msg in CASES:
        args = dict(valid)
        args.update({k: named.get(v, v) if isinstance(v, str) else v for k, v in wrong.items()})
        h = args["p"] if "p" in ENTRIES[entry] else None
        st = one_shot[h.value] if h is not None else None
        if st is not None:
            # a text of another entry in front of the case, so that "unchanged" and "set" can be told apart
            prime = TRK_NULL if msg == LOCK_NULL else LOCK_NULL
            if prime == LOCK_NULL:
                assert L.vp_stft_pitch_shift_locked(st.h, None, None, None, None) == INVALID
            else:
                assert L.vp_stft_track_pitch(st.h, None, 44100.0, None, None, None, None) == INVALID
            assert L.vp_stft_last_error(st.h).decode() == prime
        got = getattr(L, entry)(*[args[n] for n in ENTRIES[entry]])
        assert got == code, (entry, wrong, got, code)
        if st is not None:
            text = L.vp_stft_last_error(st.h).decode()
            assert text == (prime if msg is KEEP else msg), (entry, wrong, text)
        else:
            assert msg is KEEP and L.vp_stft_last_error(None) == b""
    # the handles the cases used give what fresh ones give, and have allocated nothing since
    fresh, fresh_pv, fresh_trk = StftRoundTrip(S, T, 1024, 256), PhaseVocoderStream(S, N), StreamingPitchTracker(S, N, 44100.0)
    fresh_xs, fresh_hz = CrossSynthStream(S, N), HarmonizerStream(S, N, V)
    assert pv.debug_alloc_count() == fresh_pv.debug_alloc_count() and trk.debug_alloc_count() == fresh_trk.debug_alloc_count()
    assert xs.debug_alloc_count() == fresh_xs.debug_alloc_count() and hz.debug_alloc_count() == fresh_hz.debug_alloc_count()
    got, want = _curve_call(h1, d_in, d_ratio), _curve_call(fresh, d_in, d_ratio)
    assert np.isfinite(want).all() and np.abs(want).max() > 0.01 and np.array_equal(got, want)
    got, want = _stream_call(pv, d_sin, d_sratio), _stream_call(fresh_pv, d_sin, d_sratio)
    assert np.isfinite(want).all() and np.abs(want).max() > 0.01 and np.array_equal(got, want)
    got, want = _cross_call(xs, d_sin, d_scarrier), _cross_call(fresh_xs, d_sin, d_scarrier)
    assert np.isfinite(want).all() and np.abs(want).max() > 0.01 and np.array_equal(got, want)
    got, want = _harm_call(hz, d_sin, d_shratio), _harm_call(fresh_hz, d_sin, d_shratio)
    assert np.isfinite(want).all() and np.abs(want).max() > 0.01 and np.array_equal(got, want)
    assert xs.debug_alloc_count() == fresh_xs.debug_alloc_count() and hz.debug_alloc_count() == fresh_hz.debug_alloc_count()
    for h in (h1, h2k, hshort, pv, trk, pv3, xs, hz, fresh, fresh_pv, fresh_trk, fresh_xs, fresh_hz):
        h.close()


# ---- the pending changes at the edges of one launch's VP_PV_MAX_UPDATES = 16 ----------------------------------------------------------------
# 34 streams of blocks of 64 samples at hop 256.  Two blocks of noise, then K per-stream resets in front of a two-block call: K = 15 and 16
# travel in the call itself (16: a full group), 17 and 32 need one update-only launch in front of it (a one-entry and a full carried group),
# 33 needs two.  The first 960 samples of a fresh stream are 0, so twenty more blocks follow, in which every stream's state shows.
ES, EN, HEAD, CALL, TAIL = 34, 64, 2, 2, 20
COUNTS = (15, 16, 17, 32, 33)


def _edge_slab(seed):
    x = np.random.default_rng(seed).normal(0, 0.2, (HEAD + CALL + TAIL, ES, EN)).astype(np.float32)
    return torch.from_numpy(x).cuda()


def _edge_streams(k):
    return np.sort(np.random.default_rng(k).permutation(ES)[:k])


def _edge_check(make, feed, prepare=lambda h, streams: None, fresh_prepare=lambda h: None):
    """make(): a handle; feed(h, b0, b1): blocks b0 .. b1 through one process call, the output as a numpy array [b1 - b0][ES][EN].  On the
    streams reset in front of the two-block call the output from there on is a fresh handle's (fresh_prepare: what such a handle needs
    first), on the others an undisturbed twin's, bit for bit; the handle has allocated nothing since it was made."""
    def rest(h):
        return np.concatenate([feed(h, HEAD, HEAD + CALL), feed(h, HEAD + CALL, HEAD + CALL + TAIL)])
    twin, fresh = make(), make()
    feed(twin, 0, HEAD)
    fresh_prepare(fresh)
    want_twin, want_fresh = rest(twin), rest(fresh)
    assert np.isfinite(want_twin).all() and np.isfinite(want_fresh).all()
    assert (np.abs(want_twin).max(axis=(0, 2)) > 0.01).all() and (np.abs(want_fresh).max(axis=(0, 2)) > 0.01).all()
    assert not np.array_equal(want_twin, want_fresh)
    for k in COUNTS:
        used, streams = make(), _edge_streams(k)
        allocs = used.debug_alloc_count()
        feed(used, 0, HEAD)
        for s in streams:
            used.reset(int(s))
        prepare(used, streams)
        got = rest(used)
        others = np.setdiff1d(np.arange(ES), streams)
        assert np.array_equal(got[:, streams], want_fresh[:, streams]), k
        assert np.array_equal(got[:, others], want_twin[:, others]), k
        assert used.debug_alloc_count() == allocs == twin.debug_alloc_count(), k
        used.close()
    twin.close()
    fresh.close()
    return want_fresh


def test_cross_synth_stream_resets_at_the_edges_of_one_launchs_updates():
    from vocoderproject_amd import CrossSynthStream
    d_v, d_c = _edge_slab(1), _edge_slab(2)

    def feed(h, b0, b1):
        d_out = torch.full_like(d_v[b0:b1], NAN)
        h.process_device(d_v[b0:b1], d_c[b0:b1], d_out, n_blocks=b1 - b0)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()
    _edge_check(lambda: CrossSynthStream(ES, EN), feed)


def test_harmonizer_stream_resets_at_the_edges_of_one_launchs_updates():
    from vocoderproject_amd import HarmonizerStream
    d_x = _edge_slab(3)

    def feed(h, b0, b1):
        d_out = torch.full_like(d_x[b0:b1], NAN)
        h.process_device(d_x[b0:b1], d_out, n_blocks=b1 - b0, semitones=[4.0, 7.0], dry=0.5)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()
    _edge_check(lambda: HarmonizerStream(ES, EN, V), feed)


def test_phase_vocoder_stream_resets_and_intervals_at_the_edges_of_one_launchs_updates():
    """Every reset stream also gets an interval of its own in front of the same call (one update carries both).  Once more with an
    all-stream reset in front of sixteen per-stream ones: seventeen updates, the all-stream one first."""
    from vocoderproject_amd import PhaseVocoderStream
    d_x = _edge_slab(4)
    semi = ((np.arange(ES) * 5) % 23 - 11).astype(np.float64)                  # (no stream keeps the interval 0 of the twin)
    semi[semi == 0.0] = 0.5

    def feed(h, b0, b1):
        d_out = torch.full_like(d_x[b0:b1], NAN)
        h.process_device(d_x[b0:b1], d_out, n_blocks=b1 - b0)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()

    def intervals(h, streams):
        for s in streams:
            h.set_semitones(semi[s], int(s))
    want_fresh = _edge_check(lambda: PhaseVocoderStream(ES, EN), feed, prepare=intervals, fresh_prepare=lambda h: intervals(h, range(ES)))
    used, streams = PhaseVocoderStream(ES, EN), _edge_streams(16)
    allocs = used.debug_alloc_count()
    intervals(used, range(ES))
    feed(used, 0, HEAD)
    used.reset(-1)
    for s in streams:
        used.reset(int(s))
    got = np.concatenate([feed(used, HEAD, HEAD + CALL), feed(used, HEAD + CALL, HEAD + CALL + TAIL)])
    assert np.array_equal(got, want_fresh) and used.debug_alloc_count() == allocs
    used.close()
