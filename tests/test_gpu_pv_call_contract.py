"""The argument contract of every vp_stft_* / vp_pv_* processing and autotune entry (include/vp_amd.h), one table: for each entry every
pointer null in turn, every scalar out of its range in turn and the pairs of simultaneous errors whose winner callers can see -- the code
returned and the exact vp_stft_last_error text, or that the text did not change.  No case launches a kernel.  Afterwards one valid
ratio-curve call on the one-shot handle and on the stream the cases used equals the same call on fresh handles, bit for bit: a refused
call leaves nothing behind."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

pytestmark = pytest.mark.gpu

INVALID, GEOMETRY = -1, -4                                    # include/vp_amd.h VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY
S, T, N, NB = 2, 4096, 64, 32
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
TRK_NULL = "pitch tracker: null input"
TRK_OUT = "pitch tracker: period and ratio outputs are both null"
TRK_FS = "pitch tracker: sample rate outside 8000 .. 51200 Hz"
TRK_SHORT = "pitch tracker: rows of 1024 samples are shorter than frame_len + tauMax = 1465"
TUNE_NULL = "autotune: null output or ratio table (the table is result and scratch)"

# entry -> its arguments, by the names of the valid values below (p: one-shot handle; pv, trk: stream and tracker; s*: the stream's slabs)
ENTRIES = {
    "vp_stft_roundtrip": ("p", "in", "out", "mag", "stream"),
    "vp_stft_pitch_shift": ("p", "in", "out", "semitones", "stream"),
    "vp_stft_pitch_shift_curve": ("p", "in", "out", "ratio", "stream"),
    "vp_stft_pitch_shift_locked": ("p", "in", "out", "ratio", "stream"),
    "vp_stft_pitch_shift_formant": ("p", "in", "out", "ratio", "formant", "lifter", "stream"),
    "vp_stft_time_stretch": ("p", "in", "n_in", "pos", "out", "semitones", "stream"),
    "vp_stft_time_stretch_locked": ("p", "in", "n_in", "pos", "out", "ratio", "stream"),
    "vp_stft_track_pitch": ("p", "in", "fs", "key", "period", "ratio", "stream"),
    "vp_stft_autotune": ("p", "in", "out", "fs", "key", "period", "ratio", "stream"),
    "vp_stft_autotune_formant": ("p", "in", "out", "fs", "key", "period", "ratio", "formant", "lifter", "stream"),
    "vp_pv_process_blocks_device": ("pv", "sin", "sout", "n_blocks", "stream"),
    "vp_pv_process_blocks_curve_device": ("pv", "sin", "sout", "sratio", "n_blocks", "stream"),
    "vp_pv_process_blocks_locked_device": ("pv", "sin", "sout", "sratio", "n_blocks", "stream"),
    "vp_pv_process_blocks_formant_device": ("pv", "sin", "sout", "sratio", "formant", "lifter", "n_blocks", "stream"),
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
for _e in ("vp_pv_process_blocks_curve_device", "vp_pv_process_blocks_locked_device", "vp_pv_process_blocks_formant_device"):
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


def test_every_entry_refuses_every_wrong_argument_with_its_code_and_message_and_leaves_the_handles_as_they_were():
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip, StreamingPitchTracker
    h1, h2k, hshort = StftRoundTrip(S, T, 1024, 256), StftRoundTrip(S, T, 2048, 512), StftRoundTrip(S, 1024, 1024, 256)
    pv, trk, pv3 = PhaseVocoderStream(S, N), StreamingPitchTracker(S, N, 44100.0), PhaseVocoderStream(3, N)
    L = h1.L
    rng = np.random.default_rng(7)
    d_in = torch.from_numpy(rng.normal(0, 0.2, (S, T)).astype(np.float32)).cuda()
    d_sin = torch.from_numpy(rng.normal(0, 0.2, (NB, S, N)).astype(np.float32)).cuda()
    d_ratio = torch.from_numpy(2.0 ** (rng.uniform(-12, 12, (S, h1.n_frames)) / 12)).cuda()
    d_sratio = torch.from_numpy(2.0 ** (rng.uniform(-12, 12, (NB, S)) / 12)).cuda()
    bufs = dict(out=torch.empty_like(d_in), pos=torch.zeros((S, h1.n_frames), dtype=torch.int32).cuda(), formant=torch.ones(S, dtype=torch.float64).cuda(),
                key=torch.zeros(S, dtype=torch.int32).cuda(), period=torch.zeros((S, h1.n_frames), dtype=torch.int32).cuda(),
                sout=torch.empty_like(d_sin), speriod=torch.zeros((NB, S), dtype=torch.int32).cuda())
    hin, hout = np.zeros((S, N), np.float32), np.zeros((S, N), np.float32)
    valid = {k: v.data_ptr() for k, v in bufs.items()}
    valid.update({"p": h1.h, "pv": pv.h, "trk": trk.h, "in": d_in.data_ptr(), "ratio": d_ratio.data_ptr(), "sin": d_sin.data_ptr(), "sratio": d_sratio.data_ptr(),
                  "mag": None, "semitones": 3.0, "n_in": T, "lifter": 32, "fs": 44100.0, "n_blocks": NB, "hin": hin.ctypes.data, "hout": hout.ctypes.data,
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
    assert pv.debug_alloc_count() == fresh_pv.debug_alloc_count() and trk.debug_alloc_count() == fresh_trk.debug_alloc_count()
    got, want = _curve_call(h1, d_in, d_ratio), _curve_call(fresh, d_in, d_ratio)
    assert np.isfinite(want).all() and np.abs(want).max() > 0.01 and np.array_equal(got, want)
    got, want = _stream_call(pv, d_sin, d_sratio), _stream_call(fresh_pv, d_sin, d_sratio)
    assert np.isfinite(want).all() and np.abs(want).max() > 0.01 and np.array_equal(got, want)
    for h in (h1, h2k, hshort, pv, trk, pv3, fresh, fresh_pv, fresh_trk):
        h.close()
