"""Host-side mirror of the reference's plugin surface over the C ABI (include/vp_amd.h).

`BatchVocoderProcessor` plays the role of `VocoderAudioProcessor` (PluginProcessor.h:24-80) for a
batch of independent streams on one MI355X: the same ten parameters (PluginProcessor.cpp:37-73),
`prepareToPlay(sampleRate, samplesPerBlock)` (:144) and `processBlock(buffer)` (:203) on planar
float32 buffers `[stream][channel][sample]`.  Everything below the class is ctypes plumbing; the
compute lives in libvp_amd.so (HIP kernels).  There is no CPU fallback: if the shared library is
missing or no GPU is present the constructor raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VP_AMD_LIB") or os.path.join(_HERE, "libvp_amd.so")   # VP_AMD_LIB: diagnostic builds only

PARAM_IDS = ("gainPitch", "gainVoice", "gainSynth", "gainVoc", "lpcVoice", "lpcPitch",
             "lpcSynth", "keyPitch", "pitchBool", "vocBool")
KEYS = ("A", "A#", "B", "C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "Chrom")   # PluginProcessor.cpp:64
GEOM_KEYS = ("N", "F", "H", "C", "W", "h", "toKeep", "latency", "inSize", "outSize", "tauMax", "chunksPerFrame")
KERNEL_SLOTS = 4
MARK_CAP = 64


class VpParams(C.Structure):
    _fields_ = [("gainPitch", C.c_float), ("gainVoice", C.c_float), ("gainSynth", C.c_float), ("gainVoc", C.c_float),
                ("lpcVoice", C.c_int), ("lpcPitch", C.c_int), ("lpcSynth", C.c_int), ("keyPitch", C.c_int),
                ("pitchBool", C.c_int), ("vocBool", C.c_int)]


class VpPitchState(C.Structure):
    _fields_ = [("period", C.c_int), ("prevPeriod", C.c_int), ("prevVoicedPeriod", C.c_int), ("periodNew", C.c_int),
                ("nAn", C.c_int), ("nSt", C.c_int), ("stMarkIdx", C.c_int), ("gateOpen", C.c_int),
                ("pitch", C.c_double), ("prevPitch", C.c_double), ("beta", C.c_double), ("closestFreq", C.c_double),
                ("anMarks", C.c_int * MARK_CAP), ("stMarks", C.c_int * MARK_CAP), ("a", C.c_double * 101)]


class VpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libvp_amd error {code}: {msg}")
        self.code = code


_lib = None


def load_library():
    """dlopen libvp_amd.so (built by vocoderproject_amd.build). Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not built: run `python -m vocoderproject_amd.build` "
                                "(needs hipcc); this package has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    fp = C.c_void_p      # float* passed as integer addresses (host numpy or device data_ptr)
    L.vp_abi_version.restype = C.c_int
    L.vp_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.vp_destroy.argtypes = [vp]
    L.vp_set_params.argtypes = [vp, C.POINTER(VpParams)]
    L.vp_get_params.argtypes = [vp, C.POINTER(VpParams)]
    L.vp_default_params.argtypes = [C.POINTER(VpParams)]
    L.vp_default_params.restype = None
    L.vp_prepare_to_play.argtypes = [vp, C.c_double, C.c_int, C.c_int]
    L.vp_prepare_explicit.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.vp_process_block.argtypes = [vp, fp, fp]
    L.vp_process_block_inplace.argtypes = [vp, fp]
    L.vp_process_block_device.argtypes = [vp, fp, fp, C.c_void_p]
    L.vp_get_latency.argtypes = [vp]
    L.vp_get_geometry.argtypes = [vp, C.POINTER(C.c_int)]
    L.vp_get_num_streams.argtypes = [vp]
    L.vp_read_pitch_state.argtypes = [vp, C.c_int, C.POINTER(VpPitchState)]
    L.vp_synchronize.argtypes = [vp]
    L.vp_profile_enable.argtypes = [vp, C.c_int]
    L.vp_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long), C.c_int]
    L.vp_kernel_slot_name.argtypes = [C.c_int]
    L.vp_kernel_slot_name.restype = C.c_char_p
    if hasattr(L, "vp_process_blocks_device"):
        L.vp_process_blocks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "vp_set_stream_params"):            # absent only from older builds loaded through VP_AMD_LIB (tools/ab.sh)
        L.vp_set_stream_params.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.vp_get_stream_params.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "vp_process_block_mono"):
        L.vp_process_block_mono.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.vp_process_block_mono_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vp_process_blocks_mono_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "vp_process_block_channels"):        # (absent only from older libraries loaded through VP_AMD_LIB)
        L.vp_process_block_channels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.vp_process_block_channels_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.vp_process_blocks_channels_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "vp_process_blocks"):
        L.vp_process_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    if hasattr(L, "vp_set_pitch_shift"):
        L.vp_set_pitch_shift.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
        L.vp_get_pitch_shift.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.vp_pitch_kernel_name.argtypes = [C.c_void_p]
    L.vp_pitch_kernel_name.restype = C.c_char_p
    if hasattr(L, "vp_vocoder_kernel_name"):
        L.vp_vocoder_kernel_name.argtypes = [C.c_void_p]
        L.vp_vocoder_kernel_name.restype = C.c_char_p
    if hasattr(L, "vp_set_vocoder_path"):
        L.vp_set_vocoder_path.argtypes = [C.c_void_p, C.c_int]
        L.vp_get_vocoder_path.argtypes = [C.c_void_p]
    if hasattr(L, "vp_set_overlap"):
        L.vp_set_overlap.argtypes = [C.c_void_p, C.c_int]
        L.vp_get_overlap.argtypes = [C.c_void_p]
    if hasattr(L, "vp_reserve_blocks"):                  # (an older A/B library handed over through VP_AMD_LIB still loads)
        L.vp_reserve_blocks.argtypes = [C.c_void_p, C.c_int]
        L.vp_get_reserved_blocks.argtypes = [C.c_void_p]
        L.vp_debug_alloc_count.argtypes = [C.c_void_p]
        L.vp_debug_alloc_count.restype = C.c_long
    if hasattr(L, "vp_set_time_parallel"):
        L.vp_set_time_parallel.argtypes = [C.c_void_p, C.c_int]
        L.vp_get_time_parallel.argtypes = [C.c_void_p]
    if hasattr(L, "vp_set_wave_specialised"):
        L.vp_set_wave_specialised.argtypes = [C.c_void_p, C.c_int]
        L.vp_get_wave_specialised.argtypes = [C.c_void_p]
    if hasattr(L, "vp_debug_pitch_symbol"):
        L.vp_debug_pitch_symbol.argtypes = [C.c_void_p]
        L.vp_debug_pitch_symbol.restype = C.c_char_p
    if hasattr(L, "vp_debug_set_spin_limit"):          # (ABI version 3)
        L.vp_debug_set_spin_limit.argtypes = [C.c_void_p, C.c_int]
    L.vp_read_ub_counters.argtypes = [vp, C.POINTER(C.c_long)]
    L.vp_debug_read_stamps.argtypes = [vp, C.POINTER(C.c_ulonglong), C.c_int]
    L.vp_set_yin_mode.argtypes = [vp, C.c_int]
    L.vp_get_yin_mode.argtypes = [vp]
    L.vp_set_iir_mode.argtypes = [vp, C.c_int]
    L.vp_get_iir_mode.argtypes = [vp]
    L.vp_stft_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.vp_stft_destroy.argtypes = [vp]
    L.vp_stft_num_frames.argtypes = [vp]
    L.vp_stft_roundtrip.argtypes = [vp, fp, fp, fp, C.c_void_p]
    L.vp_stft_pitch_shift.argtypes = [vp, fp, fp, C.c_double, C.c_void_p]
    L.vp_stft_is_fused.argtypes = [vp]
    if hasattr(L, "vp_stft_pitch_shift_curve"):        # (the ratio-curve entries; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_stft_pitch_shift_curve.argtypes = [vp, fp, fp, C.c_void_p, C.c_void_p]
        L.vp_semitones_to_ratios.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
        L.vp_pv_process_blocks_curve_device.argtypes = [vp, fp, fp, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "vp_stft_pitch_shift_locked"):       # (the peak-locked entries; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_stft_pitch_shift_locked.argtypes = [vp, fp, fp, C.c_void_p, C.c_void_p]
        L.vp_pv_process_blocks_locked_device.argtypes = [vp, fp, fp, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "vp_stft_pitch_shift_locked_subbin"):   # (the sub-bin locked entries; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_stft_pitch_shift_locked_subbin.argtypes = [vp, fp, fp, C.c_void_p, C.c_void_p]
        L.vp_pv_process_blocks_locked_subbin_device.argtypes = [vp, fp, fp, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "vp_stft_time_stretch"):             # (the time stretch; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_stft_time_stretch.argtypes = [vp, fp, C.c_int, C.c_void_p, fp, C.c_double, C.c_void_p]
        L.vp_stretch_positions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]
    if hasattr(L, "vp_stft_time_stretch_locked"):      # (the locked time stretch; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_stft_time_stretch_locked.argtypes = [vp, fp, C.c_int, C.c_void_p, fp, C.c_void_p, C.c_void_p]
    if hasattr(L, "vp_stft_onset_flux"):               # (the transient-preserving stretch; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_onset_num_frames.argtypes = [C.c_int, C.c_int, C.c_int]
        L.vp_stft_onset_flux.argtypes = [vp, fp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vp_onset_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
        L.vp_stretch_positions_transient.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.vp_stft_time_stretch_locked_reset.argtypes = [vp, fp, C.c_int, C.c_void_p, fp, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "vp_stft_track_pitch"):              # (the pitch tracker; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_track_tau_max.argtypes = [C.c_double]
        L.vp_stft_track_pitch.argtypes = [vp, fp, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vp_stft_autotune.argtypes = [vp, fp, fp, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vp_stft_last_error.argtypes = [vp]
        L.vp_stft_last_error.restype = C.c_char_p
    if hasattr(L, "vp_stft_track_pitch_fine"):         # (the fine tracker; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_stft_set_track_mode.argtypes = [vp, C.c_int]
        L.vp_stft_get_track_mode.argtypes = [vp]
        L.vp_stft_track_pitch_fine.argtypes = [vp, fp, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vp_pv_tracker_set_mode.argtypes = [vp, C.c_int]
        L.vp_pv_tracker_get_mode.argtypes = [vp]
        L.vp_pv_tracker_process_blocks_fine_device.argtypes = [vp, fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.vp_stft_set_runs.argtypes = [vp, C.c_int]
    L.vp_stft_set_precision.argtypes = [vp, C.c_int]
    L.vp_stft_get_precision.argtypes = [vp]
    if hasattr(L, "vp_pv_create"):                     # (the streaming phase vocoder; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_pv_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.vp_pv_destroy.argtypes = [vp]
        L.vp_pv_get_latency.argtypes = [vp]
        L.vp_pv_set_semitones.argtypes = [vp, C.c_int, C.c_double]
        L.vp_pv_get_semitones.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
        L.vp_pv_reset.argtypes = [vp, C.c_int]
        L.vp_pv_process_block.argtypes = [vp, fp, fp]
        L.vp_pv_process_blocks_device.argtypes = [vp, fp, fp, C.c_int, C.c_void_p]
        L.vp_pv_debug_alloc_count.argtypes = [vp]
        L.vp_pv_debug_alloc_count.restype = C.c_long
    if hasattr(L, "vp_pv_tracker_create"):             # (the streaming pitch tracker; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_pv_tracker_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(vp)]
        L.vp_pv_tracker_destroy.argtypes = [vp]
        L.vp_pv_tracker_debug_alloc_count.argtypes = [vp]
        L.vp_pv_tracker_debug_alloc_count.restype = C.c_long
        L.vp_pv_tracker_reset.argtypes = [vp, C.c_int]
        L.vp_pv_tracker_set_follow.argtypes = [vp, C.c_int, C.c_double]
        L.vp_pv_tracker_process_blocks_device.argtypes = [vp, fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.vp_pv_autotune_blocks_device.argtypes = [vp, vp, fp, fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "vp_stft_pitch_shift_formant"):      # (the formant entries; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_stft_pitch_shift_formant.argtypes = [vp, fp, fp, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.vp_stft_autotune_formant.argtypes = [vp, fp, fp, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.vp_pv_process_blocks_formant_device.argtypes = [vp, fp, fp, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.vp_pv_autotune_blocks_formant_device.argtypes = [vp, vp, fp, fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "vp_stft_cross_synth"):              # (the cross-synthesis entries; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_stft_cross_synth.argtypes = [vp, fp, fp, fp, C.c_void_p, C.c_int, C.c_void_p]
        L.vp_xs_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.vp_xs_destroy.argtypes = [vp]
        L.vp_xs_get_latency.argtypes = [vp]
        L.vp_xs_reset.argtypes = [vp, C.c_int]
        L.vp_xs_process_blocks_device.argtypes = [vp, fp, fp, fp, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.vp_xs_debug_alloc_count.argtypes = [vp]
        L.vp_xs_debug_alloc_count.restype = C.c_long
    if hasattr(L, "vp_stft_harmonize"):                # (the harmonizer entries; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_stft_harmonize.argtypes = [vp, fp, fp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vp_hz_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.vp_hz_destroy.argtypes = [vp]
        L.vp_hz_get_latency.argtypes = [vp]
        L.vp_hz_reset.argtypes = [vp, C.c_int]
        L.vp_hz_process_blocks_device.argtypes = [vp, fp, fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.vp_hz_debug_alloc_count.argtypes = [vp]
        L.vp_hz_debug_alloc_count.restype = C.c_long
    if hasattr(L, "vp_stft_track_harmony"):            # (the key-aware voices; absent from older libraries loaded through VP_AMD_LIB)
        L.vp_stft_track_harmony.argtypes = [vp, fp, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vp_stft_harmonize_key.argtypes = [vp, fp, fp, C.c_double, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.vp_pv_tracker_process_blocks_voices_device.argtypes = [vp, fp, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                                 C.c_void_p]
        L.vp_hz_autoharm_blocks_device.argtypes = [vp, vp, fp, fp] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
    L.vp_error_string.argtypes = [C.c_int]
    L.vp_error_string.restype = C.c_char_p
    L.vp_last_error.argtypes = [vp]
    L.vp_last_error.restype = C.c_char_p
    _lib = L
    return L


class BatchVocoderProcessor:
    """A batch of `VocoderAudioProcessor` instances on one GPU (one per stream)."""

    def __init__(self, device=0, **params):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.vp_create(int(device), C.byref(h))
        if rc:
            raise VpError(rc, self.L.vp_error_string(rc).decode())
        self.h = h
        self.device = device
        self._p = VpParams()
        self.L.vp_default_params(C.byref(self._p))
        self.n_streams = 0
        self.N = 0
        for k, v in params.items():
            self.setParameter(k, v)

    # ---- lifetime ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.L.vp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise VpError(rc, f"{self.L.vp_error_string(rc).decode()} ({self.L.vp_last_error(self.h).decode()})")

    # ---- parameters (treeState) --------------------------------------------------------------------
    def setParameter(self, pid, value):
        if pid not in PARAM_IDS:
            raise KeyError(pid)
        old = getattr(self._p, pid)
        setattr(self._p, pid, type(old)(value))
        rc = self.L.vp_set_params(self.h, C.byref(self._p))
        if rc:
            setattr(self._p, pid, old)
            self._chk(rc)

    def getParameter(self, pid):
        return getattr(self._p, pid)

    def setStreamParameter(self, stream, pid, value):
        """One stream's own value of a parameter (each stream is a plugin instance with its own treeState).  After
        prepare; pitchBool, vocBool and lpcPitch stay per handle.  setParameter() puts all streams back on one set."""
        if pid not in PARAM_IDS:
            raise KeyError(pid)
        q = VpParams()
        self._chk(self.L.vp_get_stream_params(self.h, int(stream), C.byref(q)))
        setattr(q, pid, type(getattr(q, pid))(value))
        self._chk(self.L.vp_set_stream_params(self.h, int(stream), C.byref(q)))

    def setPitchShift(self, semitones, on=True, stream=-1):
        """Extension (no reference counterpart): shift by a fixed interval of +-12 semitones instead of correcting to
        the key's nearest note; stream = -1 sets every stream of the batch."""
        self._chk(self.L.vp_set_pitch_shift(self.h, int(stream), int(bool(on)), float(semitones)))

    def getPitchShift(self, stream):
        on, semi = C.c_int(), C.c_double()
        self._chk(self.L.vp_get_pitch_shift(self.h, int(stream), C.byref(on), C.byref(semi)))
        return bool(on.value), semi.value

    def getStreamParameter(self, stream, pid):
        q = VpParams()
        self._chk(self.L.vp_get_stream_params(self.h, int(stream), C.byref(q)))
        return getattr(q, pid)

    def set_iir_mode(self, mode):
        """"exact" (default, bit-identical to the reference's summation order) or "fast" (VP_IIR_FAST)."""
        self._chk(self.L.vp_set_iir_mode(self.h, {"exact": 0, "fast": 1}[mode] if isinstance(mode, str) else int(mode)))

    def set_vocoder_path(self, path):
        """"auto" (default: batched above 256 streams), "workgroup" (one workgroup per stream) or
        "batched" (the lane-per-window pipeline wherever it can run)."""
        self._chk(self.L.vp_set_vocoder_path(self.h, {"auto": 0, "workgroup": 1, "batched": 2}[path] if isinstance(path, str) else int(path)))

    def set_overlap(self, on):
        """FAST mode, both processes, batched vocoder: pitch corrector beside the vocoder pipeline (default) or behind it."""
        self._chk(self.L.vp_set_overlap(self.h, 2 if on == "auto" else int(bool(on))))

    def set_time_parallel(self, on):
        """Kept for older callers: stored and returned, without effect (the analysis front end it selected was removed in round 6)."""
        self._chk(self.L.vp_set_time_parallel(self.h, int(bool(on))))

    def set_wave_specialised(self, on):
        """Single-block calls of the plugin's geometry on the wave-specialised pitch kernel (default) or on the phase kernels (same bits).
        2: the wave-specialised kernel's generic builds only, never its lean build (vp_k_pitch_ws_l; same bits again)."""
        self._chk(self.L.vp_set_wave_specialised(self.h, 2 if on == 2 else int(bool(on))))

    def set_yin_mode(self, mode):
        """"direct" (default: the reference's sums), "xcorr" (certified cross-correlation form, fused multiply-adds) or "fft" (the same
        certified form with its cross-correlations by FFT where the build carries it); all three give the same output bits."""
        self._chk(self.L.vp_set_yin_mode(self.h, {"direct": 0, "fft": 1, "xcorr": 2, "xcorr_force_fallback": 3}[mode] if isinstance(mode, str) else int(mode)))

    def get_yin_mode(self):
        return {0: "direct", 1: "fft", 2: "xcorr", 3: "xcorr_force_fallback"}[self.L.vp_get_yin_mode(self.h)]

    def get_iir_mode(self):
        return "fast" if self.L.vp_get_iir_mode(self.h) == 1 else "exact"

    # ---- prepareToPlay -----------------------------------------------------------------------------
    def prepareToPlay(self, sampleRate, samplesPerBlock, nStreams=1):
        self._chk(self.L.vp_prepare_to_play(self.h, float(sampleRate), int(samplesPerBlock), int(nStreams)))
        self.n_streams, self.N = int(nStreams), int(samplesPerBlock)

    def prepareExplicit(self, sampleRate, samplesPerBlock, nStreams, frameLenPitch, hopPitch, wlenVoc, hopVoc):
        self._chk(self.L.vp_prepare_explicit(self.h, float(sampleRate), int(samplesPerBlock), int(nStreams),
                                             int(frameLenPitch), int(hopPitch), int(wlenVoc), int(hopVoc)))
        self.n_streams, self.N = int(nStreams), int(samplesPerBlock)

    def getLatencySamples(self):
        rc = self.L.vp_get_latency(self.h)
        if rc < 0:
            self._chk(rc)
        return rc

    @property
    def latency(self):
        return self.getLatencySamples()

    def geometry(self):
        g = (C.c_int * 12)()
        self._chk(self.L.vp_get_geometry(self.h, g))
        return dict(zip(GEOM_KEYS, list(g)))

    # ---- processBlock ---------------------------------------------------------------------------------
    def processBlock(self, buffer):
        """In place, like the reference: float32 numpy [S][3][N]; on return ch0/ch1 = out L/R, ch2 = 0."""
        assert isinstance(buffer, np.ndarray) and buffer.dtype == np.float32 and buffer.flags.c_contiguous
        assert buffer.shape == (self.n_streams, 3, self.N), buffer.shape
        self._chk(self.L.vp_process_block_inplace(self.h, buffer.ctypes.data))

    def process(self, x):
        """Host convenience: float32 numpy [S][3][N] -> new float32 [S][2][N]."""
        assert x.dtype == np.float32 and x.flags.c_contiguous and x.shape == (self.n_streams, 3, self.N)
        out = np.empty((self.n_streams, 2, self.N), np.float32)
        self._chk(self.L.vp_process_block(self.h, x.ctypes.data, out.ctypes.data))
        return out

    def process_mono(self, voice):
        """Buffers without the side-chain bus: float32 numpy [S][N] -> new float32 [S][2][N] (== process() with zeroed ch1/ch2)."""
        assert voice.dtype == np.float32 and voice.flags.c_contiguous and voice.shape == (self.n_streams, self.N)
        out = np.empty((self.n_streams, 2, self.N), np.float32)
        self._chk(self.L.vp_process_block_mono(self.h, voice.ctypes.data, out.ctypes.data))
        return out

    def process_mono_device(self, d_voice, d_out, stream=None):
        """Device-resident mono entry: torch float32 tensors [S][N] -> [S][2][N]."""
        assert d_voice.is_cuda and d_out.is_cuda and d_voice.is_contiguous() and d_out.is_contiguous()
        assert tuple(d_voice.shape) == (self.n_streams, self.N) and tuple(d_out.shape) == (self.n_streams, 2, self.N)
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(d_voice.device).cuda_stream
        self._chk(self.L.vp_process_block_mono_device(self.h, d_voice.data_ptr(), d_out.data_ptr(), C.c_void_p(stream)))

    def process_blocks_mono_device(self, d_voice, d_out, stream=None):
        """B consecutive mono blocks at once: torch float32 [B][S][N] -> [B][S][2][N]."""
        assert d_voice.is_cuda and d_out.is_cuda and d_voice.is_contiguous() and d_out.is_contiguous()
        B = d_voice.shape[0]
        assert tuple(d_voice.shape) == (B, self.n_streams, self.N) and tuple(d_out.shape) == (B, self.n_streams, 2, self.N)
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(d_voice.device).cuda_stream
        self.reserve_blocks(B)
        self._chk(self.L.vp_process_blocks_mono_device(self.h, d_voice.data_ptr(), d_out.data_ptr(), int(B), C.c_void_p(stream)))

    def reserve_blocks(self, n_blocks):
        """vp_reserve_blocks: size the multi-block scratch and staging for calls of up to n_blocks blocks (the C process calls never
        allocate; the process_blocks* methods of this mirror call it for the caller when a call is larger than what is reserved)."""
        if int(n_blocks) > self.L.vp_get_reserved_blocks(self.h):
            self._chk(self.L.vp_reserve_blocks(self.h, int(n_blocks)))

    def alloc_count(self):
        return int(self.L.vp_debug_alloc_count(self.h))

    def process_device(self, d_in, d_out, stream=None):
        """Device-resident, asynchronous: torch CUDA(HIP) float32 tensors [S][3][N] -> [S][2][N]."""
        assert d_in.is_cuda and d_out.is_cuda and d_in.is_contiguous() and d_out.is_contiguous()
        assert tuple(d_in.shape) == (self.n_streams, 3, self.N) and tuple(d_out.shape) == (self.n_streams, 2, self.N)
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(d_in.device).cuda_stream
        self._chk(self.L.vp_process_block_device(self.h, d_in.data_ptr(), d_out.data_ptr(), C.c_void_p(stream)))

    def process_blocks_device(self, d_in, d_out, stream=None):
        """B consecutive blocks at once: torch float32 tensors [B][S][3][N] -> [B][S][2][N]; same results as B calls of
        process_device (pitch corrector alone: ONE launch, state stays on chip between the blocks; vocoder alone, or both in the
        fast IIR mode: groups of up to 16 blocks per launch of the pipeline -- see include/vp_amd.h)."""
        assert d_in.is_cuda and d_out.is_cuda and d_in.is_contiguous() and d_out.is_contiguous()
        B = d_in.shape[0]
        assert tuple(d_in.shape) == (B, self.n_streams, 3, self.N) and tuple(d_out.shape) == (B, self.n_streams, 2, self.N)
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(d_in.device).cuda_stream
        self.reserve_blocks(B)
        self._chk(self.L.vp_process_blocks_device(self.h, d_in.data_ptr(), d_out.data_ptr(), int(B), C.c_void_p(stream)))

    def process_blocks(self, x):
        """vp_process_blocks: float32 numpy [B][S][3][N] -> new float32 [B][S][2][N], same results as B calls of
        process() (pitch corrector alone: one launch; used by the offline front end)."""
        assert x.dtype == np.float32 and x.flags.c_contiguous and x.ndim == 4 and x.shape[1:] == (self.n_streams, 3, self.N), x.shape
        out = np.empty((x.shape[0], self.n_streams, 2, self.N), np.float32)
        self.reserve_blocks(x.shape[0])
        self._chk(self.L.vp_process_blocks(self.h, x.ctypes.data, out.ctypes.data, int(x.shape[0])))
        return out

    # ---- channel pointers (what AudioBuffer<float> holds: one row per channel, not a slab) -------------------
    def process_channels(self, ins, outs):
        """vp_process_block_channels: `ins` a sequence of S * n_in rows (n_in 1 or 3; row (s, ch) = ins[s * n_in + ch]), `outs` of
        S * n_out rows (n_out 2 or 3): float32 numpy arrays of N samples each, or None -- silence on the input side (MyBuffer.cpp:93-102),
        "not wanted" on the output side.  Output rows are written in place and may be the input rows; row 2 of a stream receives zeros."""
        S, N = self.n_streams, self.N
        n_in, n_out = len(ins) // max(S, 1), len(outs) // max(S, 1)
        assert len(ins) == S * n_in and len(outs) == S * n_out, (len(ins), len(outs), S)

        def table(rows, writable):
            t = (C.c_void_p * len(rows))()
            for i, r in enumerate(rows):
                if r is None:
                    continue
                assert isinstance(r, np.ndarray) and r.dtype == np.float32 and r.ndim == 1 and r.shape[0] == N and r.strides[0] == 4, i
                assert not writable or r.flags.writeable, i
                t[i] = r.ctypes.data
            return t
        self._chk(self.L.vp_process_block_channels(self.h, table(ins, False), n_in, table(outs, True), n_out))

    @staticmethod
    def channel_table(rows):
        """A device table for process_channels_device: `rows` a sequence of 1-D float32 CUDA tensors (each a row of samples, any
        alignment a float has) or None -> int64 CUDA tensor of their data_ptr()s (0 for None).  The table keeps the rows alive
        (`table.rows`); build it once and reuse it."""
        import torch
        dev = next((r.device for r in rows if r is not None), torch.device("cuda"))
        for r in rows:
            assert r is None or (r.is_cuda and r.dtype == torch.float32 and r.dim() == 1 and r.stride(0) == 1 and r.device == dev)
        t = torch.tensor([0 if r is None else r.data_ptr() for r in rows], dtype=torch.int64).to(dev)
        t.rows = list(rows)
        t.min_len = min((r.numel() for r in rows if r is not None), default=1 << 62)    # (checked against n_blocks * N per call: one comparison, not a loop)
        return t

    def process_channels_device(self, in_table, n_in, out_table, n_out, n_blocks=1, stream=None):
        """vp_process_block_channels_device (n_blocks = 1) / vp_process_blocks_channels_device (rows of n_blocks * N samples): device
        tables from channel_table(), S * n_in and S * n_out entries; enqueued on `stream` (default: the current torch stream) without
        synchronising.  Bit-identical to process_device / process_blocks_device on the packed data."""
        import torch
        for t, n in ((in_table, n_in), (out_table, n_out)):
            assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == self.n_streams * n, (t.shape, n)
        for t in (in_table, out_table):
            assert getattr(t, "min_len", int(n_blocks) * self.N) >= int(n_blocks) * self.N, "a row is shorter than n_blocks * N samples"
        if stream is None:
            stream = torch.cuda.current_stream(in_table.device).cuda_stream
        if int(n_blocks) == 1:
            self._chk(self.L.vp_process_block_channels_device(self.h, in_table.data_ptr(), int(n_in), out_table.data_ptr(), int(n_out), C.c_void_p(stream)))
        else:
            self._chk(self.L.vp_process_blocks_channels_device(self.h, in_table.data_ptr(), int(n_in), out_table.data_ptr(), int(n_out), int(n_blocks),
                                                               C.c_void_p(stream)))

    def run(self, x):
        """x: float32 numpy [S][3][T], T a multiple of N -> float32 [S][2][T] (block by block)."""
        S, _, T = x.shape
        assert S == self.n_streams and T % self.N == 0
        out = np.empty((S, 2, T), np.float32)
        for b in range(T // self.N):
            blk = np.ascontiguousarray(x[:, :, b * self.N:(b + 1) * self.N])
            out[:, :, b * self.N:(b + 1) * self.N] = self.process(blk)
        return out

    # ---- introspection ------------------------------------------------------------------------------------
    def synchronize(self):
        self._chk(self.L.vp_synchronize(self.h))

    def pitch_state(self, stream):
        st = VpPitchState()
        self._chk(self.L.vp_read_pitch_state(self.h, int(stream), C.byref(st)))
        return dict(period=st.period, prevPeriod=st.prevPeriod, prevVoicedPeriod=st.prevVoicedPeriod,
                    periodNew=st.periodNew, pitch=st.pitch, prevPitch=st.prevPitch, beta=st.beta,
                    closestFreq=st.closestFreq, gateOpen=st.gateOpen, stMarkIdx=st.stMarkIdx,
                    anMarks=list(st.anMarks[:st.nAn]), stMarks=list(st.stMarks[:st.nSt]), a=np.array(st.a[:]))

    def ub_counters(self):
        c = (C.c_long * 5)()
        self._chk(self.L.vp_read_ub_counters(self.h, c))
        return list(c)

    def debug_stamps(self, reset=True):
        """Diagnostic build only: per-phase microseconds accumulated by workgroup 0."""
        v = (C.c_ulonglong * 64)()
        self._chk(self.L.vp_debug_read_stamps(self.h, v, int(bool(reset))))
        return [t / 100.0 for t in v]

    def yin_certified_counts(self, reset=True):
        """(frames whose pitch decision the certified cross-correlation form settled, frames it handed to the reference's
        arithmetic) since the last reset, over all streams; both 0 outside VP_YIN_XCORR."""
        v = (C.c_ulonglong * 64)()
        self._chk(self.L.vp_debug_read_stamps(self.h, v, int(bool(reset))))
        assert int(v[61]) == 0, "the prefix-sum flag of VP_YIN_XCORR timed out (kernel bug)"
        return int(v[62]), int(v[63])

    def profile_enable(self, on=True):
        """True/1: HIP events around every kernel launch; k > 1: around every k-th one; False/0: off."""
        self._chk(self.L.vp_profile_enable(self.h, int(on)))

    def profile_read(self, reset=True):
        ms = (C.c_double * KERNEL_SLOTS)()
        n = (C.c_long * KERNEL_SLOTS)()
        self._chk(self.L.vp_profile_read(self.h, ms, n, int(bool(reset))))
        names = [self.L.vp_kernel_slot_name(i).decode() for i in range(KERNEL_SLOTS)]
        names[2] = self.pitch_kernel_name() or names[2]          # the build actually launched (rocprof shows this symbol)
        return {names[i]: (ms[i], n[i]) for i in range(KERNEL_SLOTS)}

    def pitch_kernel_name(self):
        return self.L.vp_pitch_kernel_name(self.h).decode()

    def debug_pitch_symbol(self):
        """Diagnostic: symbol of the pitch kernel the last process call launched ("" before the first)."""
        return self.L.vp_debug_pitch_symbol(self.h).decode()

    def debug_set_spin_limit(self, polls):
        """Diagnostic: polls a kernel's bounded inter-wavefront wait makes before it raises VP_ERR_TIMEOUT (default 2^22)."""
        self._chk(self.L.vp_debug_set_spin_limit(self.h, int(polls)))

    def vocoder_kernel_name(self):
        return self.L.vp_vocoder_kernel_name(self.h).decode()


def semitones_to_ratios(semitones):
    """Pitch ratios 2^(st / 12) of an array of intervals, float64 of the same shape, through the library's vp_semitones_to_ratios:
    the bits vp_stft_pitch_shift and vp_pv_set_semitones use (numpy.power's may differ).  VpError for an entry outside +-12 or not finite."""
    L = load_library()
    st = np.ascontiguousarray(semitones, dtype=np.float64)
    r = np.empty_like(st)
    rc = L.vp_semitones_to_ratios(st.ctypes.data, r.ctypes.data, st.size)
    if rc:
        raise VpError(rc, L.vp_error_string(rc).decode())
    return r


def stretch_positions(n_frames, hop, stretch, n_in, frame_len=1024):
    """The position table of a constant time stretch, int32 [n_frames] through the library's vp_stretch_positions:
    pos[f] = min(floor(f hop / stretch), n_in - frame_len), stretch = output duration / input duration in [0.25, 4].  VpError outside
    that range or for a stretch that is not finite.  No device is touched."""
    L = load_library()
    pos = np.empty(int(n_frames), dtype=np.int32)
    rc = L.vp_stretch_positions(pos.ctypes.data, int(n_frames), int(hop), float(stretch), int(n_in), int(frame_len))
    if rc:
        raise VpError(rc, L.vp_error_string(rc).decode())
    return pos


ONSET_THRESHOLD = 0.2                   # include/vp_amd.h VP_DEFAULT_ONSET_THRESHOLD (DESIGN.md says why)
ONSET_SPAN_MIN, ONSET_SPAN_MAX = 1, 8   # include/vp_amd.h VP_ONSET_SPAN_MIN, VP_ONSET_SPAN_MAX


def default_onset_span(frame_len, hop):
    """The span's half width K the tools take when none is given: max(frame_len / (2 hop), 1) -- the frames that overlap the onset's."""
    return max(int(frame_len) // (2 * int(hop)), 1)


def pick_onsets(flux, mass, thr=ONSET_THRESHOLD):
    """The onsets of one row from its flux and mass tables (StftRoundTrip.onset_flux), uint8 [nG] through the library's vp_onset_pick:
    frame g is an onset iff flux[g] > 0, flux[g] >= thr mass[g], flux[g] > flux[g-1] and flux[g] >= flux[g+1]; a missing neighbour counts
    as -inf, a NaN in a comparison is "no".  thr in [0, 1]; VpError outside.  No device is touched."""
    L = load_library()
    fl, ms = np.ascontiguousarray(flux, dtype=np.float64), np.ascontiguousarray(mass, dtype=np.float64)
    if fl.ndim != 1 or fl.shape != ms.shape:
        raise ValueError(f"pick_onsets: flux and mass are one row each of one length, got {fl.shape} and {ms.shape}")
    on = np.zeros(fl.shape, dtype=np.uint8)
    rc = L.vp_onset_pick(fl.ctypes.data, ms.ctypes.data, fl.size, float(thr), on.ctypes.data)
    if rc:
        raise VpError(rc, L.vp_error_string(rc).decode())
    return on


def stretch_positions_transient(onsets, n_frames, hop, stretch, n_in, frame_len=1024, span=None):
    """(pos int32 [n_frames], reset uint8 [n_frames]) through the library's vp_stretch_positions_transient: a constant stretch's table in
    which a span of 2 span + 1 frames around every accepted onset is read exactly hop apart, the stretch made up between the spans, and
    the span's first frame flagged for a phase reset (include/vp_amd.h writes the rules out).  onsets: uint8 [nG] over the input's own
    grid, nG = (n_in - frame_len) // hop + 1.  span: 1 .. 8, None = default_onset_span(frame_len, hop).  With no accepted onset the table
    is the two-anchor line, not stretch_positions's.  VpError as stretch_positions, or for a span out of range.  No device is touched."""
    L = load_library()
    K = default_onset_span(frame_len, hop) if span is None else int(span)
    on = np.ascontiguousarray(onsets, dtype=np.uint8)
    nG = L.vp_onset_num_frames(int(n_in), int(frame_len), int(hop))
    if nG < 0:
        raise VpError(nG, L.vp_error_string(nG).decode())
    if on.shape != (nG,):
        raise ValueError(f"stretch_positions_transient: onsets: [{nG}] expected, got {on.shape}")
    pos, reset = np.zeros(int(n_frames), dtype=np.int32), np.zeros(int(n_frames), dtype=np.uint8)
    rc = L.vp_stretch_positions_transient(pos.ctypes.data, reset.ctypes.data, int(n_frames), int(hop), float(stretch), int(n_in), int(frame_len), on.ctypes.data, K)
    if rc:
        raise VpError(rc, L.vp_error_string(rc).decode())
    return pos, reset


def _is(t, dtype, shape):
    """The contract of every device argument: a tensor on the GPU of this dtype and shape, contiguous."""
    return t.is_cuda and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()


_T = None                               # torch, once a helper below has needed it (the package imports without it)


def _torch():
    global _T
    import torch
    _T = torch
    return torch


def _stream_of(stream, t):
    """`stream`, or torch's current stream on t's device when there is none, as the library takes it."""
    return C.c_void_p((_T or _torch()).cuda.current_stream(t.device).cuda_stream if stream is None else stream)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _not_formant_on_locked(formant_semitones, d_formant=None):
    """A locked call's first check (callers test `locked` themselves: the other calls pay nothing for it)."""
    if formant_semitones is not None or d_formant is not None:
        raise ValueError("locked and formant_semitones exclude each other: formant correction on top of locking is not built")


def _subbin_needs_locked(locked):
    """subbin=True is a variant of the locked call (callers test `subbin` themselves)."""
    if not locked:
        raise ValueError("subbin=True needs locked=True: the sub-bin region offsets are a variant of the peak-locked call")


def _upload_ratios(tables, semitones, dev):
    """The ratios of a table of intervals (already in the kernel's layout) in a device table of that shape, allocated once per shape in
    the caller's `tables`; the copy goes on torch's current stream."""
    import torch
    r = semitones_to_ratios(semitones)
    tab = tables.get(r.shape)
    if tab is None:
        tab = tables[r.shape] = torch.empty(r.shape, dtype=torch.float64, device=dev)
    tab.copy_(torch.from_numpy(r))
    return tab


def _device_keys(owner, keys, dev):
    """The key table of a tracker call, or None: a device int32 tensor [S] as it is; host data (an int or S ints) goes into one device
    table kept on `owner` (owner._key_table), rewritten on torch's current stream."""
    import torch
    if keys is None:
        return None
    if isinstance(keys, torch.Tensor):
        assert _is(keys, torch.int32, (owner.S,))
        return keys
    k = np.asarray(keys)
    assert k.dtype.kind in "iu" and k.shape in ((), (owner.S,)), (k.dtype, k.shape)
    k = np.ascontiguousarray(np.broadcast_to(k, (owner.S,)), dtype=np.int32)
    if getattr(owner, "_key_table", None) is None:
        owner._key_table = torch.empty((owner.S,), dtype=torch.int32, device=dev)
    owner._key_table.copy_(torch.from_numpy(k))
    return owner._key_table


FORMANT_LIFTER = 32                     # the cepstral lifter's default length in samples (VP_FORMANT_LIFTER_MIN .. _MAX = 4 .. 64)


def _device_formants(owner, formant_semitones, d_formant, dev):
    """The formant table of a formant call, or None (the library's NULL: ratio 1.0 everywhere): a device float64 tensor [S] of ratios as
    it is; intervals (a scalar or S values, each |value| <= 12) go through semitones_to_ratios into one device table kept on `owner`
    (owner._formant_table), rewritten on torch's current stream."""
    import torch
    if d_formant is not None:
        assert _is(d_formant, torch.float64, (owner.S,))
        return d_formant
    st = np.asarray(0.0 if formant_semitones is None else formant_semitones, dtype=np.float64)
    assert st.shape in ((), (owner.S,)), st.shape
    r = semitones_to_ratios(np.ascontiguousarray(np.broadcast_to(st, (owner.S,))))
    if getattr(owner, "_formant_table", None) is None:
        owner._formant_table = torch.empty((owner.S,), dtype=torch.float64, device=dev)
    owner._formant_table.copy_(torch.from_numpy(r))
    return owner._formant_table


def _cross_check(d_voice, d_carrier, d_out, shape, lifter):
    """The contract of a cross-synthesis call, before anything is launched: three float32 device tensors of `shape`, contiguous, the output
    no alias of an input; the lifter within its range.  ValueError otherwise."""
    torch = _T or _torch()
    for name, t in (("voice", d_voice), ("carrier", d_carrier), ("output", d_out)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"cross_synth: {name}: a contiguous float32 tensor on the GPU expected")
    if tuple(d_voice.shape) != tuple(d_carrier.shape):
        raise ValueError(f"cross_synth: voice {tuple(d_voice.shape)} and carrier {tuple(d_carrier.shape)} differ in shape")
    for name, t in (("voice", d_voice), ("output", d_out)):
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"cross_synth: {name}: shape {tuple(shape)} expected, got {tuple(t.shape)}")
    if d_out.data_ptr() in (d_voice.data_ptr(), d_carrier.data_ptr()):
        raise ValueError("cross_synth: the output must not alias an input")
    if not 4 <= int(lifter) <= 64:
        raise ValueError("cross_synth: lifter: 4 to 64 samples expected")


def _device_depths(owner, depth, d_depth, dev):
    """The depth table of a cross-synthesis call: a device float64 tensor [S] as it is; host values (a scalar or S values, each finite) go
    into one device table kept on `owner` (owner._depth_table), rewritten on torch's current stream.  The kernel clamps to [0, 1].
    Neither (depth None): None, the library's NULL -- depth 1 everywhere."""
    torch = _T or _torch()
    if depth is None and d_depth is None:
        return None
    if d_depth is not None:
        if not _is(d_depth, torch.float64, (owner.S,)):
            raise ValueError(f"cross_synth: d_depth: a contiguous float64 tensor [{owner.S}] on the GPU expected")
        return d_depth
    d = np.asarray(depth, dtype=np.float64)
    if d.shape not in ((), (owner.S,)) or not np.all(np.isfinite(d)):
        raise ValueError(f"cross_synth: depth: one finite value or {owner.S} of them expected")
    if getattr(owner, "_depth_table", None) is None:
        owner._depth_table = torch.empty((owner.S,), dtype=torch.float64, device=dev)
    owner._depth_table.copy_(torch.from_numpy(np.array(np.broadcast_to(d, (owner.S,)))))
    return owner._depth_table


HARM_MAX_VOICES = 4                     # VP_HARM_MAX_VOICES


def _harm_io(d_in, d_out, shape):
    """The contract of a harmonizer call's input and output, before anything is launched: float32 device tensors of `shape`, contiguous.
    ValueError otherwise."""
    torch = _T or _torch()
    for name, t in (("input", d_in), ("output", d_out)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"harmonize: {name}: a contiguous float32 tensor on the GPU expected")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"harmonize: {name}: shape {tuple(shape)} expected, got {tuple(t.shape)}")


def _harm_levels(owner, V, gains, dry, dev):
    """The gain and dry tables of a harmonizer call as device float64 tensors [S][V] and [S], or None for the library's NULL (every gain
    1; no dry part).  A device tensor is used as it is; host values -- gains [V] or [S][V], dry a scalar or [S] -- go into tables kept on
    `owner`, rewritten on torch's current stream.  The kernel clamps to [-4, 4] and takes a NaN or an infinity as 0."""
    torch = _T or _torch()
    S = owner.S

    def table(x, name, shape, admitted, slot):
        if x is None:
            return None
        if isinstance(x, torch.Tensor):
            if not _is(x, torch.float64, shape):
                raise ValueError(f"harmonize: {name}: a contiguous float64 tensor {list(shape)} on the GPU expected")
            return x
        a = np.asarray(x, dtype=np.float64)
        if a.shape not in admitted:
            raise ValueError(f"harmonize: {name}: shape {a.shape}, one of {admitted} expected")
        tabs = owner.__dict__.setdefault("_harm_tables", {})
        if (slot, shape) not in tabs:
            tabs[(slot, shape)] = torch.empty(shape, dtype=torch.float64, device=dev)
        tabs[(slot, shape)].copy_(torch.from_numpy(np.array(np.broadcast_to(a, shape))))
        return tabs[(slot, shape)]
    return table(gains, "gains", (S, V), [(V,), (S, V)], "gain"), table(dry, "dry", (S,), [(), (S,)], "dry")


TRACK_INTEGER, TRACK_FINE = 0, 1        # VP_TRACK_INTEGER, VP_TRACK_FINE: the tracker mode of a handle
HARM_MAX_DEGREE = 12                    # VP_TRACK_MAX_DEGREE: the kernels clamp a degree to +-12 steps of the key's table


def _host_keys(keys, S):
    """`keys` as S ints with values outside 0 .. 12 counted as 12 (None: chromatic), or None when it is a device tensor."""
    if keys is None:
        return np.full((S,), 12, np.int64)
    if not isinstance(keys, (int, np.integer, list, tuple, np.ndarray)):
        return None
    k = np.broadcast_to(np.asarray(keys), (S,)).astype(np.int64)
    return np.where((k < 0) | (k > 12), 12, k)


def _voice_tables(owner, degrees, keys, unvoiced, dev, V=None):
    """The degree and unvoiced tables of a key-aware voices call as device tensors (int32 [S][V], float64 [S][V]), and V.  degrees: V ints
    for every stream or [S][V], V = 1 .. 4 (`V` given: exactly that many), or a device int32 tensor [S][V].  unvoiced: [V], [S][V], a device
    float64 tensor [S][V], or None = each voice's nominal interval, 2^(d / 12) in the chromatic key and 2^(round(12 d / 7) / 12) in a scale
    key, computed here on the host (it needs host degrees and host keys: ValueError otherwise).  Host data goes into tables kept on `owner`,
    rewritten on torch's current stream.  ValueError before anything is launched."""
    torch = _T or _torch()
    S = owner.S
    host = None
    if isinstance(degrees, torch.Tensor):
        if not (degrees.is_cuda and degrees.dtype == torch.int32 and degrees.dim() == 2 and degrees.is_contiguous() and degrees.shape[0] == S
                and 1 <= degrees.shape[1] <= HARM_MAX_VOICES):
            raise ValueError(f"degrees: a contiguous int32 tensor [{S}][V] on the GPU with V = 1 .. {HARM_MAX_VOICES} expected")
        d_degree, nV = degrees, int(degrees.shape[1])
    else:
        host = np.asarray(degrees)
        if host.dtype.kind not in "iu" or host.ndim not in (1, 2) or not 1 <= host.shape[-1] <= HARM_MAX_VOICES or (host.ndim == 2 and host.shape[0] != S):
            raise ValueError(f"degrees: V integers or [{S}][V] of them with V = 1 .. {HARM_MAX_VOICES} expected, got {np.shape(degrees)}")
        nV = int(host.shape[-1])
        host = np.array(np.broadcast_to(host, (S, nV)), dtype=np.int32)             # (a copy: torch wants it writable)
        d_degree = None
    if V is not None and nV != V:
        raise ValueError(f"degrees: {V} voices expected, got {nV}")
    if unvoiced is None:
        k = _host_keys(keys, S)
        if host is None or k is None:
            raise ValueError("unvoiced=None (the nominal intervals) needs degrees and keys on the host: pass an unvoiced table")
        d = np.clip(host, -HARM_MAX_DEGREE, HARM_MAX_DEGREE).astype(np.float64)
        semis = np.where(k[:, None] == 12, d, np.floor(12.0 * d / 7.0 + 0.5))
        u = 2.0 ** (semis / 12.0)
    elif isinstance(unvoiced, torch.Tensor):
        if not _is(unvoiced, torch.float64, (S, nV)):
            raise ValueError(f"unvoiced: a contiguous float64 tensor [{S}][{nV}] on the GPU expected")
        u = None
    else:
        u = np.asarray(unvoiced, dtype=np.float64)
        if u.shape not in ((nV,), (S, nV)):
            raise ValueError(f"unvoiced: [{nV}] or [{S}][{nV}] expected, got {u.shape}")
        u = np.broadcast_to(u, (S, nV))
    tabs = owner.__dict__.setdefault("_voice_tabs", {})
    if d_degree is None:
        if ("deg", nV) not in tabs:
            tabs[("deg", nV)] = torch.empty((S, nV), dtype=torch.int32, device=dev)
        d_degree = tabs[("deg", nV)]
        d_degree.copy_(torch.from_numpy(host))
    if u is None:
        return d_degree, unvoiced, nV
    if ("unv", nV) not in tabs:
        tabs[("unv", nV)] = torch.empty((S, nV), dtype=torch.float64, device=dev)
    tabs[("unv", nV)].copy_(torch.from_numpy(np.array(u)))
    return d_degree, tabs[("unv", nV)], nV


class _Handle:
    """The lifecycle of a library handle: <_prefix>_create or VpError, _chk for every later call, close() and __del__ through
    <_prefix>_destroy."""
    _prefix = None

    def _open(self, *args):
        self.L = load_library()
        self._destroy = getattr(self.L, self._prefix + "_destroy")
        h = C.c_void_p()
        self._chk(getattr(self.L, self._prefix + "_create")(*args, C.byref(h)))
        self.h = h

    def _chk(self, rc):
        if rc:
            raise VpError(rc, self.L.vp_error_string(rc).decode())

    def close(self):
        if getattr(self, "h", None):
            self._destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _StreamHandle(_Handle):
    """... of a handle that keeps per-stream state across process calls: reset() and the allocation count too."""

    def _open(self, *args):
        try:
            import torch  # noqa: F401  (run() and process_device() use torch: load its HIP runtime before the library loads one)
        except ImportError:
            pass
        super()._open(*args)
        self._reset, self._alloc_count = getattr(self.L, self._prefix + "_reset"), getattr(self.L, self._prefix + "_debug_alloc_count")

    def reset(self, stream=-1):
        """The stream (-1: all) starts again like a fresh one at the next process call (a PhaseVocoderStream's interval stays; a tracker
        has no history and no held ratio)."""
        self._chk(self._reset(self.h, int(stream)))

    def debug_alloc_count(self):
        return self._alloc_count(self.h)


class _BlockStream(_StreamHandle):
    """... of a stream of audio blocks [S][N] in and out: what the run() methods share.  Each kind has its `latency`."""

    def _n_blocks(self, T):
        """(n_blocks, latency) of a run over T samples: the input padded with `latency` zeros and up to whole blocks."""
        lat = self.latency
        return -(-(T + lat) // self.N), lat

    def _slab(self, x, nb):
        """The host array [S][T], zero-padded to nb blocks, as the device slab [nb][S][N]."""
        import torch
        xp = np.zeros((self.S, nb * self.N), np.float32)
        xp[:, :x.shape[1]] = x
        return torch.from_numpy(np.ascontiguousarray(xp.reshape(self.S, nb, self.N).transpose(1, 0, 2))).to(torch.device("cuda", self.device))

    def _trimmed(self, d_out, T, lat):
        """The device slab [nb][S][N], once its stream's work is done, as the host array [S][T] aligned with the input: the first `lat`
        samples dropped."""
        import torch
        torch.cuda.synchronize(d_out.device)
        y = d_out.cpu().numpy().transpose(1, 0, 2).reshape(self.S, -1)
        return np.ascontiguousarray(y[:, lat:lat + T])


class StftRoundTrip(_Handle):
    """Standalone batched STFT -> iSTFT (no reference counterpart; see include/vp_amd.h vp_stft_*)."""
    _prefix = "vp_stft"

    def __init__(self, n_streams, n_samples, frame_len=1024, hop=256, device=0):
        self._open(int(device), int(n_streams), int(n_samples), int(frame_len), int(hop))
        self.S, self.T, self.F, self.hop = n_streams, n_samples, frame_len, hop
        self.n_frames = self.L.vp_stft_num_frames(self.h)
        self._curve_tables, self._stretch_tables = {}, {}      # device ratio / position tables, one per shape, allocated at first use

    def __call__(self, d_in, d_out, d_mag=None, stream=None):
        self._io(d_in, d_out)
        self._chk(self.L.vp_stft_roundtrip(self.h, d_in.data_ptr(), d_out.data_ptr(), _ptr(d_mag), _stream_of(stream, d_in)))

    @property
    def fused(self):
        """True when the handle runs the fused kernel (csrc/vp_stft.hip: 1024-point frames)."""
        return self.L.vp_stft_is_fused(self.h) == 1

    def set_runs(self, runs_per_stream):
        """Diagnostic: runs of frames (workgroups) per stream, 0 = automatic; the output does not depend on it."""
        self._chk(self.L.vp_stft_set_runs(self.h, int(runs_per_stream)))

    def set_precision(self, precision):
        """"f64" (default) or "f32": arithmetic of the round trip's transforms (vp_stft_set_precision)."""
        self._chk(self.L.vp_stft_set_precision(self.h, {"f64": 0, "f32": 1}[precision]))

    @property
    def precision(self):
        return "f32" if self.L.vp_stft_get_precision(self.h) == 1 else "f64"

    def _io(self, d_in, d_out, any_length=False):
        """The contract of a call's input and output: device float32 [S][n_samples], contiguous (any_length: the input is [S][n_in] with
        n_in >= frame_len).  Returns the input's row length."""
        f32 = (_T or _torch()).float32
        n_in = int(d_in.shape[1]) if any_length and d_in.dim() == 2 else self.T
        assert d_in.is_cuda and d_in.dtype == f32 and tuple(d_in.shape) == (self.S, n_in) and d_in.is_contiguous()
        assert d_out.is_cuda and d_out.dtype == f32 and tuple(d_out.shape) == (self.S, self.T) and d_out.is_contiguous()
        assert n_in >= self.F, n_in
        return n_in

    def _ratio_table(self, semitones, d_ratio, dev, scalar=False, per_stream=False, none_is_zero=False):
        """`semitones` or `d_ratio` as the checked device ratio table [S][n_frames] of a call.  Host intervals are [n_frames] or
        [S][n_frames], with `scalar` also one value, with `per_stream` also [S] (when S != n_frames: a vector of n_frames is a curve); they
        become ratios in the device table the handle keeps per shape.  none_is_zero: neither given means no shift."""
        torch = _T or _torch()
        if none_is_zero:
            assert semitones is None or d_ratio is None, "at most one of semitones and d_ratio"
            semitones = 0.0 if semitones is None and d_ratio is None else semitones
        assert (semitones is None) != (d_ratio is None), "one of semitones and d_ratio"
        if d_ratio is None:
            st = np.asarray(semitones, dtype=np.float64)
            if per_stream and st.shape == (self.S,) and self.S != self.n_frames:
                st = st[:, None]
            admitted = [(self.n_frames,), (self.S, self.n_frames)] + [()] * scalar + [(self.S, 1)] * per_stream
            assert st.shape in admitted, st.shape
            d_ratio = _upload_ratios(self._curve_tables, np.broadcast_to(st, (self.S, self.n_frames)), dev)
        assert _is(d_ratio, torch.float64, (self.S, self.n_frames))
        return d_ratio

    def pitch_shift(self, d_in, d_out, semitones, stream=None):
        """Round trip with the phase-vocoder stage (per-bin phase unwrap / accumulate) shifting the pitch by `semitones`
        (|semitones| <= 12), for 1024- and 2048-point frames at every hop the handle admits.  Always double precision
        (set_precision has no effect on it); every call starts from zero phase state."""
        self._io(d_in, d_out)
        self._chk(self.L.vp_stft_pitch_shift(self.h, d_in.data_ptr(), d_out.data_ptr(), float(semitones), _stream_of(stream, d_in)))

    def pitch_shift_curve(self, d_in, d_out, semitones=None, stream=None, d_ratio=None):
        """pitch_shift along a pitch curve (vp_stft_pitch_shift_curve): `semitones` is array-like [n_frames] (every stream follows it) or
        [S][n_frames], each |value| <= 12; frame f of stream s is shifted by semitones[s][f].  The intervals become ratios through
        semitones_to_ratios and are uploaded into a device table the handle allocates once (on torch's current stream: with another
        `stream`, order it behind that one).  d_ratio instead: a device float64 tensor [S][n_frames] of ratios, used as it is (the
        kernel clamps to [0.5, 2])."""
        self._io(d_in, d_out)
        d_ratio = self._ratio_table(semitones, d_ratio, d_in.device)
        self._chk(self.L.vp_stft_pitch_shift_curve(self.h, d_in.data_ptr(), d_out.data_ptr(), d_ratio.data_ptr(), _stream_of(stream, d_in)))

    def pitch_shift_locked(self, d_in, d_out, semitones=None, stream=None, d_ratio=None, subbin=False):
        """pitch_shift_curve with peak locking (vp_stft_pitch_shift_locked; 1024-point frames): every frame's spectral peaks are found and a
        peak's whole region of bins moves by one integer offset and turns by one accumulated angle, so a sinusoid's main lobe stays one
        windowed sinusoid (the definition is tests/pv_lock_reference.py).  `semitones`, `d_ratio` and `stream` as in pitch_shift_curve --
        the same table-building path.  A 2048-point handle raises VpError (VP_ERR_GEOMETRY).
        subbin=True: vp_stft_pitch_shift_locked_subbin -- a region is translated by the real-valued offset of its peak's interpolated
        centre and the spectrum interpolated with six taps, so a shifted tone keeps its level (tests/pv_lockf_reference.py)."""
        self._io(d_in, d_out)
        d_ratio = self._ratio_table(semitones, d_ratio, d_in.device)
        call = self.L.vp_stft_pitch_shift_locked_subbin if subbin else self.L.vp_stft_pitch_shift_locked
        self._track_chk(call(self.h, d_in.data_ptr(), d_out.data_ptr(), d_ratio.data_ptr(), _stream_of(stream, d_in)))

    def pitch_shift_formant(self, d_in, d_out, semitones=None, stream=None, d_ratio=None, formant_semitones=0.0, lifter=FORMANT_LIFTER, d_formant=None):
        """pitch_shift_curve with the spectral envelope kept apart from the pitch (vp_stft_pitch_shift_formant; 1024-point frames): the
        formants stay where they were (formant_semitones = 0, the default) or move by an interval of their own, a scalar or [S] values,
        |value| <= 12 (d_formant instead: a device float64 tensor [S] of ratios, used as it is).  `semitones`: a scalar, [S] (one interval
        per stream; with S == n_frames a vector is a curve), [n_frames] or [S][n_frames]; d_ratio as in pitch_shift_curve -- the same
        table-building path.  lifter: length of the cepstral lifter in samples, 4 .. 64 (short: a smoother envelope)."""
        self._io(d_in, d_out)
        d_ratio = self._ratio_table(semitones, d_ratio, d_in.device, scalar=True, per_stream=True)
        d_formant = _device_formants(self, formant_semitones, d_formant, d_in.device)
        self._track_chk(self.L.vp_stft_pitch_shift_formant(self.h, d_in.data_ptr(), d_out.data_ptr(), d_ratio.data_ptr(), d_formant.data_ptr(), int(lifter),
                                                           _stream_of(stream, d_in)))

    def harmonize(self, d_in, d_out, semitones=None, d_ratio=None, gains=None, dry=None, stream=None, degrees=None, sample_rate=None, keys=None,
                  unvoiced=None):
        """The harmonizer (vp_stft_harmonize; 1024-point frames): V = 1 .. 4 peak-locked voices, each shifted by its own interval and mixed
        by its own gain, beside the dry signal, from one analysis of every frame -- dry roundtrip(x) + sum_v gains[v] pitch_shift_locked(x,
        semitones[v]) (the definition is tests/pv_harm_reference.py).  `semitones`: [V] fixed intervals, [V][n_frames] one curve per voice
        for every stream, or [S][V][n_frames], each |value| <= 12; they become ratios through semitones_to_ratios in a device table the
        handle keeps per shape.  d_ratio instead: a device float64 tensor [S][V][n_frames], used as it is (the kernel clamps to [0.5, 2]).
        gains: None (every gain 1), [V], [S][V] or a device float64 tensor [S][V]; dry: None (no dry part), a scalar, [S] or a device
        float64 tensor [S].  One voice with gain 1 and no dry part has pitch_shift_locked's bits.
        degrees=..., sample_rate=... [, keys=..., unvoiced=...] instead of both: the voices sit at scale degrees of the tracked pitch
        (vp_stft_harmonize_key: track_harmony, then this call along its table, on one stream); returns track_harmony's (period, ratio).
        Wrong dtypes or shapes, or more than one of semitones, d_ratio and degrees, raise ValueError before any launch; a 2048-point handle
        raises VpError."""
        torch = _T or _torch()
        _harm_io(d_in, d_out, (self.S, self.T))
        if (semitones is not None) + (d_ratio is not None) + (degrees is not None) != 1:
            raise ValueError("harmonize: exactly one of semitones, d_ratio and degrees expected")
        if degrees is not None:
            if sample_rate is None:
                raise ValueError("harmonize: degrees need sample_rate")
            d_degree, d_unv, V = _voice_tables(self, degrees, keys, unvoiced, d_in.device)
            d_gain, d_dry = _harm_levels(self, V, gains, dry, d_in.device)
            d_key, period, ratio = self._track_tables(keys, d_in.device, V)
            self._track_chk(self.L.vp_stft_harmonize_key(self.h, d_in.data_ptr(), d_out.data_ptr(), float(sample_rate), _ptr(d_key), V, d_degree.data_ptr(),
                                                         _ptr(d_unv), _ptr(d_gain), _ptr(d_dry), period.data_ptr(), ratio.data_ptr(),
                                                         _stream_of(stream, d_in)))
            return period, ratio
        if sample_rate is not None or keys is not None or unvoiced is not None:
            raise ValueError("harmonize: sample_rate, keys and unvoiced go with degrees")
        nF = self.n_frames
        if d_ratio is None:
            st = np.asarray(semitones, dtype=np.float64)
            if st.ndim == 1:
                st = st[:, None]
            elif st.ndim == 3 and st.shape[0] != self.S:
                raise ValueError(f"harmonize: semitones: [{self.S}][V][{nF}] expected, got {st.shape}")
            if st.ndim not in (2, 3) or not 1 <= st.shape[-2] <= HARM_MAX_VOICES or st.shape[-1] not in (1, nF):
                raise ValueError(f"harmonize: semitones: [V], [V][{nF}] or [{self.S}][V][{nF}] with V = 1 .. {HARM_MAX_VOICES} expected, got {np.shape(semitones)}")
            V = st.shape[-2]
            d_ratio = _upload_ratios(self._curve_tables, np.broadcast_to(st, (self.S, V, nF)), d_in.device)
        else:
            if not (d_ratio.is_cuda and d_ratio.dtype == torch.float64 and d_ratio.dim() == 3 and d_ratio.is_contiguous()
                    and 1 <= d_ratio.shape[1] <= HARM_MAX_VOICES and tuple(d_ratio.shape) == (self.S, d_ratio.shape[1], nF)):
                raise ValueError(f"harmonize: d_ratio: a contiguous float64 tensor [{self.S}][V][{nF}] on the GPU with V = 1 .. {HARM_MAX_VOICES} expected")
            V = int(d_ratio.shape[1])
        d_gain, d_dry = _harm_levels(self, V, gains, dry, d_in.device)
        self._track_chk(self.L.vp_stft_harmonize(self.h, d_in.data_ptr(), d_out.data_ptr(), V, d_ratio.data_ptr(), _ptr(d_gain), _ptr(d_dry),
                                                 _stream_of(stream, d_in)))

    def cross_synth(self, d_voice, d_carrier, d_out, depth=1.0, lifter=FORMANT_LIFTER, stream=None, d_depth=None):
        """STFT cross-synthesis (vp_stft_cross_synth; 1024-point frames): the spectral envelope of d_voice imposed on d_carrier, frame by
        frame -- the carrier's bins times exp(min(depth (env voice - env carrier), ln 256)) with pitch_shift_formant's cepstral envelope
        (the definition is tests/pv_cross_reference.py).  d_voice, d_carrier, d_out: device float32 [S][n_samples], the output no alias of
        an input.  depth: 0 (the carrier's plain round trip, bit for bit) .. 1, a scalar or [S] values, None for the library's NULL table (1
        everywhere); d_depth instead: a device float64 tensor [S], used as it is (the kernel clamps to [0, 1]).  lifter: the cepstral lifter, 4 .. 64 samples.  Always double precision;
        set_runs applies.  Wrong dtypes, shapes or lifter raise ValueError before any launch; a 2048-point handle raises VpError."""
        _cross_check(d_voice, d_carrier, d_out, (self.S, self.T), lifter)
        d_depth = _device_depths(self, depth, d_depth, d_voice.device)
        self._track_chk(self.L.vp_stft_cross_synth(self.h, d_voice.data_ptr(), d_carrier.data_ptr(), d_out.data_ptr(), _ptr(d_depth), int(lifter),
                                                   _stream_of(stream, d_voice)))

    def _position_table(self, positions, stretch, d_pos, n_in, dev):
        """The checked device position table [S][n_frames] of a time-stretch call: d_pos as it is, or host data -- `stretch` through
        stretch_positions, `positions` broadcast and clipped to int32 -- in the device table the handle keeps per shape
        (self._stretch_tables), rewritten on torch's current stream."""
        torch = _T or _torch()
        assert (positions is not None) + (stretch is not None) + (d_pos is not None) == 1, "one of positions, stretch and d_pos"
        if stretch is not None:
            a = np.broadcast_to(np.asarray(stretch, dtype=np.float64).reshape(-1), (self.S,))
            pos = np.stack([stretch_positions(self.n_frames, self.hop, v, n_in, self.F) for v in a])
        elif positions is not None:
            pos = np.asarray(positions)
            assert pos.dtype.kind in "iu" and pos.shape in ((self.n_frames,), (self.S, self.n_frames)), (pos.dtype, pos.shape)
            pos = np.clip(np.broadcast_to(pos, (self.S, self.n_frames)), -2 ** 31, 2 ** 31 - 1).astype(np.int32)
        if d_pos is None:
            d_pos = self._stretch_tables.get(pos.shape)
            if d_pos is None:
                d_pos = self._stretch_tables[pos.shape] = torch.empty(pos.shape, dtype=torch.int32, device=dev)
            d_pos.copy_(torch.from_numpy(np.ascontiguousarray(pos)))
        assert _is(d_pos, torch.int32, (self.S, self.n_frames))
        return d_pos

    def time_stretch(self, d_in, d_out, positions=None, stretch=None, semitones=0.0, stream=None, d_pos=None):
        """Time stretch (vp_stft_time_stretch): pitch_shift with frame f of stream s analysed at input sample positions[s][f] and written
        at output sample f hop, so duration and pitch are independent.  d_in is float32 [S][n_in] with any n_in >= frame_len, d_out
        [S][n_samples] (the handle's length is the OUTPUT's).  One of
          positions: array-like int [n_frames] (every stream follows it) or [S][n_frames];
          stretch:   output duration / input duration in [0.25, 4], a scalar or [S] -- tables through stretch_positions;
          d_pos:     a device int32 tensor [S][n_frames], used as it is.
        The kernel clamps positions to [0, n_in - frame_len]; any table gives a finite output.  positions and stretch are uploaded into a
        device table the handle allocates once per shape (on torch's current stream: with another `stream`, order it behind that one).
        semitones (|value| <= 12): the pitch shift on top, 0 = pure stretch.  Always double precision; every call starts from zero phase
        state."""
        n_in = self._io(d_in, d_out, any_length=True)
        d_pos = self._position_table(positions, stretch, d_pos, n_in, d_in.device)
        self._chk(self.L.vp_stft_time_stretch(self.h, d_in.data_ptr(), n_in, d_pos.data_ptr(), d_out.data_ptr(), float(semitones), _stream_of(stream, d_in)))

    def onset_flux(self, d_in, d_flux=None, d_mass=None, stream=None):
        """The onset flux of the input's own frame grid (vp_stft_onset_flux; 1024-point frames): d_in float32 [S][n_in], any
        n_in >= frame_len -> (flux, mass), device float64 [S][nG], nG = (n_in - frame_len) // hop + 1: mass[g] the sum of frame g's 513
        magnitudes, flux[g] the sum of their rises over frame g - 1 (flux[0] = 0).  d_flux, d_mass: tensors to write into; None: new ones,
        the caller's to keep.  No synchronisation.  The host picks the onsets (pick_onsets) and plans around them
        (stretch_positions_transient)."""
        torch = _T or _torch()
        assert d_in.is_cuda and d_in.dtype == torch.float32 and d_in.dim() == 2 and d_in.shape[0] == self.S and d_in.is_contiguous()
        n_in = int(d_in.shape[1])
        assert n_in >= self.F, n_in
        nG = (n_in - self.F) // self.hop + 1
        if d_flux is None:
            d_flux = torch.empty((self.S, nG), dtype=torch.float64, device=d_in.device)
        if d_mass is None:
            d_mass = torch.empty((self.S, nG), dtype=torch.float64, device=d_in.device)
        assert _is(d_flux, torch.float64, (self.S, nG)) and _is(d_mass, torch.float64, (self.S, nG))
        self._track_chk(self.L.vp_stft_onset_flux(self.h, d_in.data_ptr(), n_in, d_flux.data_ptr(), d_mass.data_ptr(), _stream_of(stream, d_in)))
        return d_flux, d_mass

    def _transient_tables(self, d_in, n_in, stretch, thr, span, stream):
        """flux -> copy -> pick and plan per stream -> upload: the device position and reset tables of a transients= call.  ONE
        synchronisation: the copy of the flux tables to the host."""
        torch = _T or _torch()
        assert stretch is not None, "transients= plans a constant stretch: give stretch="
        a = np.broadcast_to(np.asarray(stretch, dtype=np.float64).reshape(-1), (self.S,))
        d_flux, d_mass = self.onset_flux(d_in, stream=stream)
        both = torch.stack((d_flux, d_mass)).cpu().numpy()                    # (the call's one synchronisation)
        pos, reset = np.empty((self.S, self.n_frames), np.int32), np.empty((self.S, self.n_frames), np.uint8)
        for s in range(self.S):
            pos[s], reset[s] = stretch_positions_transient(pick_onsets(both[0, s], both[1, s], thr), self.n_frames, self.hop, a[s], n_in, self.F, span)
        d_reset = self._stretch_tables.get("reset")
        if d_reset is None or tuple(d_reset.shape) != reset.shape:
            d_reset = self._stretch_tables["reset"] = torch.empty(reset.shape, dtype=torch.uint8, device=d_in.device)
        d_reset.copy_(torch.from_numpy(reset))
        return self._position_table(pos, None, None, n_in, d_in.device), d_reset

    def time_stretch_locked(self, d_in, d_out, positions=None, stretch=None, semitones=None, stream=None, d_pos=None, d_ratio=None, d_reset=None,
                            transients=None, span=None):
        """time_stretch with peak locking (vp_stft_time_stretch_locked; 1024-point frames): the frames are analysed at the table's positions
        as in time_stretch, and the stage between the transforms is pitch_shift_locked's with the frame's own analysis advance -- a
        sinusoid's main lobe stays one windowed sinusoid under any stretch, with or without a pitch shift on top (the definition is
        tests/pv_stretch_lock_reference.py).  positions, stretch and d_pos as in time_stretch, from the same per-handle tables.  The pitch
        is per frame and per stream: `semitones` a scalar, [n_frames] (every stream follows the curve) or [S][n_frames], each |value| <= 12,
        None = no shift; d_ratio instead: a device float64 tensor [S][n_frames] of ratios, used as it is (the kernel clamps to [0.5, 2]).
        A 2048-point handle raises VpError (VP_ERR_GEOMETRY).
        d_reset: a device uint8 tensor [S][n_frames]; a frame with a non-zero byte restarts the angles (vp_stft_time_stretch_locked_reset:
        every peak's angle is 0 there), an all-zero table gives the call without it, bit for bit.
        transients=thr (with stretch=; True: the default threshold 0.2): the transient-preserving stretch in one call -- onset_flux,
        the flux tables copied to the host, pick_onsets(thr) and stretch_positions_transient(span) per stream against the input's
        length, the tables uploaded, the reset kernel.  It SYNCHRONISES ONCE, for the copy of the flux tables; the explicit four steps
        give the same bits.  span: the span's half width in frames, 1 .. 8, None = max(frame_len / (2 hop), 1)."""
        n_in = self._io(d_in, d_out, any_length=True)
        if transients is not None and transients is not False:
            assert positions is None and d_pos is None and d_reset is None, "transients= plans its own tables from stretch="
            thr = ONSET_THRESHOLD if transients is True else float(transients)
            d_pos, d_reset = self._transient_tables(d_in, n_in, stretch, thr, span, stream)
        else:
            d_pos = self._position_table(positions, stretch, d_pos, n_in, d_in.device)
        d_ratio = self._ratio_table(semitones, d_ratio, d_in.device, scalar=True, none_is_zero=True)
        if d_reset is not None:
            assert _is(d_reset, (_T or _torch()).uint8, (self.S, self.n_frames))
            self._track_chk(self.L.vp_stft_time_stretch_locked_reset(self.h, d_in.data_ptr(), n_in, d_pos.data_ptr(), d_out.data_ptr(), d_ratio.data_ptr(),
                                                                     d_reset.data_ptr(), _stream_of(stream, d_in)))
            return
        self._track_chk(self.L.vp_stft_time_stretch_locked(self.h, d_in.data_ptr(), n_in, d_pos.data_ptr(), d_out.data_ptr(), d_ratio.data_ptr(),
                                                           _stream_of(stream, d_in)))

    def _track_tables(self, keys, dev, V=None):
        """(d_key or None, period, ratio): the call's key table and outputs.  The key table is kept per handle (one device int32 [S],
        rewritten on torch's current stream when `keys` is host data); the outputs are new tensors, the caller's to keep.  V: the ratio
        table of a voices call, [S][V][n_frames]."""
        import torch
        d_key = _device_keys(self, keys, dev)
        period = torch.empty((self.S, self.n_frames), dtype=torch.int32, device=dev)
        ratio = torch.empty((self.S, self.n_frames) if V is None else (self.S, V, self.n_frames), dtype=torch.float64, device=dev)
        return d_key, period, ratio

    def _track_chk(self, rc):
        if rc:
            msg = self.L.vp_stft_last_error(self.h).decode()
            raise VpError(rc, msg or self.L.vp_error_string(rc).decode())

    def set_track_mode(self, fine):
        """fine=True: the calls that track (track_pitch, autotune, track_harmony, harmonize with degrees) use the fine tracker
        (vp_stft_set_track_mode, VP_TRACK_FINE): the period refined below one sample by a parabola through the normalised difference
        function's minimum, the note looked up on the refined pitch.  False (the default): the integer period, today's bits."""
        rc = self.L.vp_stft_set_track_mode(self.h, TRACK_FINE if fine else TRACK_INTEGER)
        if rc:
            raise VpError(rc, self.L.vp_error_string(rc).decode())

    @property
    def track_fine(self):
        return self.L.vp_stft_get_track_mode(self.h) == TRACK_FINE

    def track_pitch(self, d_in, sample_rate, keys=None, stream=None, with_fine_period=False):
        """The pitch tracker (vp_stft_track_pitch): PitchProcess's YIN and nearest note for every frame of the batch at once.  Returns
        (period, ratio), device tensors int32 / float64 [S][n_frames]: the period in samples (0 = unvoiced) and the ratio
        closestFreq / pitch that moves the frame onto its key's nearest note (1.0 where unvoiced) -- the table pitch_shift_curve(d_ratio=...)
        takes.  keys: Notes::key per stream, 0..12 (12 = chromatic, also for any value outside the range): an int, a sequence of S ints or
        a device int32 tensor [S]; None = chromatic.  8000 <= sample_rate <= 51200 and n_samples >= frame_len + ceil(sample_rate / 100)
        (VpError otherwise).  Frames are independent: no smoothing, no hold across unvoiced frames.
        with_fine_period=True: the fine tracker whatever the mode (vp_stft_track_pitch_fine); returns (period, ratio, period_fine), the
        third a float64 [S][n_frames] table of refined periods (0.0 where unvoiced)."""
        import torch
        assert _is(d_in, torch.float32, (self.S, self.T))
        d_key, period, ratio = self._track_tables(keys, d_in.device)
        if with_fine_period:
            fine = torch.empty((self.S, self.n_frames), dtype=torch.float64, device=d_in.device)
            self._track_chk(self.L.vp_stft_track_pitch_fine(self.h, d_in.data_ptr(), float(sample_rate), _ptr(d_key), period.data_ptr(), fine.data_ptr(),
                                                            ratio.data_ptr(), _stream_of(stream, d_in)))
            return period, ratio, fine
        self._track_chk(self.L.vp_stft_track_pitch(self.h, d_in.data_ptr(), float(sample_rate), _ptr(d_key), period.data_ptr(), ratio.data_ptr(),
                                                   _stream_of(stream, d_in)))
        return period, ratio

    def track_harmony(self, d_in, sample_rate, degrees, keys=None, unvoiced=None, stream=None):
        """Key-aware voices (vp_stft_track_harmony): track_pitch's decision for every frame, then one ratio per voice that puts it
        `degrees[v]` steps of the key's table (scale degrees in a scale key, semitones in the chromatic key; clamped to +-12) from the note
        the tracker chose.  Returns (period, ratio), device tensors int32 [S][n_frames] / float64 [S][V][n_frames] -- the table
        harmonize(d_ratio=...) takes.  degrees: V ints for every stream or [S][V], V = 1 .. 4; keys as track_pitch's; unvoiced: the ratio of
        unvoiced frames, [V] or [S][V], None = each voice's nominal interval (2^(d / 12) chromatic, 2^(round(12 d / 7) / 12) in a scale
        key).  Degree 0 gives track_pitch's ratio bit for bit.  Wrong shapes raise ValueError before any launch."""
        torch = _T or _torch()
        if not _is(d_in, torch.float32, (self.S, self.T)):
            raise ValueError(f"track_harmony: input: a contiguous float32 tensor [{self.S}][{self.T}] on the GPU expected")
        d_degree, d_unv, V = _voice_tables(self, degrees, keys, unvoiced, d_in.device)
        d_key, period, ratio = self._track_tables(keys, d_in.device, V)
        self._track_chk(self.L.vp_stft_track_harmony(self.h, d_in.data_ptr(), float(sample_rate), _ptr(d_key), V, d_degree.data_ptr(), _ptr(d_unv),
                                                     period.data_ptr(), ratio.data_ptr(), _stream_of(stream, d_in)))
        return period, ratio

    def autotune(self, d_in, d_out, sample_rate, keys=None, stream=None, formant_semitones=None, lifter=FORMANT_LIFTER, locked=False, subbin=False):
        """Automatic pitch correction (vp_stft_autotune): track_pitch, then pitch_shift_curve along its ratios, on one stream; d_out has
        the bits of those two calls.  Returns track_pitch's (period, ratio).
        formant_semitones (a scalar or [S]; None: the call above, unchanged): the correction runs through pitch_shift_formant instead
        (vp_stft_autotune_formant) -- 0 keeps the formants where the singer had them.
        locked=True: track_pitch followed by pitch_shift_locked along its ratios, on the same stream (not together with
        formant_semitones: ValueError before any launch).  subbin=True (with locked=True only: ValueError otherwise, before any launch):
        the locked call is pitch_shift_locked(subbin=True)."""
        self._io(d_in, d_out)
        if locked:
            _not_formant_on_locked(formant_semitones)
        if subbin:
            _subbin_needs_locked(locked)
        if locked:
            period, ratio = self.track_pitch(d_in, sample_rate, keys=keys, stream=stream)
            self.pitch_shift_locked(d_in, d_out, stream=stream, d_ratio=ratio, **({"subbin": True} if subbin else {}))
            return period, ratio
        d_key, period, ratio = self._track_tables(keys, d_in.device)
        head = (self.h, d_in.data_ptr(), d_out.data_ptr(), float(sample_rate), _ptr(d_key), period.data_ptr(), ratio.data_ptr())
        if formant_semitones is not None:
            d_formant = _device_formants(self, formant_semitones, None, d_in.device)
            self._track_chk(self.L.vp_stft_autotune_formant(*head, d_formant.data_ptr(), int(lifter), _stream_of(stream, d_in)))
        else:
            self._track_chk(self.L.vp_stft_autotune(*head, _stream_of(stream, d_in)))
        return period, ratio


class PhaseVocoderStream(_BlockStream):
    """Streaming phase-vocoder pitch shifter: `n_streams` independent streams, blocks of `block_size` samples, state kept across
    calls (include/vp_amd.h vp_pv_*).  Output sample t of a stream is sample t - latency of what StftRoundTrip.pitch_shift gives on
    everything the stream has received, bit for bit; the first `latency` samples are 0."""
    _prefix = "vp_pv"
    latency = property(lambda self: self.L.vp_pv_get_latency(self.h), doc="F - gcd(N, hop) samples.")

    def __init__(self, n_streams, block_size, hop=256, frame_len=1024, device=0):
        self._open(int(device), int(n_streams), int(block_size), int(frame_len), int(hop))
        self.S, self.N, self.hop, self.F, self.device = int(n_streams), int(block_size), int(hop), int(frame_len), device
        self._curve_tables = {}                                # device ratio tables, one per n_blocks, allocated at first use

    def set_semitones(self, v, stream=-1):
        """Interval in [-12, 12] for one stream or (-1) all; takes effect at the next process call."""
        self._chk(self.L.vp_pv_set_semitones(self.h, int(stream), float(v)))

    def semitones(self, stream):
        v = C.c_double()
        self._chk(self.L.vp_pv_get_semitones(self.h, int(stream), C.byref(v)))
        return v.value

    def process(self, x):
        """One block from host memory: float32 [S][N] -> [S][N] (synchronous)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.shape == (self.S, self.N), x.shape
        y = np.empty_like(x)
        self._chk(self.L.vp_pv_process_block(self.h, x.ctypes.data, y.ctypes.data))
        return y

    def _held_table(self, n_blocks, dev):
        """The device ratio table [n_blocks][S] of a curve call without one of its own: the intervals set_semitones holds, for every block."""
        held = np.array([self.semitones(s) for s in range(self.S)])
        return _upload_ratios(self._curve_tables, np.broadcast_to(held, (n_blocks, self.S)), dev)

    def process_device(self, d_in, d_out, n_blocks=1, stream=None, semitones_per_block=None, d_ratio=None, formant_semitones=None, lifter=FORMANT_LIFTER,
                       d_formant=None, locked=False, subbin=False):
        """n_blocks blocks on the device: torch float32 [n_blocks][S][N] (or [S][N] for one block), enqueued on `stream`
        (default: the current torch stream) without synchronising.
        semitones_per_block: array-like [n_blocks] or [n_blocks][S], |value| <= 12 -- this call's frames take the interval of the block in
        which their last sample arrives (vp_pv_process_blocks_curve_device); set_semitones' interval is neither used nor changed.  The
        table is uploaded on torch's current stream into a device table kept per n_blocks.  d_ratio instead: a device float64 tensor
        [n_blocks][S] of ratios, used as it is.
        formant_semitones (a scalar or [S], |value| <= 12; None: the calls above, unchanged) or d_formant (device float64 [S] of ratios):
        the call keeps the spectral envelope apart from the pitch (vp_pv_process_blocks_formant_device) -- 0 leaves the formants where
        they were; `lifter` is the cepstral lifter's length, 4 .. 64.  It is a curve call: without a table of its own it takes the
        intervals set_semitones holds, for every block.
        locked=True: the curve call with peak locking (vp_pv_process_blocks_locked_device); without a table of its own it takes the
        intervals set_semitones holds, like a formant call.  Not together with formant_semitones / d_formant: ValueError before any
        launch.  The kinds of call share the stream's state: after a change of kind the output is finite but carries a phase jump
        (reset() the stream at the change to avoid it).
        subbin=True (with locked=True only: ValueError otherwise, before any launch): the locked call with sub-bin region offsets
        (vp_pv_process_blocks_locked_subbin_device); it shares the locked call's state."""
        # (the asserts and the stream's default are written out here and in autotune_device: a helper's call would be most of what a
        # call of one small block costs the host)
        import torch
        if locked:
            _not_formant_on_locked(formant_semitones, d_formant)
        if subbin:
            _subbin_needs_locked(locked)
        n = int(n_blocks)
        shape = (self.S, self.N) if n == 1 and d_in.dim() == 2 else (n, self.S, self.N)
        assert d_in.is_cuda and d_in.dtype == torch.float32 and tuple(d_in.shape) == shape and d_in.is_contiguous()
        assert d_out.is_cuda and d_out.dtype == torch.float32 and tuple(d_out.shape) == shape and d_out.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream(d_in.device).cuda_stream
        io, st = (self.h, d_in.data_ptr(), d_out.data_ptr()), C.c_void_p(stream)
        if semitones_per_block is not None:
            assert d_ratio is None, "one of semitones_per_block and d_ratio"
            semi = np.asarray(semitones_per_block, dtype=np.float64)
            assert semi.shape in ((n,), (n, self.S)), semi.shape
            d_ratio = _upload_ratios(self._curve_tables, np.broadcast_to(semi.reshape(n, -1), (n, self.S)), d_in.device)
        formant = formant_semitones is not None or d_formant is not None
        if d_ratio is None:
            if not (formant or locked):
                return self._chk(self.L.vp_pv_process_blocks_device(*io, n, st))
            d_ratio = self._held_table(n, d_in.device)
        assert d_ratio.is_cuda and d_ratio.dtype == torch.float64 and tuple(d_ratio.shape) == (n, self.S) and d_ratio.is_contiguous()
        if locked:
            call = self.L.vp_pv_process_blocks_locked_subbin_device if subbin else self.L.vp_pv_process_blocks_locked_device
            self._chk(call(*io, d_ratio.data_ptr(), n, st))
        elif formant:
            d_formant = _device_formants(self, formant_semitones, d_formant, d_in.device)
            self._chk(self.L.vp_pv_process_blocks_formant_device(*io, d_ratio.data_ptr(), d_formant.data_ptr(), int(lifter), n, st))
        else:
            self._chk(self.L.vp_pv_process_blocks_curve_device(*io, d_ratio.data_ptr(), n, st))

    def autotune_device(self, tracker, d_in, d_out, n_blocks=1, keys=None, stream=None, formant_semitones=None, lifter=FORMANT_LIFTER, locked=False,
                        subbin=False):
        """Automatic pitch correction block by block (vp_pv_autotune_blocks_device): `tracker` (a StreamingPitchTracker of the same
        streams, block size and device) decides one ratio per block and stream from the audio received so far, this stream shifts along
        that table, both on `stream`; d_out has the bits of tracker.process_device followed by process_device(d_ratio=...).  Returns the
        tracker's (period, ratio), device tensors [n_blocks][S].  reset() does not reach the tracker: reset both.
        formant_semitones (a scalar or [S]; None: the call above, unchanged): the shift runs through the formant call instead
        (vp_pv_autotune_blocks_formant_device).
        locked=True: tracker.process_device followed by process_device(d_ratio=..., locked=True) on the same stream (not together with
        formant_semitones: ValueError before any launch).  subbin=True (with locked=True only): the locked call is
        process_device(d_ratio=..., locked=True, subbin=True)."""
        if locked:
            _not_formant_on_locked(formant_semitones)
        if subbin:
            _subbin_needs_locked(locked)
        if locked:
            period, ratio = tracker.process_device(d_in, n_blocks=n_blocks, keys=keys, stream=stream)
            self.process_device(d_in, d_out, n_blocks=n_blocks, stream=stream, d_ratio=ratio, locked=True, **({"subbin": True} if subbin else {}))
            return period, ratio
        import torch
        n = int(n_blocks)
        shape = (self.S, self.N) if n == 1 and d_in.dim() == 2 else (n, self.S, self.N)
        assert d_in.is_cuda and d_in.dtype == torch.float32 and tuple(d_in.shape) == shape and d_in.is_contiguous()
        assert d_out.is_cuda and d_out.dtype == torch.float32 and tuple(d_out.shape) == shape and d_out.is_contiguous()
        d_key, period, ratio = tracker._tables(keys, n, d_in.device)
        if stream is None:
            stream = torch.cuda.current_stream(d_in.device).cuda_stream
        head = (self.h, tracker.h, d_in.data_ptr(), d_out.data_ptr(), d_key.data_ptr() if d_key is not None else None, period.data_ptr(), ratio.data_ptr())
        if formant_semitones is not None:
            d_formant = _device_formants(self, formant_semitones, None, d_in.device)
            self._chk(self.L.vp_pv_autotune_blocks_formant_device(*head, d_formant.data_ptr(), int(lifter), n, C.c_void_p(stream)))
        else:
            self._chk(self.L.vp_pv_autotune_blocks_device(*head, n, C.c_void_p(stream)))
        return period, ratio

    def run(self, x, blocks_per_call=8, curve=None, autotune=None, keys=None, formant_semitones=None, lifter=FORMANT_LIFTER, locked=False, subbin=False):
        """Whole signals float [S][T] -> output aligned with the input, [S][T]: the input padded with `latency` zeros (and up to
        whole blocks), streamed through the device entry point `blocks_per_call` blocks at a time, the first `latency` samples
        dropped.  Continues from the handle's state (reset() first for a fresh start).
        curve: semitones per block, array-like [n] or [n][S] with n >= 1; block b takes row min(b, n - 1) (the padding keeps the last
        row), through process_device(semitones_per_block=...).
        autotune: a StreamingPitchTracker instead -- every call goes through autotune_device(autotune, ..., keys=keys), and the result is
        (output, period, ratio) with the tracker's tables as numpy arrays [n_blocks][S] (the padding blocks included).
        formant_semitones (a scalar or [S]; None: as above, unchanged): every call is a formant call (process_device / autotune_device).
        locked=True: every call is a peak-locked call (process_device / autotune_device with locked=True; not with formant_semitones).
        subbin=True (with locked=True only): every call also takes subbin=True."""
        assert curve is None or autotune is None, "one of curve and autotune"
        if locked:
            _not_formant_on_locked(formant_semitones)
        if subbin:
            _subbin_needs_locked(locked)
        lk = {"locked": True, **({"subbin": True} if subbin else {})} if locked else {}                     # (without the flag: exactly the calls made before it existed)
        import torch
        x = np.asarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[0] == self.S, x.shape
        T = x.shape[1]
        nb, lat = self._n_blocks(T)
        if curve is not None:
            curve = np.asarray(curve, dtype=np.float64)
            assert curve.ndim in (1, 2) and curve.shape[0] >= 1 and (curve.ndim == 1 or curve.shape[1] == self.S), curve.shape
            curve = curve[np.minimum(np.arange(nb), curve.shape[0] - 1)]
        d_in = self._slab(x, nb)
        d_out = torch.empty_like(d_in)
        b, tables = 0, []
        while b < nb:
            k = min(int(blocks_per_call), nb - b)
            if autotune is not None:
                tables.append(self.autotune_device(autotune, d_in[b:b + k], d_out[b:b + k], n_blocks=k, keys=keys, formant_semitones=formant_semitones,
                                                   lifter=lifter, **lk))
            elif curve is None:
                self.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k, formant_semitones=formant_semitones, lifter=lifter, **lk)
            else:
                self.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k, semitones_per_block=curve[b:b + k], formant_semitones=formant_semitones,
                                    lifter=lifter, **lk)
            b += k
        y = self._trimmed(d_out, T, lat)
        if autotune is not None:
            return y, torch.cat([p for p, _ in tables]).cpu().numpy(), torch.cat([r for _, r in tables]).cpu().numpy()
        return y


class CrossSynthStream(_BlockStream):
    """Streaming STFT cross-synthesis: `n_streams` independent pairs of voice and carrier, blocks of `block_size` samples, state kept
    across calls (include/vp_amd.h vp_xs_*).  Output sample t of a stream is sample t - latency of what StftRoundTrip.cross_synth gives
    on everything the stream has received, bit for bit; the first `latency` samples are 0."""
    _prefix = "vp_xs"
    latency = property(lambda self: self.L.vp_xs_get_latency(self.h), doc="F - gcd(N, hop) samples.")

    def __init__(self, n_streams, block_size, hop=256, frame_len=1024, device=0):
        self._open(int(device), int(n_streams), int(block_size), int(frame_len), int(hop))
        self.S, self.N, self.hop, self.F, self.device = int(n_streams), int(block_size), int(hop), int(frame_len), device

    def process_device(self, d_voice, d_carrier, d_out, n_blocks=1, depth=1.0, lifter=FORMANT_LIFTER, stream=None, d_depth=None):
        """n_blocks blocks on the device: torch float32 [n_blocks][S][N] each (or [S][N] for one block), enqueued on `stream` (default: the
        current torch stream) without synchronising.  depth, d_depth, lifter: as StftRoundTrip.cross_synth's, for the frames this call
        completes.  Wrong dtypes, shapes or lifter raise ValueError before any launch."""
        n = int(n_blocks)
        if n < 1:
            raise ValueError("cross_synth: at least one block expected")
        shape = (self.S, self.N) if n == 1 and d_voice.dim() == 2 else (n, self.S, self.N)
        _cross_check(d_voice, d_carrier, d_out, shape, lifter)
        d_depth = _device_depths(self, depth, d_depth, d_voice.device)
        self._chk(self.L.vp_xs_process_blocks_device(self.h, d_voice.data_ptr(), d_carrier.data_ptr(), d_out.data_ptr(), _ptr(d_depth), int(lifter), n,
                                                     _stream_of(stream, d_voice)))

    def run(self, voice, carrier, blocks_per_call=8, depth=1.0, lifter=FORMANT_LIFTER):
        """Whole signals float [S][T] each -> output aligned with the inputs, [S][T]: the inputs padded with `latency` zeros (and up to
        whole blocks), streamed through process_device `blocks_per_call` blocks at a time, the first `latency` samples dropped.  Continues
        from the handle's state (reset() first for a fresh start)."""
        import torch
        v, c = np.asarray(voice, dtype=np.float32), np.asarray(carrier, dtype=np.float32)
        if v.ndim != 2 or v.shape[0] != self.S or v.shape != c.shape:
            raise ValueError(f"cross_synth: voice {v.shape} and carrier {c.shape}: two arrays [{self.S}][T] expected")
        if not 4 <= int(lifter) <= 64:
            raise ValueError("cross_synth: lifter: 4 to 64 samples expected")
        T = v.shape[1]
        nb, lat = self._n_blocks(T)
        d_v, d_c = self._slab(v, nb), self._slab(c, nb)
        d_out = torch.empty_like(d_v)
        for b in range(0, nb, int(blocks_per_call)):
            k = min(int(blocks_per_call), nb - b)
            self.process_device(d_v[b:b + k], d_c[b:b + k], d_out[b:b + k], n_blocks=k, depth=depth, lifter=lifter)
        return self._trimmed(d_out, T, lat)


class HarmonizerStream(_BlockStream):
    """Streaming harmonizer: `n_streams` independent streams of `n_voices` peak-locked voices each beside the dry signal, blocks of
    `block_size` samples, state kept across calls (include/vp_amd.h vp_hz_*).  Output sample t of a stream is sample t - latency of what
    StftRoundTrip.harmonize gives on everything the stream has received, bit for bit -- the dry part delayed with the voices --; the
    first `latency` samples are 0."""
    _prefix = "vp_hz"
    latency = property(lambda self: self.L.vp_hz_get_latency(self.h), doc="F - gcd(N, hop) samples.")

    def __init__(self, n_streams, block_size, n_voices, hop=256, frame_len=1024, device=0):
        self._open(int(device), int(n_streams), int(block_size), int(frame_len), int(hop), int(n_voices))
        self.S, self.N, self.V, self.hop, self.F, self.device = int(n_streams), int(block_size), int(n_voices), int(hop), int(frame_len), device
        self._tables = {}

    def process_device(self, d_in, d_out, n_blocks=1, semitones=None, d_ratio=None, gains=None, dry=None, stream=None):
        """n_blocks blocks on the device: torch float32 [n_blocks][S][N] each (or [S][N] for one block), enqueued on `stream` (default: the
        current torch stream) without synchronising.  `semitones`: [V] fixed intervals, [S][V], or [n_blocks][S][V] (a frame takes the
        block its last sample arrives in); d_ratio instead: a device float64 tensor [n_blocks][S][V].  gains, dry: as
        StftRoundTrip.harmonize's, for the frames this call completes.  Wrong dtypes or shapes raise ValueError before any launch."""
        torch = _T or _torch()
        n = int(n_blocks)
        if n < 1:
            raise ValueError("harmonize: at least one block expected")
        _harm_io(d_in, d_out, (self.S, self.N) if n == 1 and d_in.dim() == 2 else (n, self.S, self.N))
        if (semitones is None) == (d_ratio is None):
            raise ValueError("harmonize: one of semitones and d_ratio expected")
        if d_ratio is None:
            st = np.asarray(semitones, dtype=np.float64)
            if st.shape not in ((self.V,), (self.S, self.V), (n, self.S, self.V)):
                raise ValueError(f"harmonize: semitones: [{self.V}], [{self.S}][{self.V}] or [{n}][{self.S}][{self.V}] expected, got {st.shape}")
            d_ratio = _upload_ratios(self._tables, np.broadcast_to(st, (n, self.S, self.V)), d_in.device)
        elif not _is(d_ratio, torch.float64, (n, self.S, self.V)):
            raise ValueError(f"harmonize: d_ratio: a contiguous float64 tensor [{n}][{self.S}][{self.V}] on the GPU expected")
        d_gain, d_dry = _harm_levels(self, self.V, gains, dry, d_in.device)
        self._chk(self.L.vp_hz_process_blocks_device(self.h, d_in.data_ptr(), d_out.data_ptr(), d_ratio.data_ptr(), _ptr(d_gain), _ptr(d_dry), n,
                                                     _stream_of(stream, d_in)))

    def autoharm_device(self, tracker, d_in, d_out, degrees, n_blocks=1, keys=None, unvoiced=None, gains=None, dry=None, stream=None):
        """Key-aware harmony on the device (vp_hz_autoharm_blocks_device): tracker.process_voices_device with this handle's voice count, then
        process_device along its table, on one stream; the output has the bits of those two calls.  `tracker`: a StreamingPitchTracker
        of the same S, N and device.  degrees, keys, unvoiced as StreamingPitchTracker.process_voices_device's; gains, dry as
        process_device's.  Returns the tracker's (period, ratio).  Resets stay separate.  ValueError before any launch."""
        torch = _T or _torch()
        n = int(n_blocks)
        if n < 1:
            raise ValueError("harmonize: at least one block expected")
        _harm_io(d_in, d_out, (self.S, self.N) if n == 1 and d_in.dim() == 2 else (n, self.S, self.N))
        if (tracker.S, tracker.N) != (self.S, self.N):
            raise ValueError(f"harmonize: the tracker has {tracker.S} streams of {tracker.N}-sample blocks, the harmonizer {self.S} of {self.N}")
        d_degree, d_unv, _ = _voice_tables(tracker, degrees, keys, unvoiced, d_in.device, V=self.V)
        d_gain, d_dry = _harm_levels(self, self.V, gains, dry, d_in.device)
        d_key = _device_keys(tracker, keys, d_in.device)
        period = torch.empty((n, self.S), dtype=torch.int32, device=d_in.device)
        ratio = torch.empty((n, self.S, self.V), dtype=torch.float64, device=d_in.device)
        self._chk(self.L.vp_hz_autoharm_blocks_device(self.h, tracker.h, d_in.data_ptr(), d_out.data_ptr(), _ptr(d_key), d_degree.data_ptr(), _ptr(d_unv),
                                                      _ptr(d_gain), _ptr(d_dry), period.data_ptr(), ratio.data_ptr(), n, _stream_of(stream, d_in)))
        return period, ratio

    def run(self, x, semitones=None, blocks_per_call=8, gains=None, dry=None, degrees=None, autoharm=None, keys=None, unvoiced=None):
        """Whole signals float [S][T] -> output aligned with the input, [S][T]: the input padded with `latency` zeros (and up to whole
        blocks), streamed through process_device `blocks_per_call` blocks at a time, the first `latency` samples dropped.  `semitones`:
        [V], [S][V] or [n_blocks_total][S][V] with n_blocks_total = ceil((T + latency) / N).  degrees=..., autoharm=tracker [, keys=...,
        unvoiced=...] instead of semitones: the blocks go through autoharm_device, and the result is (output, period [n_blocks_total][S],
        ratio [n_blocks_total][S][V]).  Continues from the handle's state (reset() first for a fresh start)."""
        import torch
        x = np.asarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] != self.S:
            raise ValueError(f"harmonize: input {x.shape}: an array [{self.S}][T] expected")
        if (semitones is None) == (degrees is None):
            raise ValueError("harmonize: one of semitones and degrees expected")
        if (degrees is None) != (autoharm is None):
            raise ValueError("harmonize: degrees and autoharm=tracker go together")
        T = x.shape[1]
        nb, lat = self._n_blocks(T)
        if degrees is not None:
            d_x = self._slab(x, nb)
            d_out = torch.empty_like(d_x)
            ps, rs = [], []
            for b in range(0, nb, int(blocks_per_call)):
                k = min(int(blocks_per_call), nb - b)
                p, r = self.autoharm_device(autoharm, d_x[b:b + k], d_out[b:b + k], degrees, n_blocks=k, keys=keys, unvoiced=unvoiced, gains=gains, dry=dry)
                ps.append(p)
                rs.append(r)
            y = self._trimmed(d_out, T, lat)
            return y, torch.cat(ps).cpu().numpy(), torch.cat(rs).cpu().numpy()
        st = np.asarray(semitones, dtype=np.float64)
        if st.shape not in ((self.V,), (self.S, self.V), (nb, self.S, self.V)):
            raise ValueError(f"harmonize: semitones: [{self.V}], [{self.S}][{self.V}] or [{nb}][{self.S}][{self.V}] expected, got {st.shape}")
        st = np.broadcast_to(st, (nb, self.S, self.V))
        d_x = self._slab(x, nb)
        d_out = torch.empty_like(d_x)
        for b in range(0, nb, int(blocks_per_call)):
            k = min(int(blocks_per_call), nb - b)
            self.process_device(d_x[b:b + k], d_out[b:b + k], n_blocks=k, semitones=st[b:b + k], gains=gains, dry=dry)
        return self._trimmed(d_out, T, lat)


class StreamingPitchTracker(_StreamHandle):
    """Streaming pitch tracker (include/vp_amd.h vp_pv_tracker_*): StftRoundTrip.track_pitch's decision once per block and stream, from the
    last frame_len + ceil(sample_rate / 100) samples the stream has received (period 0, ratio 1.0 until it has that many), then followed:
    the last voiced ratio is held for `hold_blocks` unvoiced blocks before the target returns to 1.0, and the ratio moves the fraction
    `glide` of the way to its target per block (1.0: at once).  frame_len (1024 or 2048) is the tracker's own analysis length.  The ratio
    table is what PhaseVocoderStream.process_device(d_ratio=...) takes; PhaseVocoderStream.autotune_device runs both."""

    _prefix = "vp_pv_tracker"

    def __init__(self, n_streams, block_size, sample_rate, frame_len=1024, hold_blocks=0, glide=1.0, device=0):
        self._open(int(device), int(n_streams), int(block_size), int(frame_len), float(sample_rate))
        self.S, self.N, self.F, self.fs, self.device = int(n_streams), int(block_size), int(frame_len), float(sample_rate), device
        if hold_blocks != 0 or glide != 1.0:
            self.set_follow(hold_blocks, glide)

    def set_follow(self, hold_blocks, glide):
        """0 <= hold_blocks <= 2^20 unvoiced blocks the last voiced ratio outlives, 0 < glide <= 1; every stream, from the next call on."""
        self._chk(self.L.vp_pv_tracker_set_follow(self.h, int(hold_blocks), float(glide)))

    def set_fine(self, fine):
        """fine=True: every process call of this tracker (mono, voices, and the composed autotune / autoharm calls) uses the fine raw
        decision (vp_pv_tracker_set_mode, VP_TRACK_FINE) from the next call on; no stream state is touched.  False: the integer one."""
        self._chk(self.L.vp_pv_tracker_set_mode(self.h, TRACK_FINE if fine else TRACK_INTEGER))

    @property
    def fine(self):
        return self.L.vp_pv_tracker_get_mode(self.h) == TRACK_FINE

    def _tables(self, keys, n_blocks, dev):
        """(d_key or None, period, ratio) of a call of n_blocks blocks: the key table is kept per handle (one device int32 [S], rewritten
        on torch's current stream when `keys` is host data); the outputs are new tensors, the caller's to keep."""
        import torch
        d_key = _device_keys(self, keys, dev)
        return d_key, torch.empty((n_blocks, self.S), dtype=torch.int32, device=dev), torch.empty((n_blocks, self.S), dtype=torch.float64, device=dev)

    def process_device(self, d_in, n_blocks=1, keys=None, stream=None, with_fine_period=False):
        """n_blocks blocks on the device: torch float32 [n_blocks][S][N] (or [S][N] for one block), the slab PhaseVocoderStream takes,
        enqueued on `stream` (default: the current torch stream) without synchronising.  keys as StftRoundTrip.track_pitch's.  Returns
        (period, ratio), device tensors int32 / float64 [n_blocks][S]: the period in samples (0 = unvoiced) and the followed ratio.
        with_fine_period=True: the fine tracker whatever the mode (vp_pv_tracker_process_blocks_fine_device); returns (period, ratio,
        period_fine), the third the raw decision's refined period, float64 [n_blocks][S] (0.0 unvoiced or while the ring fills)."""
        import torch
        shape = (self.S, self.N) if n_blocks == 1 and d_in.dim() == 2 else (int(n_blocks), self.S, self.N)
        assert d_in.is_cuda and d_in.dtype == torch.float32 and tuple(d_in.shape) == shape and d_in.is_contiguous()
        d_key, period, ratio = self._tables(keys, int(n_blocks), d_in.device)
        if stream is None:
            stream = torch.cuda.current_stream(d_in.device).cuda_stream
        if with_fine_period:
            fine = torch.empty((int(n_blocks), self.S), dtype=torch.float64, device=d_in.device)
            self._chk(self.L.vp_pv_tracker_process_blocks_fine_device(self.h, d_in.data_ptr(), _ptr(d_key), period.data_ptr(), fine.data_ptr(),
                                                                      ratio.data_ptr(), int(n_blocks), C.c_void_p(stream)))
            return period, ratio, fine
        self._chk(self.L.vp_pv_tracker_process_blocks_device(self.h, d_in.data_ptr(), d_key.data_ptr() if d_key is not None else None,
                                                             period.data_ptr(), ratio.data_ptr(), int(n_blocks), C.c_void_p(stream)))
        return period, ratio

    def process_voices_device(self, d_in, degrees, n_blocks=1, keys=None, unvoiced=None, stream=None):
        """Key-aware voices (vp_pv_tracker_process_blocks_voices_device): process_device's decision, then per voice the ratio `degrees[v]`
        steps of the key's table from the note chosen, followed per voice (hold, glide: set_follow's; after the hold the target is
        `unvoiced`).  degrees, keys, unvoiced as StftRoundTrip.track_harmony's.  Returns (period, ratio), device tensors int32 [n_blocks][S] /
        float64 [n_blocks][S][V] -- the table HarmonizerStream.process_device(d_ratio=...) takes.  A block goes through this call or
        process_device, not both; each keeps its own follow state.  ValueError before any launch."""
        torch = _T or _torch()
        n = int(n_blocks)
        if n < 1:
            raise ValueError("process_voices_device: at least one block expected")
        shape = (self.S, self.N) if n == 1 and d_in.dim() == 2 else (n, self.S, self.N)
        if not _is(d_in, torch.float32, shape):
            raise ValueError(f"process_voices_device: input: a contiguous float32 tensor {list(shape)} on the GPU expected")
        d_degree, d_unv, V = _voice_tables(self, degrees, keys, unvoiced, d_in.device)
        d_key = _device_keys(self, keys, d_in.device)
        period = torch.empty((n, self.S), dtype=torch.int32, device=d_in.device)
        ratio = torch.empty((n, self.S, V), dtype=torch.float64, device=d_in.device)
        self._chk(self.L.vp_pv_tracker_process_blocks_voices_device(self.h, d_in.data_ptr(), _ptr(d_key), V, d_degree.data_ptr(), _ptr(d_unv),
                                                                    period.data_ptr(), ratio.data_ptr(), n, _stream_of(stream, d_in)))
        return period, ratio
