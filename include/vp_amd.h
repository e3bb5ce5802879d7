/*
 * vp_amd.h -- C ABI of libvp_amd.so: the MI355X (gfx950) batch implementation of the
 * DamRsn/VocoderProject DSP hot path (PitchProcess pitch corrector + LPC/VocoderProcess
 * cross-synthesis behind VocoderAudioProcessor::processBlock()).
 *
 * One handle = a BATCH of S independent plugin instances (one per audio stream) living on one
 * GPU.  Every entry point is what the reference's host code would bind through FFI for this
 * path; the reference interface each one replaces is cited as file:line relative to
 * /root/reference/Source/.  Plain pointers and sizes only; no C++/torch types.
 *
 * Threading: one caller thread per handle (the reference runs processBlock() on one audio
 * thread per instance, PluginProcessor.cpp:203).  Parameters are snapshotted at call entry
 * (the reference reads std::atomic<float> values with load(), :214-230).
 * No allocation happens in any vp_process_*() call (reference: all vectors are sized in
 * prepareToPlay, PitchProcess.cpp:95-121): vp_prepare_*() and vp_reserve_blocks() are the only
 * entry points that allocate device memory (vp_debug_alloc_count() counts the allocations).
 */
#ifndef VP_AMD_H
#define VP_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VP_ABI_VERSION 3        /* 3 (round 6): + VP_ERR_TIMEOUT, vp_debug_set_spin_limit (additions only: a version-2 caller keeps working); 2 (round 5): + vp_set_wave_specialised, vp_debug_read_ws_stamps; round 4 had added vp_reserve_blocks and the
                                   vp_stft_* precision / pitch-shift entries and narrowed vp_stft_create to 1024- and 2048-point frames */

/* status codes (the reference has none: it prints to std::cerr and assert(false)s) */
enum {
    VP_OK = 0,
    VP_ERR_INVALID_ARG = -1,     /* null pointer, non-positive size, parameter out of its range (PluginProcessor.cpp:41-69) */
    VP_ERR_NOT_PREPARED = -2,    /* processBlock before prepareToPlay */
    VP_ERR_INVALID_OVERLAP = -3, /* VocoderProcess.cpp:110-114 "Invalid overlap": (wlen-hop)/wlen must be 0.5 or 0.75 */
    VP_ERR_GEOMETRY = -4,        /* frameLen % (frameLen-hop) != 0 (PitchProcess.cpp:91-92), tauMax > samplesToKeep (:364), ... */
    VP_ERR_ORDER = -5,           /* LPC order above its parameter maximum (VocoderProcess.cpp:145-148,161-164) */
    VP_ERR_NO_DEVICE = -6,       /* no usable HIP device: this library has NO CPU fallback */
    VP_ERR_HIP = -7,             /* a HIP runtime call failed; see vp_last_error() */
    VP_ERR_OOM = -8,
    VP_ERR_TIMEOUT = -9          /* a kernel's bounded inter-wavefront wait ran out (a lost signal, or a wavefront held up for about a second
                                    by a debugger / preemption): that launch's output and the handle's device state are INVALID.  The handle
                                    is poisoned -- every later process call returns this code -- until it is prepared again.  Reported by the
                                    call that synchronises behind the launch (vp_process_block*, vp_process_blocks with host pointers,
                                    vp_synchronize) or, on the device-pointer entry points, by the next call on the handle; the reference's
                                    counterpart is the assert(false) on impossible state, PitchProcess.cpp:824,828 */
};

/* The ten plugin parameters, same ids, ranges and defaults as
 * VocoderAudioProcessor::createParameterLayout() (PluginProcessor.cpp:37-73).
 * vp_set_params() gives every stream of the handle this set; vp_set_stream_params() gives ONE stream its own (each stream
 * of a batch is a plugin instance with its own treeState), all ten parameters except lpcPitch. */
typedef struct vp_params {
    float gainPitch;   /* dB  [-60, 6]   default   0 */
    float gainVoice;   /* dB  [-60, 6]   default -60 (dry voice off) */
    float gainSynth;   /* dB  [-60, 6]   default -60 (dry carrier off) */
    float gainVoc;     /* dB  [-60, 6]   default   0 */
    int lpcVoice;      /* [2, 100] default 40; re-read every vocoder window (VocoderProcess.cpp:193-194) */
    int lpcPitch;      /* [2, 100] default 15; read ONLY at prepare (PitchProcess.cpp:70) */
    int lpcSynth;      /* [2, 30]  default  5 */
    int keyPitch;      /* 0..11 = major key on A, A#, ... G#; 12 = chromatic (default) (Notes.h:18) */
    int pitchBool;     /* 1: pitch corrector on (default) */
    int vocBool;       /* 1: vocoder on (default) */
} vp_params;

/* Per-stream pitch-tracker state, for tracing/parity tests (the reference keeps these as private
 * members, PitchProcess.h:108-131). */
#define VP_MARK_CAP 64
typedef struct vp_pitch_state {
    int period, prevPeriod, prevVoicedPeriod, periodNew;
    int nAn, nSt, stMarkIdx, gateOpen;
    double pitch, prevPitch, beta, closestFreq;
    int anMarks[VP_MARK_CAP];
    int stMarks[VP_MARK_CAP];
    double a[101];
} vp_pitch_state;

typedef struct vp_handle vp_handle;

/* createPluginFilter() (PluginProcessor.cpp:272-275): a batch of plugin instances on HIP device
 * `device`.  Fails with VP_ERR_NO_DEVICE when no GPU is present. */
int vp_create(int device, vp_handle **out);
int vp_destroy(vp_handle *h);

/* treeState.getRawParameterValue(id)->store(v) for all ten ids at once (PluginProcessor.cpp:37-73).
 * May be called between blocks at any time; lpcPitch only takes effect at the next prepare. */
int vp_set_params(vp_handle *h, const vp_params *p);
int vp_get_params(const vp_handle *h, vp_params *p);
/* One parameter set PER STREAM (each stream of a batch is its own plugin instance with its own treeState).
 * After prepare; takes effect at the next block.  Everything is per stream, pitchBool and vocBool included: a process that
 * is switched off does not advance its startSample / nChunk (PluginProcessor.cpp:214-221), so the library keeps streams
 * whose switches differ(ed) as separate cohorts and launches each with a stream-index map.  Only lpcPitch stays per handle
 * (it is read at prepare and selects the pitch kernel's build): `p` must repeat the handle's value for it
 * (VP_ERR_INVALID_ARG otherwise).  A later vp_set_params() puts every stream back on one common set; so does a new prepare. */
int vp_set_stream_params(vp_handle *h, int stream, const vp_params *p);
int vp_get_stream_params(const vp_handle *h, int stream, vp_params *p);
void vp_default_params(vp_params *p);

/* EXTENSION (no reference counterpart; BASELINE configs[1] "+-12-semitone pitch shift"): a fixed interval instead of
 * the correction to the key's nearest note.  placeStMarks (PitchProcess.cpp:593-598) then takes
 * beta = 2^(semitones/12) (host libm) in place of closestFreq/pitch; everything else on the path is unchanged.
 * stream = -1 sets every stream.  After prepare; takes effect at the next analysed frame; a new prepare switches it
 * off.  |semitones| <= 12 (VP_ERR_INVALID_ARG); VP_ERR_GEOMETRY when an upward shift would need more synthesis marks
 * per frame than VP_MARK_CAP (F / round(floor(fs/fMax) / beta) + 2). */
int vp_set_pitch_shift(vp_handle *h, int stream, int on, double semitones);
int vp_get_pitch_shift(const vp_handle *h, int stream, int *on, double *semitones);

/* VocoderAudioProcessor::prepareToPlay(sampleRate, samplesPerBlock) (PluginProcessor.cpp:144-184)
 * for n_streams instances: derives the vocoder/pitch geometry from the sample rate (:159-170),
 * allocates and zeroes all per-stream state in HBM. */
int vp_prepare_to_play(vp_handle *h, double sample_rate, int samples_per_block, int n_streams);

/* Same with explicit geometry: pitchProcess.prepare(fs,100,800,F,H,N,-60),
 * vocoderProcess.prepare(W,h,"sine",-60), myBuffer.prepare(N,F,max(F,W),fs,1,2,2)
 * (PluginProcessor.cpp:172-181; both prepare()s are public: PitchProcess.h:40, VocoderProcess.h:29). */
int vp_prepare_explicit(vp_handle *h, double sample_rate, int samples_per_block, int n_streams,
                        int frame_len_pitch, int hop_pitch, int wlen_voc, int hop_voc);

/* processBlock(AudioBuffer<float>&, MidiBuffer&) (PluginProcessor.cpp:203-234) for every stream.
 * Host buffers, planar float32:  in  [n_streams][3][N]  (ch0 voice, ch1/ch2 side-chain L/R),
 *                                out [n_streams][2][N]  (L, R).
 * Synchronous: returns when `out` is filled. */
int vp_process_block(vp_handle *h, const float *in, float *out);

/* The reference's exact in-place form: io [n_streams][3][N]; on return ch0/ch1 hold out L/R and
 * ch2 is zero (MyBuffer.cpp:115 buffer.clear()). Host buffer, synchronous. */
int vp_process_block_inplace(vp_handle *h, float *io);

/* Device-resident form (the multi-GPU / throughput path): d_in, d_out are device pointers with
 * the layouts above; kernels are enqueued on `hip_stream` (a hipStream_t, may be NULL = default
 * stream) and the call returns without synchronising. */
int vp_process_block_device(vp_handle *h, const float *d_in, float *d_out, void *hip_stream);
/* processBlock() on buffers without the side-chain bus (mono voice in, stereo out): voice float [n_streams][N].
 * MyBuffer::fillInputBuffers takes null side-chain pointers and fills the synth ring with zeros (MyBuffer.cpp:93-102);
 * results are identical to vp_process_block with zeroed ch1/ch2, at a third of the input traffic.  May be mixed freely
 * with the three-channel calls. */
int vp_process_block_mono(vp_handle *h, const float *voice, float *out);
int vp_process_block_mono_device(vp_handle *h, const float *d_voice, float *d_out, void *hip_stream);
/* n_blocks of them at once: d_voice float [n_blocks][n_streams][N] (the mono form of vp_process_blocks_device below) */
int vp_process_blocks_mono_device(vp_handle *h, const float *d_voice, float *d_out, int n_blocks, void *hip_stream);
/* n_blocks consecutive processBlock() calls at once (offline rendering, servers with audio queued up):
 * d_in float [n_blocks][n_streams][3][N], d_out float [n_blocks][n_streams][2][N], i.e. block b's slabs are what
 * vp_process_block_device would take.  Parameters are read once, at entry.  What runs:
 *  - pitch corrector alone: the blocks run in ONE launch (tracker state and the frame in flight stay on chip between them);
 *    results identical to n_blocks single calls;
 *  - vocoder alone (LPC orders <= 48): groups of up to 16 blocks as ONE launch of the lane-per-window pipeline -- the window grid
 *    carries across blocks, so B blocks are B times the windows, i.e. B times the lanes; every block keeps its own ring ingest,
 *    silence gate and output slab.  In VP_IIR_EXACT always (the pipeline and the workgroup kernel give the same bits: results
 *    identical to single calls; 256 streams, 8 blocks per call: 3x the single-call throughput); in VP_IIR_FAST only where
 *    single-block calls take the pipeline too (VP_VOC_AUTO above 256 streams, or VP_VOC_BATCHED) -- the two implementations'
 *    tolerance-mode roundings differ, and the output must not depend on how the caller groups blocks;
 *  - both enabled, VP_IIR_FAST, and single-block calls on the pipeline (same condition): groups of up to 16 blocks as one launch of
 *    the serial pitch kernel followed by one launch of the pipeline (the pitch kernel ingests the blocks and adds its chunks into a
 *    linear accumulator of the call, the pipeline works from a snapshot of the rings and folds that accumulator in when it emits):
 *    every decision and every filter output is the block-by-block path's; the audio equals it to the rounding of the additions
 *    into the output accumulator, which happen chunks-first instead of windows-first (<= 2e-6 of full scale, tested);
 *  - anything else (VP_IIR_EXACT with both enabled, per-stream switches that split the batch, ...): block by block.
 * The two pipeline plans are only taken where they pay (round 6, measured): a batch whose single block already fills the chip
 * (8192 windows and more per block: e.g. 1024 streams at 512 / 128) runs the vocoder-only plan never and the combined plan from
 * groups of eight blocks on -- as does a batch whose single-block calls overlap the pitch kernel with the pipeline's tail
 * (vp_set_overlap) --; smaller batches take both from two blocks on.  Same results either way (the plans' arithmetic is the
 * single-block pipeline's).
 * The two pipeline plans need scratch for the call's windows: vp_reserve_blocks(h, n) sizes it for calls of up to n blocks; a
 * larger call is carried out in groups of n, and without a reservation these plans fall back to block by block.  Nothing is
 * allocated here. */
int vp_process_blocks_device(vp_handle *h, const float *d_in, float *d_out, int n_blocks, void *hip_stream);
/* The same from HOST memory: in float [n_blocks][n_streams][3][N], out float [n_blocks][n_streams][2][N]; upload, the blocks,
 * download, in groups of as many blocks as vp_reserve_blocks sized the staging buffers for (none reserved: block by block through
 * the single-block staging buffers of prepare); synchronises before returning. */
int vp_process_blocks(vp_handle *h, const float *in, float *out, int n_blocks);
/* Channel-pointer forms: processBlock() on what AudioBuffer<float> holds, one pointer per channel (getReadPointer / getWritePointer,
 * MyBuffer.cpp:74-105), the channels of a stream neither contiguous nor all present.
 *   in:  n_streams * n_in  pointers; row (s, ch) = in[s * n_in + ch], N floats each.   n_in  = 1 (voice only) or 3.
 *   out: n_streams * n_out pointers; row (s, ch) = out[s * n_out + ch], N floats each. n_out = 2 (L, R) or 3.
 *  - A null input pointer reads as silence (MyBuffer.cpp:93-102, here for every channel and per stream); a null output pointer means
 *    that channel is not wanted.  With n_out = 3, channel 2 (where not null) receives zeros (MyBuffer.cpp:115 buffer.clear()).
 *  - Output rows may alias input rows (JUCE's in-place buffer): every input row is consumed before any output row is written.  Output
 *    rows must not overlap each other (not checked).  Rows need float alignment only.
 *  - Host form (vp_process_block_channels): table and rows in host memory, synchronous like vp_process_block.  n_in = 1, or n_in = 3 with
 *    every side-chain pointer null, takes the mono path (vp_process_block_mono).
 *  - Device forms: the tables are DEVICE arrays of device pointers (the convention of batched BLAS), the rows device memory; the work is
 *    enqueued on hip_stream without synchronising, like vp_process_block_device.  Build the tables once and reuse them.  n_in = 1 takes
 *    the mono path; null side-chain entries in an n_in = 3 table are zero-filled on the three-channel path (same results).
 *  - vp_process_blocks_channels_device: every row holds n_blocks * N contiguous samples -- a stream's recording as it lies in memory.
 *    The result is what vp_process_blocks_device gives on the equivalent [n_blocks][n_streams][3][N] slab, its grouping of the blocks
 *    under vp_reserve_blocks included.  A call within the reservation costs one pack and one unpack kernel around that plan; a larger
 *    one is carried out in groups of the reserved size (whole multiples of 16 blocks above 16; the consumed-before-written rule then
 *    holds per group), and without a reservation block by block through the single-block staging.
 * The results are bit-identical to the packed entry points on the packed data: the same plans run on the same values.  No allocation in
 * any of the three (the packed staging is sized in prepare and in vp_reserve_blocks).  VP_ERR_INVALID_ARG (null handle or table, n_in
 * not 1 or 3, n_out not 2 or 3, n_blocks < 1) and VP_ERR_NOT_PREPARED are reported before the device is touched. */
int vp_process_block_channels(vp_handle *h, const float *const *in, int n_in, float *const *out, int n_out);
int vp_process_block_channels_device(vp_handle *h, const float *const *d_in, int n_in, float *const *d_out, int n_out, void *hip_stream);
int vp_process_blocks_channels_device(vp_handle *h, const float *const *d_in, int n_in, float *const *d_out, int n_out, int n_blocks, void *hip_stream);
/* Allocation for the multi-block entry points, outside the process calls: scratch of the lane-per-window pipeline for the windows of
 * min(n_blocks, 16) blocks, the combined plan's ring snapshots / per-block gates / linear accumulator, and host staging for
 * n_blocks blocks.  After prepare (a new prepare drops the reservation); grows only; synchronises the device.  VP_ERR_OOM.
 * (The reference sizes everything in prepareToPlay, PitchProcess.cpp:95-121; how many blocks a caller queues per call is not a
 * prepareToPlay argument, hence the separate entry point.) */
int vp_reserve_blocks(vp_handle *h, int n_blocks);
int vp_get_reserved_blocks(const vp_handle *h);
/* Device allocations (hipMalloc calls) made for this handle since vp_create: constant across any sequence of vp_process_*() calls. */
long vp_debug_alloc_count(const vp_handle *h);

/* Arithmetic of the two all-pole synthesis filters (VocoderProcess.cpp:277-286, PitchProcess.cpp:307-322).
 * VP_IIR_EXACT (default): the reference's summation order, output bit-identical to the CPU restatement.
 * VP_IIR_FAST: transposed-form recursion with the taps spread over the lanes; differs from EXACT by
 * rounding only (measured max |diff| ~1e-12 of full scale before the float32 cast); every decision of
 * the algorithm (pitch, marks, gate) is still bit-identical because none depends on a filter output. */
#define VP_IIR_EXACT 0
#define VP_IIR_FAST 1
int vp_set_iir_mode(vp_handle *h, int mode);
int vp_get_iir_mode(const vp_handle *h);

/* Which implementation of the vocoder (VocoderProcess::process) a block runs.  Same results (bit-identical in
 * VP_IIR_EXACT mode), different mapping onto the GPU:
 * VP_VOC_WORKGROUP: one workgroup per stream, one wavefront per window (vp_k_vocoder / vp_k_vocoder_lite);
 * VP_VOC_BATCHED: a pipeline of small kernels in which one LANE owns one window (vp_voc2.hip) -- pays when a block of the
 *   batch has thousands of windows; LPC orders up to 48, at most 64 windows per stream and block, else the call falls back;
 * VP_VOC_AUTO (default): batched for batches of more than 256 streams (one workgroup per CU no longer holds them) with at
 *   least 1024 windows per block. */
#define VP_VOC_AUTO 0
#define VP_VOC_WORKGROUP 1
#define VP_VOC_BATCHED 2
int vp_set_vocoder_path(vp_handle *h, int path);
int vp_get_vocoder_path(const vp_handle *h);

/* VP_IIR_FAST only, both processes on, batched vocoder: run the pitch corrector BESIDE the tail of the vocoder pipeline (its all-pole
 * recursion and overlap-add: register-light kernels that fit into what the pitch kernel leaves of a SIMD's register file; second
 * HIP stream, accumulator of its own, merged at emit) instead of behind it.  0 off, 1 on, VP_OVERLAP_AUTO (the default): on where it
 * pays -- the full-register pitch builds (frames too large for two workgroups per CU: 419 -> 376 us per block at the configs[4]
 * geometry), off for the register-light ones (1024 streams of the plugin's geometry: 276 against 274 us).  What is given up is the
 * order in which the two processes' contributions are added into the output accumulator (PluginProcessor.cpp:214-221), i.e.
 * rounding; the exact mode never does this.  A caller's hip_stream is respected: the work it sees is ordered on that stream. */
#define VP_OVERLAP_AUTO 2
int vp_set_overlap(vp_handle *h, int on);
int vp_get_overlap(const vp_handle *h);
/* SURVEY 8(f2), queued audio.  What serves it (round 6): vp_process_blocks[_mono]_device hands the pitch corrector's blocks to ONE launch
 * of vp_k_pitch_ws_mb (exact arithmetic: _x_mb; lpcPitch 16 .. 24: _mb_o24 / _x_mb_o24) per group of up to sixteen (state, frame in flight, voice window and accumulator slice stay on chip between the
 * blocks; 27 M frames/s against 24 M block by block at 256 streams) -- no switch, same bits.  The earlier attempt, a time-parallel
 * analysis front end in front of the serial kernel (vp_k_pitch_front, rounds 3-5), never paid -- its cross-correlations were the same
 * vector work on the same CUs -- and was removed; the two entry points below are kept so that a version-2 caller links: the value is
 * stored and returned, and changes nothing. */
int vp_set_time_parallel(vp_handle *h, int on);
int vp_get_time_parallel(const vp_handle *h);
/* Round 5: which pitch-corrector kernel serves single-block calls of the plugin's own geometry (1024-sample frames, lpcPitch <= 15,
 * up to 256 streams).  1 (default): vp_k_pitch_ws / vp_k_pitch_ws_x, the WAVE-SPECIALISED kernel (csrc/vp_pitch_ws.inc: every frame
 * start's yin() / LPC / marks on four background wavefronts beside the running frame's chunks, PitchProcess.cpp:203-271).  0: the
 * phase kernels (vp_k_pitch_fast_c / vp_k_pitch_c), which also serve every other geometry.  Same output bits either way
 * (tests/test_gpu_round5.py); the switch exists for that test and for same-box A/B timing (tools/ws_ab.py).
 * Under 1, FAST single-block calls of exactly the plugin's geometry at 44.1 kHz (pitch corrector alone, certified YIN, blocks of one
 * to four whole chunks) launch vp_k_pitch_ws_l, the lean build of vp_k_pitch_ws (csrc/vp_pitch_ws_body.inc; +6.6 % on the benched
 * workload, profiles/ws_lean_ab.txt).  2: wave-specialised, GENERIC builds only -- never the lean one.  Same bits again
 * (tests/test_gpu_ws_lean.py). */
int vp_set_wave_specialised(vp_handle *h, int on);
int vp_get_wave_specialised(const vp_handle *h);
/* Diagnostic: symbol of the pitch kernel the handle's LAST process call launched ("" before the first; of a call with several
 * cohorts, the last cohort's).  vp_pitch_kernel_name() names the family the geometry selects; this names the build that ran. */
const char *vp_debug_pitch_symbol(const vp_handle *h);

/* How the YIN difference function (PitchProcess.cpp:350-403) and the pitch frame's LPC autocorrelation
 * (LPC.cpp:44-97) are evaluated.
 * VP_YIN_DIRECT (default): the reference's O(F tau) sums in its own order; decisions bit-identical.
 * VP_YIN_FFT: Wiener-Khinchin accelerator (one forward + one inverse radix-2 FFT of >= F + tauMax points in
 * LDS).  Values differ by ~1e-13 relative, so a threshold decision CAN differ on a near-tie; the measured
 * rate of frames whose period differs is reported by tests/test_gpu_parity.py.
 * VP_YIN_XCORR: the difference function as energies minus a cross-correlation (fused multiply-adds: a third of the
 * arithmetic), CERTIFIED: its values differ from the reference's by at most 2^-39 of the window energy, every
 * comparison the pitch decision rests on is checked against what that can do to it, and a frame with a comparison
 * too close to call is recomputed in the reference's arithmetic.  Decisions -- and therefore the output -- are
 * bit-identical to VP_YIN_DIRECT by construction; only the LPC autocorrelation stays as it is. */
#define VP_YIN_DIRECT 0
#define VP_YIN_FFT 1
#define VP_YIN_XCORR 2
#define VP_YIN_XCORR_FORCE_FALLBACK 3   /* diagnostic: as XCORR, but every frame is treated as "too close to call" */
int vp_set_yin_mode(vp_handle *h, int mode);
int vp_get_yin_mode(const vp_handle *h);

/* AudioProcessor::getLatencySamples() after setLatencySamples(max(F, W)) (PluginProcessor.cpp:175,183). */
int vp_get_latency(const vp_handle *h);
/* N, F, H, C, W, h, samplesToKeep, latency, inSize, outSize, tauMax, chunksPerFrame
 * (MyBuffer.h:37-43 getters + PitchProcess/VocoderProcess geometry). */
int vp_get_geometry(const vp_handle *h, int out[12]);
int vp_get_num_streams(const vp_handle *h);

/* Copies one stream's pitch-tracker state to the host (synchronises). */
int vp_read_pitch_state(vp_handle *h, int stream, vp_pitch_state *out);

/* hipDeviceSynchronize on the handle's device, then the verdict on everything launched so far: VP_OK, or the code that poisoned the
 * handle (VP_ERR_TIMEOUT / VP_ERR_HIP).  A host that drives the device-pointer entry points calls this before it trusts their output. */
int vp_synchronize(vp_handle *h);
/* Diagnostic: polls a kernel's bounded inter-wavefront wait makes before it gives up (default 2^22, about a second).  The test
 * suite sets 1 to force the timeout path (tests/test_gpu_round6.py). */
int vp_debug_set_spin_limit(vp_handle *h, int polls);

/* Kernel timing with HIP events on the launch stream (bench.py's roofline figures).
 * vp_profile_enable(h, k) brackets the kernel launches of every k-th process call with events (k = 1: every call;
 * the records cost the stream 2-3 us per bracketed launch, so a throughput measurement samples); vp_profile_read returns, per
 * kernel slot, the accumulated milliseconds and launch count since the last reset.
 * Slots: 0 ingest+gate, 1 vocoder, 2 pitch, 3 emit. */
#define VP_NUM_KERNEL_SLOTS 4
int vp_profile_enable(vp_handle *h, int on);
int vp_profile_read(vp_handle *h, double ms[VP_NUM_KERNEL_SLOTS], long launches[VP_NUM_KERNEL_SLOTS], int reset);
const char *vp_kernel_slot_name(int slot);
/* Symbol of the pitch-kernel build the handle's current geometry and modes select (slot 2 is one of
 * vp_k_pitch[_fast][_c], vp_k_pitch_lite[_fast], vp_k_pitch[_fast]_fft; _c = the common-case builds); "" before prepare. */
const char *vp_pitch_kernel_name(const vp_handle *h);
/* Likewise for slot 1: vp_k_vocoder (LPC orders up to 32 and above 48) / vp_k_vocoder_o48 (orders 33..48), vp_k_vocoder_lite
 * (FAST IIR, more than 256 streams on the workgroup path: two workgroups per CU), or "vp_k_v2_pipeline" -- the lane-per-window
 * pipeline of kernels (vp_k_v2_ingest_stage, _autocorr, _levinson2, _fir2, _energy[_slices], _iir_exact / _iir_fast, _ola) that
 * VP_VOC_AUTO picks above 256 streams with at least 1024 windows per block. */
const char *vp_vocoder_kernel_name(const vp_handle *h);

/* Counts, over all streams since prepare, how often a kernel reached one of the reference's
 * undefined-behaviour sites (back() of an empty vector, yinTemp[tauMax]):
 * same meaning as the oracle's counters. Synchronises. */
int vp_read_ub_counters(vp_handle *h, long out[5]);

/* Slots 0..58: diagnostic build (-DVP_STAMPS) only, per-phase timers (100 MHz ticks) of workgroup 0, all zero in
 * the product build.  Slots 59 / 60 / 61 (every build): wavefronts whose bounded wait for an in-workgroup flag (YIN prefix
 * sums / LPC coefficients / grain table) ran out -- always 0; anything else has also raised VP_ERR_TIMEOUT and poisoned the handle.  Slots 62 / 63 (every build): frames, over all streams, whose pitch decision VP_YIN_XCORR
 * certified / handed to the reference's arithmetic. */
int vp_debug_read_stamps(vp_handle *h, unsigned long long out[64], int reset);
/* Diagnostic build only: per-wavefront timers of the wave-specialised pitch kernel, [4 block types][16 wavefronts][8 slots] (tools/ws_stamps.py). */
int vp_debug_read_ws_stamps(vp_handle *h, unsigned long long out[512], int reset);
/* Diagnostic build only: ticks each of the first n streams' workgroups spent inside the pitch kernel (which stream paces a launch). */
int vp_debug_read_stream_ticks(vp_handle *h, unsigned long long *out, int n, int reset);

/* Standalone STFT round trip: sqrt-Hann window, batched FFT, [spectral stage], inverse FFT, overlap-add, in ONE fused kernel
 * (csrc/vp_stft.hip: one frame per wavefront, the transform's butterflies in registers, overlap-add in LDS, every input sample
 * read from HBM once and every output sample written once).  frame_len must be 1024 or 2048 (eight / sixteen complex points
 * per lane of a wavefront; VP_ERR_GEOMETRY otherwise), hop a divisor of it with 2 <= frame_len / hop <= 16.  NO reference counterpart (the
 * reference contains no FFT): these are the STFT-shaped kernels BASELINE.json's north_star lists, reported
 * on their own by bench.py and checked against numpy.fft / a build-authored NumPy restatement (tests/stft_reference.py: parity
 * unpinned by nature).  vp_stft_roundtrip is the plain round trip (double or single precision), vp_stft_pitch_shift the same with the
 * phase-vocoder pitch shift between the transforms; both serve both frame lengths.
 * d_in/d_out: device float32 [n_streams][n_samples]; d_mag (optional): [n_streams][frames][frame_len/2+1]. */
typedef struct vp_stft vp_stft;
int vp_stft_create(int device, int n_streams, int n_samples, int frame_len, int hop, vp_stft **out);
int vp_stft_destroy(vp_stft *p);
int vp_stft_num_frames(const vp_stft *p);
int vp_stft_roundtrip(vp_stft *p, const float *d_in, float *d_out, float *d_mag, void *hip_stream);
/* The north_star's "per-bin phase unwrap/accumulate" stage between the two transforms: the classic phase-vocoder pitch shift by
 * `semitones` in [-12, 12] (per frame and bin: magnitude and phase; phase advance against the previous frame minus the bin's
 * nominal advance, wrapped to (-pi, pi] -> true frequency; bins move to floor(k ratio + 0.5), magnitudes that land together
 * add; the synthesis phase accumulates the scaled advance).  Each call starts from a zero phase state.  1024- and 2048-point
 * frames, at every hop vp_stft_create admits (kernels vp_k_stft_fused<true, false> and vp_k_stft_pv2k).  The definition that holds for
 * both is tests/stft_reference.py's stft_roundtrip(x, frame_len, hop, ratio = 2^(semitones / 12)): sqrt-Hann window, 1 / sum w^2
 * normalisation, the synthesis phase summed left to right within rounds of four frames and wrapped at a round's last frame, bins 0 and
 * frame_len / 2 real, samples no frame covers 0.  Double precision whatever vp_stft_set_precision says.  VP_ERR_INVALID_ARG for null
 * pointers or |semitones| > 12, VP_ERR_HIP when the device refused the kernels' LDS size at create.  No reference counterpart. */
int vp_stft_pitch_shift(vp_stft *p, const float *d_in, float *d_out, double semitones, void *hip_stream);
/* vp_stft_pitch_shift along a pitch curve (kernels vp_k_stft_pv_curve and vp_k_stft_pv2k_curve): tests/stft_reference.py's
 * stft_roundtrip with `ratio` replaced by ratio[s][f] in frame f -- the previous-frame phases, the accumulator's rounds of four frames and
 * the gather are unchanged.  A curve that is constant per stream gives vp_stft_pitch_shift's bits.  Both frame lengths, every hop,
 * always double, one workgroup per stream.
 * d_ratio: device double [n_streams][vp_stft_num_frames(p)], the pitch ratio of frame f of stream s.
 * Used as r = fmin(fmax(r, 0.5), 2.0), so a NaN becomes 0.5.
 * VP_ERR_INVALID_ARG for null pointers, VP_ERR_HIP when the device refused the kernels' LDS size at create. */
int vp_stft_pitch_shift_curve(vp_stft *p, const float *d_in, float *d_out, const double *d_ratio, void *hip_stream);
/* vp_stft_pitch_shift_curve with PEAK LOCKING (kernel vp_k_stft_pv_lock; Laroche & Dolson 1999, identity locking with integer offsets).
 * The plain stage moves every bin on its own and runs one phase accumulator per synthesis bin, which tears a sinusoid's main lobe apart
 * and loses the phase relation of its bins ("phasiness": a +7 semitone tone comes out 9 dB low).  Here every frame's spectral peaks are
 * found, each bin belongs to its nearest peak, and a peak's whole region is translated by one integer offset and rotated by one
 * accumulated angle.  The definition is tests/pv_lock_reference.py.  Per stream pprev[k] = theta[k] = 0; per frame, with r the frame's
 * ratio clamped as in vp_stft_pitch_shift_curve, O = frame_len / hop, phases in turns:
 *   m, p magnitude and phase of the analysis bins k <= 512;  d = p - pprev - k / O, d -= rint(d);  nu = k + d O;  pprev = p;
 *   k is a peak iff m[k] > 0, m[k] > m[k-1], m[k-2] and m[k] >= m[k+1], m[k+2] (neighbours outside 0 .. 512 do not count);
 *   own[k] is the nearest peak, the lower one on equal distance;
 *   per peak P: t = theta[P] + (nu[P] (r - 1)) / O, th[P] = t - rint(t);  P' = floor(P r + 0.5), peaks with P' > 512 are not synthesised;
 *   synthesis bin kk belongs to the nearest P' (the lower on equal distance), its source is k = kk - (P' - P):
 *     Y[kk] = X[k] exp(2 pi i th[P]) if 0 <= k <= 512 and own[k] == P, else 0;  bins 0 and 512 keep their real parts;
 *   theta[k] = th[own[k]] for every k.  A frame without peaks (all zeros) gives Y = 0 and leaves theta.
 * A region is translated whole: at r > 1 the gaps stay empty, at r < 1 neighbouring regions are cut where they meet, not added.  At
 * r = 1 the stage is the identity.  1024-point frames, every hop, always double, one workgroup per stream, no allocation.
 * Out of scope: 2048-point frames; formant correction on top of locking; adding overlapping regions.  Several voices per call are
 * vp_stft_harmonize.  The integer offset costs level (a 0.5 tone leaves at 0.38 at -12 and at +7 semitones): vp_stft_pitch_shift_locked_subbin interpolates.
 * Locking in the time stretch is vp_stft_time_stretch_locked.
 * VP_ERR_INVALID_ARG (null handle, input, output or ratio table) and VP_ERR_GEOMETRY (a 2048-point handle) are reported before the
 * device is touched and vp_stft_last_error says which; VP_ERR_HIP as vp_stft_pitch_shift. */
int vp_stft_pitch_shift_locked(vp_stft *p, const float *d_in, float *d_out, const double *d_ratio, void *hip_stream);
/* vp_stft_pitch_shift_locked with SUB-BIN region offsets (kernel vp_k_stft_pv_lockf; the definition is tests/pv_lockf_reference.py).  The
 * locked stage moves a region by an integer while its angle turns at the true frequency, so the lobe sits up to half a bin (plus the
 * peak's own sub-bin position) from the frequency its phase turns at, and frames do not add up in the overlap-add.  Here peaks,
 * ownership, th[P], P', theta and silent frames are the locked stage's; what changes, with m the magnitudes:
 *   per peak P: delta = 0 if P is 0 or 512, else (m[P-1] - m[P+1]) / (2 (m[P-1] - 2 m[P] + m[P+1])), in [-1/2, 1/2];  D = (P + delta)(r - 1);
 *   synthesis bin kk (its shifted peak P', its peak P):  u = kk - D, u0 = floor(u), f = u - u0;  f == 0: the one tap k = u0, weight 1;
 *     else six taps k_j = u0 + j, j = -2 .. 3, w_j = sinc(f - j) (1/2 + 1/2 cos(pi (f - j) / 3));  a tap counts if 0 <= k_j <= 512 and
 *     own[k_j] == P;  Y[kk] = exp(2 pi i th[P]) sum_j w_j (-1)^(kk - k_j) X[k_j];  bins 0 and 512 keep their real parts.
 * At r = 1 the stage is the identity.  A 0.5 tone leaves at 0.486 - 0.498 where the integer offset gives 0.38 - 0.50
 * (profiles/pv_lockf_quality.txt).  1024-point frames, every hop, always double, one workgroup per stream, no allocation.  Out of
 * scope: the locked time stretch (it keeps integer offsets), 2048-point frames, formant correction on top, adding overlapping regions,
 * single precision.  Arguments, checks, their order and codes as vp_stft_pitch_shift_locked's; the texts begin "locked subbin: ". */
int vp_stft_pitch_shift_locked_subbin(vp_stft *p, const float *d_in, float *d_out, const double *d_ratio, void *hip_stream);
/* The HARMONIZER: n_voices peak-locked copies of the voice, each shifted along its own ratio curve and mixed by its own gain, beside the
 * dry signal, from ONE analysis of every frame (kernel vp_k_stft_harm; the definition is tests/pv_harm_reference.py).  The inverse
 * transform and the overlap-add are linear and the locked stage's analysis does not depend on the ratio, so in exact arithmetic
 *   out = dry[s] roundtrip(x) + sum_v gain[s][v] locked(x, ratio[s][v]),   roundtrip and locked the two calls of those names above;
 * the kernel reads the input, transforms, finds peaks and owners, transforms back and overlap-adds once per frame instead of
 * n_voices + 1 times, and runs only the shifted peaks, the gather and one angle array theta per voice n_voices times.  Per frame the sum
 * is dry X + gain[0] Y_0 + ... in this order, X the analysis spectrum, Y_v the locked stage's synthesis spectrum for voice v (bins 0 and
 * 512 real).  One voice with gain 1 and no dry part has the locked call's bits; all gains 0 with dry 1 has the double round trip's.  A
 * voice with gain 0 still turns its angles, so it can be faded in later.  A frame without a peak contributes its dry term alone.
 * d_ratio: device double [n_streams][n_voices][vp_stft_num_frames(p)], clamped to [0.5, 2] as in the curve call;  d_gain: device double
 * [n_streams][n_voices] or NULL = every gain 1;  d_dry: device double [n_streams] or NULL = 0.  A gain or dry value that is NaN or
 * infinite counts as 0, a finite one is clamped to [-4, 4].  n_voices: 1 .. VP_HARM_MAX_VOICES.  vp_stft_track_harmony below makes the
 * table of voices at scale degrees of the tracked pitch; vp_stft_harmonize_key runs both.  1024-point frames, every hop, always double, one workgroup per stream, no allocation; the runs setting
 * and output aliasing as in the locked call.
 * Out of scope: sub-bin region offsets per voice; formant correction per voice; 2048-point frames; single precision; gains per block
 * or per frame.
 * VP_ERR_INVALID_ARG (null handle, input, output or ratio table; n_voices outside 1 .. 4) and VP_ERR_GEOMETRY (a 2048-point handle:
 * "harmonize: 2048-point frames are not built ...") are reported before the device is touched, in that order, and vp_stft_last_error
 * says which; VP_ERR_HIP as vp_stft_pitch_shift. */
#define VP_HARM_MAX_VOICES 4
int vp_stft_harmonize(vp_stft *p, const float *d_in, float *d_out, int n_voices, const double *d_ratio, const double *d_gain, const double *d_dry,
                      void *hip_stream);
/* vp_stft_pitch_shift_curve with the spectral envelope kept apart from the pitch (kernel vp_k_stft_pv_formant): the formants stay where
 * they were, or move by a ratio of their own, while the pitch follows d_ratio.  The definition is tests/pv_formant_reference.py.  Per
 * frame, with m the analysis magnitudes, r the frame's pitch ratio and phi the stream's formant ratio (both clamped to [0.5, 2] as in
 * vp_stft_pitch_shift_curve):
 *   L[k] = 0.5 log(m[k]^2 + 1e-12), k <= 512;  c = irfft(L, 1024);  c[n] kept for n < lifter, halved at n = lifter, 0 beyond
 *   (symmetric);  le = rfft(c).real, the smoothed log envelope;  at(rho)[kk] = le interpolated linearly at clip(kk / rho, 0, 512);
 *   every gathered synthesis magnitude is multiplied by exp(clip(at(phi)[kk] - at(r)[kk], -ln 16, ln 16)).
 * phi = 1 preserves the formants, phi = 2^(st / 12) moves them by st semitones, phi = r gives vp_stft_pitch_shift_curve's bits.  The
 * correction has no state across frames.  1024-point frames, every hop, always double, one workgroup per stream, no allocation.
 * d_ratio: device double [n_streams][vp_stft_num_frames(p)]; d_formant: device double [n_streams] or NULL = 1.0 everywhere;
 * lifter: VP_FORMANT_LIFTER_MIN .. VP_FORMANT_LIFTER_MAX samples (callers default it to 32).  The tables are read when the kernel runs.
 * VP_ERR_INVALID_ARG (null handle, input, output or ratio table; lifter out of range) and VP_ERR_GEOMETRY (a 2048-point handle: that
 * build is not made) are reported before the device is touched and vp_stft_last_error says which; VP_ERR_HIP as vp_stft_pitch_shift. */
#define VP_FORMANT_LIFTER_MIN 4
#define VP_FORMANT_LIFTER_MAX 64
int vp_stft_pitch_shift_formant(vp_stft *p, const float *d_in, float *d_out, const double *d_ratio, const double *d_formant, int lifter,
                                void *hip_stream);
/* STFT cross-synthesis, the vocoder of this path (kernel vp_k_stft_cross): the spectral envelope of one signal, the voice, imposed on
 * another, the carrier.  The definition is tests/pv_cross_reference.py.  Frames, window, scale and overlap-add are vp_stft_roundtrip's;
 * between the transforms, per frame:
 *   V = rfft(w v_frame), C = rfft(w c_frame);
 *   env(m): L[k] = 0.5 log(m[k]^2 + 1e-12), k <= 512;  c = irfft(L, 1024);  c[n] kept for n < lifter, halved at n = lifter, 0 beyond
 *   (symmetric);  env = rfft(c).real -- vp_stft_pitch_shift_formant's smoothed log envelope;
 *   d = fmin(fmax(depth[s], 0), 1) (a NaN is 0; a NULL table is 1);  delta = min(d (env(|V|) - env(|C|)), ln 256);  Y = C exp(delta).
 * The gain is real, so bins 0 and 512 stay real by themselves.  Only the upper clamp exists (+48 dB: a carrier band without energy is not
 * amplified without limit); a silent voice silences the carrier.  depth 0 gives vp_stft_roundtrip's bits of the carrier, and so does
 * voice == carrier up to rounding.  The stage has no state across frames: streams split into runs as in vp_stft_roundtrip
 * (vp_stft_set_runs applies).  1024-point frames, every hop, always double (whatever vp_stft_set_precision says), no allocation.
 * d_voice, d_carrier, d_out: device float [n_streams][n_samples]; d_out must not alias an input (a run re-reads the frames in front of
 * it).  d_depth: device double [n_streams] or NULL; lifter: VP_FORMANT_LIFTER_MIN .. VP_FORMANT_LIFTER_MAX (callers default it to 32).
 * VP_ERR_INVALID_ARG (null handle or pointer; lifter out of range) and VP_ERR_GEOMETRY (a 2048-point handle: "2048-point frames are not
 * built") are reported before the device is touched, in that order; vp_stft_last_error says which under the name "cross". */
int vp_stft_cross_synth(vp_stft *p, const float *d_voice, const float *d_carrier, float *d_out, const double *d_depth, int lifter, void *hip_stream);
/* pow(2, st / 12) exactly as vp_stft_pitch_shift / vp_pv_set_semitones compute it (same bits).
 * VP_ERR_INVALID_ARG if an entry is outside +-12 or not finite; nothing is written then.  Host arrays; no device is touched. */
int vp_semitones_to_ratios(const double *semitones, double *ratios, long n);
/* Time stretch (kernels vp_k_stft_pv_stretch and vp_k_stft_pv2k_stretch): vp_stft_pitch_shift with the frames ANALYSED at caller-given
 * positions.  The handle's n_samples is the OUTPUT row length T; frame f of stream s is read at input sample
 * q = clamp(d_pos[s][f], 0, n_in - frame_len) and overlap-added at output sample f hop, so duration and pitch are independent.  The
 * definition is tests/pv_stretch_reference.py: stft_roundtrip's stage with the unwrap taking the frame's own analysis advance
 * D_0 = hop, D_f = clamp(q_f - q_(f-1), 1, frame_len) -- d = (p - p_prev) / 2 pi - (k D) / frame_len, wrapped to [-1/2, 1/2] turns, true
 * frequency k + d (frame_len / D) -- and the synthesis increment unchanged (the synthesis hop is hop).  Any table is defined and gives a
 * finite output; the table d_pos[s][f] = f hop with n_in = T gives vp_stft_pitch_shift's bits.  Both frame lengths, every hop, always
 * double, one workgroup per stream, no allocation.
 * d_in: device float [n_streams][n_in]; d_pos: device int [n_streams][vp_stft_num_frames(p)]; d_out: device float [n_streams][T];
 * semitones in [-12, 12], 0 = pure stretch.  The table is read when the kernel runs: keep it unchanged until then.
 * VP_ERR_INVALID_ARG for null pointers, n_in < frame_len or |semitones| > 12 (checked before the device is touched), VP_ERR_HIP when the
 * device refused the kernels' LDS size at create. */
int vp_stft_time_stretch(vp_stft *p, const float *d_in, int n_in, const int *d_pos, float *d_out, double semitones, void *hip_stream);
/* The time stretch with PEAK LOCKING (kernel vp_k_stft_pv_stretch_lock): vp_stft_time_stretch's framing -- positions q_f, advances D_f,
 * frame f overlap-added at output sample f hop -- with vp_stft_pitch_shift_locked's stage and its per-frame, per-stream ratio table
 * (clamped to [0.5, 2], a NaN is 0.5).  The definition is tests/pv_stretch_lock_reference.py: the locked stage with two changes, phases in
 * turns:
 *   unwrap    d = p - pprev - (k D_f) / frame_len, d -= rint(d);  nu = k + d (frame_len / D_f);
 *   rotation  per peak P: t = theta[P] + nu[P] ((r hop - D_f) / frame_len), th[P] = t - rint(t) -- the analysis phase of a partial advances
 *             nu D / frame_len turns per frame, the synthesis must advance r nu hop / frame_len.
 * Peaks, ownership, the shift P' = floor(P r + 0.5), the gather, the propagation of theta, silent frames and the real bins 0 and 512 are
 * unchanged.  The table d_pos[s][f] = f hop with n_in = T gives vp_stft_pitch_shift_locked's bits.  1024-point frames, every hop, always
 * double, one workgroup per stream, no allocation.  Out of scope: a streaming form, 2048-point frames, formant correction.
 * d_in: device float [n_streams][n_in]; d_pos: device int [n_streams][vp_stft_num_frames(p)]; d_out: device float [n_streams][T];
 * d_ratio: device double [n_streams][vp_stft_num_frames(p)].  Both tables are read when the kernel runs.
 * VP_ERR_INVALID_ARG (a null handle or pointer, n_in < frame_len) and VP_ERR_GEOMETRY (a 2048-point handle) are reported before the
 * device is touched and vp_stft_last_error says which; VP_ERR_HIP as vp_stft_pitch_shift. */
int vp_stft_time_stretch_locked(vp_stft *p, const float *d_in, int n_in, const int *d_pos, float *d_out, const double *d_ratio, void *hip_stream);
/* A constant stretch's table: pos[f] = min(floor(f hop / stretch), n_in - frame_len), f < n_frames; stretch = output duration / input
 * duration in [0.25, 4].  VP_ERR_INVALID_ARG outside that range, for a stretch that is not finite, n_in < frame_len or hop <= 0; nothing
 * is written then.  Host array; no device is touched. */
int vp_stretch_positions(int *pos, int n_frames, int hop, double stretch, int n_in, int frame_len);
/* TRANSIENT-PRESERVING locked time stretch: do not stretch across an attack, and restart the phases at it.  Four calls, in this order:
 * vp_stft_onset_flux (device), vp_onset_pick and vp_stretch_positions_transient (host, exact), vp_stft_time_stretch_locked_reset (device).
 * The definition is tests/pv_transient_reference.py.  1024-point frames, every hop of the locked stretch, always double, one-shot only.
 * Out of scope: a streaming form, 2048-point frames, sub-bin offsets, single precision, detection on the device end to end, resets in the
 * pitch-shift-only calls.  Recorded figures: profiles/pv_transient_quality.txt (the definition's, on bursts and plucks),
 * profiles/pv_onset_errors.txt, profiles/pv_transient_bench.txt (the reset kernel on an all-zero table 0.98 x vp_stft_time_stretch_locked, the
 * flux kernel 478 M frames/s on one MI355X at 256 streams x 65 536 samples, hop 256).
 *
 * vp_onset_num_frames: nG = (n_in - frame_len) / hop + 1, the frames of the INPUT's own grid g hop; VP_ERR_INVALID_ARG for
 * n_in < frame_len, frame_len <= 0 or hop <= 0. */
int vp_onset_num_frames(int n_in, int frame_len, int hop);
/* Onset flux (kernel vp_k_stft_onset_flux): over the grid g hop of every row of d_in [n_streams][n_in], with the handle's window,
 *   M_g = |rfft(x[g hop : g hop + frame_len] w)| over bins 0 .. 512;  mass[g] = sum_k M_g[k];
 *   flux[0] = 0,  flux[g] = sum_k max(M_g[k] - M_(g-1)[k], 0)  otherwise (the rectified spectral flux; a NaN stays a NaN).
 * Sums run in a fixed order, so a row's figures do not depend on its neighbours or on n_streams.  Against the NumPy definition the
 * difference is rounding: at most 4 513 log2(frame_len) 2^-53 (|x_g w|_2 + |x_(g-1) w|_2) per frame (tested).
 * d_flux, d_mass: device double [n_streams][vp_onset_num_frames(n_in, frame_len, hop)].  The handle's n_samples plays no part.  No
 * allocation, no synchronisation: the tables are ready when hip_stream reaches the call's end.
 * VP_ERR_INVALID_ARG (a null handle or pointer, n_in < frame_len) and VP_ERR_GEOMETRY (a 2048-point handle) are reported before the device
 * is touched and vp_stft_last_error says which under the name "onset flux"; VP_ERR_HIP as vp_stft_pitch_shift. */
int vp_stft_onset_flux(vp_stft *p, const float *d_in, int n_in, double *d_flux, double *d_mass, void *hip_stream);
/* Onsets of one row from its flux and mass tables: onsets[g] = 1 iff ALL of
 *   flux[g] > 0,   flux[g] >= thr mass[g],   flux[g] > flux[g-1],   flux[g] >= flux[g+1]
 * hold, else 0; a missing neighbour (g = 0, g = n - 1) counts as -infinity and a NaN anywhere in a comparison is "no".  thr in [0, 1];
 * VP_DEFAULT_ONSET_THRESHOLD is the offline tool's default.  VP_ERR_INVALID_ARG for a null pointer, n < 0 or thr outside [0, 1] or not
 * finite; nothing is written then.  Host arrays; no device is touched. */
#define VP_DEFAULT_ONSET_THRESHOLD 0.2
int vp_onset_pick(const double *flux, const double *mass, int n, double thr, unsigned char *onsets);
/* The position table and the reset flags of a constant stretch that leaves the onsets alone, for one row: pos int [n_frames], reset
 * unsigned char [n_frames], from onsets [nG], nG = vp_onset_num_frames(n_in, frame_len, hop).
 *   base[f] = min(floor(f hop / stretch), n_in - frame_len)                          (vp_stretch_positions's formula, in double).
 *   Anchors start as [(0, 0)].  The onsets g in increasing order: fc = floor(g stretch + 0.5), a = fc - K, b = fc + K; g is accepted iff
 *     g - K >= 0,  g + K <= nG - 1,  a > the last anchor's frame,  b < n_frames - 1,
 *     (g - K) hop >= the last anchor's position,  (g + K) hop <= base[n_frames - 1];
 *   then the anchors (a, (g - K) hop) and (b, (g + K) hop) are appended and reset[a] = 1.  The last anchor is
 *   (n_frames - 1, base[n_frames - 1]).
 *   Between consecutive anchors (f0, p0), (f1, p1): pos[f] = p0 + ((f - f0) (p1 - p0)) / (f1 - f0) in 64-bit integers (floor).
 * A span of 2 K + 1 frames around an accepted onset is read exactly hop apart -- no stretch there --, the stretch is made up between the
 * spans, and the table is non-decreasing.  WITH NO ACCEPTED ONSET THE TABLE IS THE TWO-ANCHOR LINE from (0, 0) to
 * (n_frames - 1, base[n_frames - 1]), not vp_stretch_positions's table.  K in [VP_ONSET_SPAN_MIN, VP_ONSET_SPAN_MAX] = [1, 8]; the
 * tools' default is max(frame_len / (2 hop), 1).
 * VP_ERR_INVALID_ARG for vp_stretch_positions's errors, a null table or K out of range; nothing is written then.  Host arrays. */
#define VP_ONSET_SPAN_MIN 1
#define VP_ONSET_SPAN_MAX 8
int vp_stretch_positions_transient(int *pos, unsigned char *reset, int n_frames, int hop, double stretch, int n_in, int frame_len,
                                   const unsigned char *onsets, int K);
/* vp_stft_time_stretch_locked with a PHASE RESET on flagged frames (kernel vp_k_stft_pv_stretch_lock_reset): one change in the rotation
 * rule -- on a frame with d_reset[s][f] != 0 (any non-zero byte), th[P] = 0 for every peak P instead of theta[P] + the advance.  pprev,
 * theta[k] = th[own[k]] and the frame without peaks (Y = 0, theta left, flagged or not) are unchanged.  At ratio 1 and frames hop apart
 * the advance is exactly 0, so from a reset on the stage is the identity: a span planned by vp_stretch_positions_transient leaves with
 * the input's spectrum -- the attack is neither smeared nor preceded by an echo.  In the definition that is bit for bit; the kernel turns
 * every region by the angle 0 through the stage's cosine fit, whose value there is 1 + 2^-52, so a bin may be one unit in the last place
 * of the double off, and the float32 output behind a reset equals vp_stft_roundtrip's on every sample the GPU test compares.  An all-zero
 * table gives vp_stft_time_stretch_locked's bits (tested).
 * d_reset: device unsigned char [n_streams][vp_stft_num_frames(p)], read when the kernel runs; every other argument, the geometry and the
 * errors are vp_stft_time_stretch_locked's, under the name "stretch locked reset", and a null d_reset is VP_ERR_INVALID_ARG.  No
 * allocation. */
int vp_stft_time_stretch_locked_reset(vp_stft *p, const float *d_in, int n_in, const int *d_pos, float *d_out, const double *d_ratio,
                                      const unsigned char *d_reset, void *hip_stream);
/* Pitch tracker and automatic correction (kernel vp_k_yin_track, csrc/vp_track.hip): PitchProcess's own decision -- YIN, the key's
 * nearest note, beta = closestFreq / pitch, with the plugin's numbers fMin 100, fMax 800, yinTol 0.25 and the Notes tables -- for every
 * frame of the handle at once, one wavefront per frame.  The definition is tests/pv_track_reference.py, and the result equals it
 * bit for bit (period and ratio; no tolerance):
 *   tauMax = ceil(fs / 100), tau0 = floor(fs / 800); 8000 <= sample_rate <= 51200 (tauMax <= 512) and n_samples >= frame_len + tauMax;
 *   frame f reads the frame_len + tauMax samples from b = min(f hop, n_samples - (frame_len + tauMax)) on -- the last frames of a row share a
 *   clamped window, no frame reads outside its row;
 *   d[k] = sum_{i < frame_len} (x[b + i] - x[b + i + k])^2 in double, each its own left-to-right sum; d[0] = 1, then tmp += d[k],
 *   d[k] *= k / tmp in increasing k; d[tauMax] = 0; the threshold walk of PitchProcess.cpp:429-447 gives the period, or 0 (unvoiced);
 *   period > 0: pitch = fs / period, ratio = closest(pitch, key) / pitch; period 0: ratio = 1.0 exactly.
 * Frames are independent: no gate, no hold of the last voiced ratio, no smoothing (the streaming tracker below, vp_pv_tracker_*, has both).  Float32-denormal input samples are outside the
 * definition's domain (the kernels widen them to 0).
 * d_in: device float [n_streams][n_samples]; d_key: device int [n_streams], Notes::key 0..12 (12 = chromatic; any other value counts
 * as 12), or NULL = chromatic everywhere; d_period: device int [n_streams][vp_stft_num_frames(p)] or NULL; d_ratio: device double of
 * that shape or NULL; not both NULL.  No allocation, no synchronisation.
 * VP_ERR_INVALID_ARG (null handle or input, both outputs NULL, sample rate out of range) and VP_ERR_GEOMETRY (rows shorter than
 * frame_len + tauMax) are reported before the device is touched; vp_stft_last_error says which. */
int vp_track_tau_max(double sample_rate);                    /* ceil(sample_rate / 100), or VP_ERR_INVALID_ARG outside 8000 .. 51200 */
int vp_stft_track_pitch(vp_stft *p, const float *d_in, double sample_rate, const int *d_key, int *d_period, double *d_ratio, void *hip_stream);
/* vp_stft_track_pitch followed by vp_stft_pitch_shift_curve along its table, on the same stream: the output has the bits of those two
 * calls.  d_ratio is required (result and scratch), d_period optional.  Both frame lengths, every hop.  Errors as the two calls'. */
int vp_stft_autotune(vp_stft *p, const float *d_in, float *d_out, double sample_rate, const int *d_key, int *d_period, double *d_ratio,
                     void *hip_stream);
/* vp_stft_track_pitch followed by vp_stft_pitch_shift_formant along its table, on the same stream: the bits of those two calls.
 * Arguments as vp_stft_autotune's plus d_formant and lifter; errors as the two calls', all before the device is touched. */
int vp_stft_autotune_formant(vp_stft *p, const float *d_in, float *d_out, double sample_rate, const int *d_key, int *d_period, double *d_ratio,
                             const double *d_formant, int lifter, void *hip_stream);
/* KEY-AWARE VOICES (kernel vp_k_yin_track_voices, csrc/vp_track.hip): vp_stft_track_pitch's decision for every frame, then n_voices
 * ratios that put a voice at scale degrees of the note the tracker chose -- "a third and a fifth above, in the key" -- in the layout
 * vp_stft_harmonize takes.  The definition is tests/pv_harmkey_reference.py, and period and ratio equal it bit for bit:
 *   the harmony table of key k is H_k = Notes::buildFreqVect(k) through the filter 25 .. 3200 Hz instead of the tracker's 100 .. 800 Hz:
 *   the tracker's table (its n entries and the popped slot) is the slice H_k[off_k .. off_k + n_k] of it, bit for bit, and twelve steps
 *   above the slice exist in every key (checked where the handle builds the tables, so no index leaves a table upwards);
 *   period > 0: pitch = fs / period; c = the index in the tracker's table of the entry getClosestFreq returns (0 .. n; n is the popped
 *   slot); voice v has the degree d = clamp(d_degree[s][v], -12, 12), counted in steps of the key's table -- scale degrees in the twelve
 *   scale keys, semitones in the chromatic key --; j = max(off + c + d, 0) and ratio[s][v][f] = H_k[j] / pitch, that one division.
 *   Degree 0 has vp_stft_track_pitch's ratio, bit for bit.  The clamp at 0 binds for low notes and large negative degrees (104 Hz in
 *   key 11 with d = -7);
 *   period 0: ratio[s][v][f] = d_unvoiced[s][v]; NULL = 1.0 everywhere; a NaN or an infinity counts as 1.0.
 * Frames are independent, as in vp_stft_track_pitch: no hold, no smoothing (vp_pv_tracker_process_blocks_voices_device has both).  The
 * ratios are not clamped here; vp_stft_harmonize clamps to [0.5, 2] as for any table.
 * d_in, d_key, sample_rate, d_period: as vp_stft_track_pitch's; d_degree: device int [n_streams][n_voices], required, read by the kernel
 * only; d_unvoiced: device double [n_streams][n_voices] or NULL; d_ratio: device double [n_streams][n_voices][vp_stft_num_frames(p)] or
 * NULL; d_period and d_ratio not both NULL.  n_voices: 1 .. VP_HARM_MAX_VOICES.  Both frame lengths, every hop.  No allocation, no
 * synchronisation.  Errors: vp_stft_track_pitch's, then VP_ERR_INVALID_ARG for n_voices outside 1 .. 4 and for a null degree table
 * ("track harmony: ..."), all before the device is touched; vp_stft_last_error says which.
 * Out of scope: per-voice formant correction or sub-bin offsets; a table of chords per degree; smoothing in this batch form; note input. */
int vp_stft_track_harmony(vp_stft *p, const float *d_in, double sample_rate, const int *d_key, int n_voices, const int *d_degree,
                          const double *d_unvoiced, int *d_period, double *d_ratio, void *hip_stream);
/* vp_stft_track_harmony followed by vp_stft_harmonize along its table, on the same stream: the output has the bits of those two calls.
 * d_ratio is required (result and scratch), d_period optional; d_gain and d_dry as vp_stft_harmonize's.  1024-point frames:
 * VP_ERR_GEOMETRY for a 2048-point handle, with the harmonizer's message.  Errors as the two calls' (the null output or table first), all
 * before the device is touched. */
int vp_stft_harmonize_key(vp_stft *p, const float *d_in, float *d_out, double sample_rate, const int *d_key, int n_voices, const int *d_degree,
                          const double *d_unvoiced, const double *d_gain, const double *d_dry, int *d_period, double *d_ratio, void *hip_stream);
/* THE FINE TRACKER (kernels vp_k_yin_track_fine and vp_k_yin_track_voices_fine, csrc/vp_track_fine_kernels.inc): the same decision, with
 * the period refined below one sample by a parabola through the normalised function d' around its minimum (step 5 of the YIN paper).  The
 * integer period quantises the pitch to +-1/2 sample (+-6 cents at 300 Hz, +-15 at 780 Hz at 44.1 kHz); refined, the error of a steady
 * voice stays below a third of a cent (profiles/pv_track_fine_quality.txt).  The definition is tests/pv_track_fine_reference.py, bit for bit:
 *   tau > 0 the integer period, a = d'[tau - 1], b = d'[tau], c = d'[tau + 1];
 *   refine iff tau - 1 >= 1 and tau + 1 <= tauMax - 1 (neither lag 0 nor the guard slot is a neighbour), a >= b, c >= b, and
 *   den = (a - b) + (c - b) is > 0 and finite; then tau_fine = tau + (0.5 (a - c)) / den, |tau_fine - tau| <= 1/2; else tau_fine = tau;
 *   pitch = fs / tau_fine, ratio = closest(pitch, key) / pitch: the note is looked up again, on the refined pitch, and may differ from
 *   the integer tracker's near the midpoint between two notes.  Unvoiced: period 0, tau_fine 0.0, ratio 1.0.  A NaN fails a comparison.
 * vp_stft_set_track_mode selects, per handle, the tracker of vp_stft_track_pitch, vp_stft_autotune, vp_stft_autotune_formant,
 * vp_stft_track_harmony (the voices' note index and division use the refined pitch) and vp_stft_harmonize_key: VP_TRACK_INTEGER (the
 * default: what those calls always did, bit for bit) or VP_TRACK_FINE; any other value is VP_ERR_INVALID_ARG.  Signatures, checks,
 * messages, no allocation and no synchronisation are the same in both modes.
 * vp_stft_track_pitch_fine always refines, whatever the mode, and also returns the refined period: d_period_fine, device double
 * [n_streams][vp_stft_num_frames(p)].  Any of the three outputs may be NULL, not all three (VP_ERR_INVALID_ARG, "pitch tracker: period,
 * refined period and ratio outputs are all null"); every other argument, check and message as vp_stft_track_pitch's. */
#define VP_TRACK_INTEGER 0
#define VP_TRACK_FINE 1
int vp_stft_set_track_mode(vp_stft *p, int mode);
int vp_stft_get_track_mode(const vp_stft *p);                /* the mode, or VP_ERR_INVALID_ARG on NULL */
int vp_stft_track_pitch_fine(vp_stft *p, const float *d_in, double sample_rate, const int *d_key, int *d_period, double *d_period_fine,
                             double *d_ratio, void *hip_stream);
/* The message of the last tracker / autotune / formant / harmony call that failed on this handle ("" before any; the pointer is valid until the next call). */
const char *vp_stft_last_error(const vp_stft *p);
int vp_stft_is_fused(const vp_stft *p);                      /* 1 (every handle runs the fused kernel; kept for older callers) */
/* Diagnostic: cut every stream into this many runs of frames (one workgroup each) instead of choosing from the batch size
 * (0 = automatic).  The output does not depend on it (tests). */
int vp_stft_set_runs(vp_stft *p, int runs_per_stream);
/* Arithmetic of vp_stft_roundtrip's transforms.  VP_STFT_F64 (default): double, as everything else in this library.  VP_STFT_F32: the
 * transform, split and merge in single precision (vp_k_stft_fused32: an f32 vector instruction issues in half the cycles of an fp64 one,
 * the kernel needs half the registers and half the LDS bytes) -- input and output are float32 either way; the result differs from the
 * default's by rounding (~2e-7 of the signal's scale; the north_star's bound is 1e-4 RMS).  Both frame lengths
 * (vp_k_stft_fused32, vp_k_stft_fused2k32); vp_stft_pitch_shift always runs in double (its phases accumulate over the whole stream). */
#define VP_STFT_F64 0
#define VP_STFT_F32 1
int vp_stft_set_precision(vp_stft *p, int precision);
int vp_stft_get_precision(const vp_stft *p);

/* Streaming phase vocoder: vp_stft_pitch_shift's pitch shifter driven block by block, with per-stream state (no reference counterpart;
 * BASELINE configs[1] "256 mono streams, +-12-semitone phase-vocoder pitch shift, 1024-pt FFT hop 256").  One handle holds S independent
 * streams, frame length F = 1024, hop = 64, 128, 256 or 512 (vp_stft_supported(1024, hop); VP_ERR_GEOMETRY otherwise), block size N >= 1
 * fixed at create.
 *  - Per stream, frame f covers input samples [f hop, f hop + F) of everything the stream received since create or its last reset (the
 *    one-shot's frame grid).  A frame is computed in the call in which its last input sample arrives, with the interval in force for
 *    that call.
 *  - Latency L = F - gcd(N, hop) (vp_pv_get_latency): the smallest value at which every output sample is finished -- covered by all the
 *    frames that will ever cover it -- when it is emitted.  N = 1024 or 4096 at hop 256: 768; N = 64: 960; N = 100: 1020.
 *  - Output sample t of a stream is sample t - L of the one-shot result; the first L output samples are 0.  With a constant interval the
 *    concatenated outputs of any number of calls, less the first L samples, are BIT-IDENTICAL to vp_stft_pitch_shift run on the
 *    concatenated input with that interval, over every sample emitted; how the blocks are grouped into calls (one or n blocks per call,
 *    host or device entry point) does not change a bit.
 *  - vp_pv_set_semitones / vp_pv_reset take effect at the next process call issued after them; a call already enqueued does not see
 *    them.  The changes travel in that call's kernel arguments (ordered on its hip_stream, no host memory read later, no allocation).
 *    |semitones| <= 12, default 0; stream -1 = every stream.
 *  - After vp_pv_reset(stream) that stream behaves like a freshly created one with the same interval: its frame grid restarts at the
 *    next call, its pending overlap-add tail is dropped.  The other streams are untouched.
 * Device memory is allocated at create only (state: ~16 KB per stream; the host call's staging); vp_pv_debug_alloc_count() stays
 * constant across process calls.  Arguments are checked before the device is touched: VP_ERR_INVALID_ARG (null pointer, non-positive
 * size, stream out of range, |semitones| > 12), VP_ERR_GEOMETRY (frame_len != 1024, unsupported hop), VP_ERR_NO_DEVICE (no GPU). */
typedef struct vp_pv vp_pv;
int vp_pv_create(int device, int n_streams, int block_size, int frame_len, int hop, vp_pv **out);
int vp_pv_destroy(vp_pv *p);
int vp_pv_get_latency(const vp_pv *p);                                  /* F - gcd(N, hop) */
int vp_pv_set_semitones(vp_pv *p, int stream, double semitones);        /* stream -1 = all; |s| <= 12; default 0 */
int vp_pv_get_semitones(const vp_pv *p, int stream, double *semitones); /* what the next call uses */
int vp_pv_reset(vp_pv *p, int stream);                                  /* stream -1 = all */
/* host float [S][N] -> [S][N]; synchronous */
int vp_pv_process_block(vp_pv *p, const float *in, float *out);
/* device float [n_blocks][S][N] -> [n_blocks][S][N] (block b's slab is what vp_pv_process_block would take), enqueued on hip_stream
 * (a hipStream_t, NULL = default stream) without synchronising, like vp_process_blocks_device */
int vp_pv_process_blocks_device(vp_pv *p, const float *d_in, float *d_out, int n_blocks, void *hip_stream);
/* The same call with one pitch ratio per block and stream (kernel vp_k_pv_stream_curve).
 * d_ratio: device double [n_blocks][S]. A frame is computed with the ratio of the block in which its last sample arrives (clamped as
 * in vp_stft_pitch_shift_curve).  Pending vp_pv_reset calls apply as in any call.  The interval set by vp_pv_set_semitones is neither
 * used nor changed by this call: it is stored as usual and holds again from the next plain call on.  The table is read when the kernel
 * runs: keep it unchanged until then.  No allocation. */
int vp_pv_process_blocks_curve_device(vp_pv *p, const float *d_in, float *d_out, const double *d_ratio, int n_blocks, void *hip_stream);
/* vp_pv_process_blocks_curve_device with vp_stft_pitch_shift_locked's stage (kernel vp_k_pv_stream_lock): d_ratio device double
 * [n_blocks][S], a frame takes the ratio of the block in which its last sample arrives.  The stream's record is unchanged: theta lives in
 * the array that holds the plain calls' synthesis accumulator and pprev in the array of the previous frame's phases.  Latency, call
 * bookkeeping, pending interval changes and resets are the curve call's; a reset stream starts from zeros.  The output, less the latency,
 * is bit-identical to vp_stft_pitch_shift_locked on the concatenated input with the table expanded per frame.  Locked, curve, plain and
 * formant calls may follow each other on one handle: they share the two arrays, so after a change of kind the output is defined and
 * finite but carries a phase jump -- a caller who minds that resets the stream (vp_pv_reset) at the change.  No allocation. */
int vp_pv_process_blocks_locked_device(vp_pv *p, const float *d_in, float *d_out, const double *d_ratio, int n_blocks, void *hip_stream);
/* vp_pv_process_blocks_locked_device with vp_stft_pitch_shift_locked_subbin's stage (kernel vp_k_pv_stream_lockf): table, record, state
 * arrays, latency, bookkeeping, checks and codes are the locked call's.  The output, less the latency, is bit-identical to
 * vp_stft_pitch_shift_locked_subbin on the concatenated input with the table expanded per frame.  Sub-bin, locked, curve, plain and
 * formant calls may follow each other on one handle under the locked call's rule.  No allocation. */
int vp_pv_process_blocks_locked_subbin_device(vp_pv *p, const float *d_in, float *d_out, const double *d_ratio, int n_blocks, void *hip_stream);
/* vp_pv_process_blocks_curve_device with vp_stft_pitch_shift_formant's correction (kernel vp_k_pv_stream_formant): d_formant device
 * double [S] or NULL = 1.0, lifter as there (VP_ERR_INVALID_ARG outside 4 .. 64, before the device is touched).  The stream's state
 * record, latency and call bookkeeping are the curve call's, so formant, curve and plain calls mix freely on one handle; pending resets
 * and interval changes behave exactly as in a curve call.  The output, less the latency, is bit-identical to vp_stft_pitch_shift_formant
 * on the concatenated input with the table expanded per frame.  No allocation. */
int vp_pv_process_blocks_formant_device(vp_pv *p, const float *d_in, float *d_out, const double *d_ratio, const double *d_formant, int lifter,
                                        int n_blocks, void *hip_stream);
long vp_pv_debug_alloc_count(const vp_pv *p);                           /* constant across process calls */

/* Streaming cross-synthesis: vp_stft_cross_synth driven block by block (kernel vp_k_xs_stream).  One handle holds S independent
 * streams of two inputs each, frame length 1024 (VP_ERR_GEOMETRY otherwise, also for a hop vp_stft_supported(1024, hop) refuses), block
 * size N >= 1 fixed at create.  Frame grid, latency L = F - gcd(N, hop) and call bookkeeping are vp_pv_*'s: output sample t of a stream is
 * sample t - L of the one-shot result on everything received, the first L samples are 0, and the concatenated outputs are BIT-IDENTICAL
 * to vp_stft_cross_synth over every sample emitted however the blocks are grouped into calls.  depth and lifter are the call's (a frame
 * takes those of the call in which its last sample arrives).  vp_xs_reset takes effect at the next process call and travels in its
 * arguments; a reset stream behaves like a fresh one, the others are untouched.  Per stream the handle keeps 12 KB of state: samples
 * received (int64), voice history, carrier history and overlap-add carry (1024 floats each).  Device memory is allocated at create only.
 * d_voice, d_carrier, d_out: device float [n_blocks][S][N]; d_depth: device double [S] or NULL = 1.  VP_ERR_INVALID_ARG (null pointer,
 * n_blocks <= 0, lifter outside 4 .. 64, stream out of range) is reported before the device is touched. */
typedef struct vp_xs vp_xs;
int vp_xs_create(int device, int n_streams, int block_size, int frame_len, int hop, vp_xs **out);
int vp_xs_destroy(vp_xs *x);
int vp_xs_get_latency(const vp_xs *x);                                  /* F - gcd(N, hop) */
int vp_xs_reset(vp_xs *x, int stream);                                  /* stream -1 = all; takes effect at the next call */
int vp_xs_process_blocks_device(vp_xs *x, const float *d_voice, const float *d_carrier, float *d_out, const double *d_depth, int lifter,
                                int n_blocks, void *hip_stream);
long vp_xs_debug_alloc_count(const vp_xs *x);                           /* constant across process calls; -1 on NULL */

/* Streaming harmonizer: vp_stft_harmonize driven block by block (kernel vp_k_hz_stream).  One handle holds S independent streams of
 * n_voices voices each (1 .. VP_HARM_MAX_VOICES, fixed at create), frame length 1024 (VP_ERR_GEOMETRY otherwise, also for a hop
 * vp_stft_supported(1024, hop) refuses), block size N >= 1 fixed at create.  Frame grid, latency L = F - gcd(N, hop) and call
 * bookkeeping are the streaming phase vocoder's: output sample t of a stream is sample t - L of the one-shot result on everything received
 * -- the dry part included, which therefore needs no delay line of the caller's --, the first L samples are 0, and the concatenated
 * outputs are BIT-IDENTICAL to vp_stft_harmonize over every sample emitted however the blocks are grouped into calls.  A frame takes the
 * ratios of the block in which its last sample arrives; gains and dry are the call's.  A reset takes effect at the next process call and
 * travels in its arguments; a reset stream behaves like a fresh one, the others are untouched.  Per stream the handle keeps 28 KB of
 * state: the previous frame's phases, samples received (int64), input history and overlap-add carry (1024 floats each) and four angle
 * arrays.  Device memory is allocated at create only.  It is a handle of its own: the streaming phase vocoder's record is not touched.
 * d_in, d_out: device float [n_blocks][S][N]; d_ratio: device double [n_blocks][S][n_voices]; d_gain: device double [S][n_voices] or
 * NULL = 1; d_dry: device double [S] or NULL = 0; values treated as in vp_stft_harmonize.  VP_ERR_INVALID_ARG (null handle, input,
 * output or ratio table, n_blocks <= 0, n_voices outside 1 .. 4 at create, stream out of range) is reported before the device is
 * touched. */
typedef struct vp_hz vp_hz;
int vp_hz_create(int device, int n_streams, int block_size, int frame_len, int hop, int n_voices, vp_hz **out);
int vp_hz_destroy(vp_hz *h);
int vp_hz_get_latency(const vp_hz *h);                                  /* F - gcd(N, hop) */
int vp_hz_reset(vp_hz *h, int stream);                                  /* stream -1 = all; takes effect at the next call */
int vp_hz_process_blocks_device(vp_hz *h, const float *d_in, float *d_out, const double *d_ratio, const double *d_gain, const double *d_dry,
                                int n_blocks, void *hip_stream);
long vp_hz_debug_alloc_count(const vp_hz *h);                           /* constant across process calls; -1 on NULL */

/* Streaming pitch tracker and automatic correction for the stream above (kernels vp_k_yin_track_stream and vp_k_track_follow,
 * csrc/vp_track.hip): vp_stft_track_pitch's decision once per block and stream, from the audio received so far, followed across unvoiced
 * blocks and over time -- the table vp_pv_process_blocks_curve_device takes.  The definition is tests/pv_track_stream_reference.py, and
 * period and ratio equal it bit for bit.  One handle holds S streams, block size N >= 1, the sample rate (8000 .. 51200) and an analysis
 * length F of 1024 or 2048 (VP_ERR_GEOMETRY otherwise) that is the tracker's own: the shifter's frame length does not enter.
 *  - tauMax = ceil(fs / 100), W = F + tauMax.  Per stream, x is everything received since create or the stream's last reset and
 *    n_b = (b + 1) N the count after block b.  n_b < W: period 0, raw ratio 1.0 (no zero-padded window is analysed).  Otherwise the raw
 *    decision is vp_stft_track_pitch's for the window x[n_b - W, n_b) taken as a row of W samples: causal, no added latency.
 *  - Follow stage, per stream (tgt = 1.0, age = 0, cur = 1.0), per handle hold_blocks H and glide g (defaults 0 and 1.0: the raw ratio):
 *      period > 0: tgt = raw ratio, age = 0;  else: age = min(age + 1, INT_MAX), and tgt = 1.0 once age > H;
 *      cur = tgt when g == 1.0, else cur + g * (tgt - cur) in double (product and add separate);  ratio[b][s] = cur.
 *  - How blocks are grouped into calls does not change a bit of either table.
 *  - vp_pv_tracker_reset(stream; -1 = all) takes effect at the next process call issued after it (a call already enqueued does not see
 *    it) and travels in the arguments of a launch in front of that call; the stream then equals a fresh handle's: no history, follow
 *    state (1.0, 0, 1.0).  vp_pv_tracker_set_follow applies to every stream from the next call on and travels as kernel arguments;
 *    0 <= hold_blocks <= 2^20 and 0 < glide <= 1 (VP_ERR_INVALID_ARG otherwise, also for a glide that is not finite).
 * d_in: device float [n_blocks][S][N], the slab the vp_pv_* calls take; d_key: device int [S] or NULL, as vp_stft_track_pitch's;
 * d_period: device int [n_blocks][S] or NULL; d_ratio: device double [n_blocks][S] or NULL; not both NULL.  The state advances whichever
 * outputs are given.  No allocation (device memory at create only: per stream a ring of its last W samples, about 6 KB at F = 1024, a
 * 64-bit sample counter and the follow state; vp_pv_tracker_debug_alloc_count stays constant), no synchronisation.  The cost of a decision
 * does not depend on N: N = 64 costs 16 times as much per second of audio as N = 1024.  VP_ERR_INVALID_ARG (null pointer, both outputs
 * NULL, n_blocks <= 0, sample rate, stream or follow parameter out of range) is reported before the device is touched. */
typedef struct vp_pv_tracker vp_pv_tracker;
int vp_pv_tracker_create(int device, int n_streams, int block_size, int frame_len, double sample_rate, vp_pv_tracker **out);
int vp_pv_tracker_destroy(vp_pv_tracker *t);
long vp_pv_tracker_debug_alloc_count(const vp_pv_tracker *t);            /* constant across process calls */
int vp_pv_tracker_reset(vp_pv_tracker *t, int stream);                  /* stream -1 = all */
int vp_pv_tracker_set_follow(vp_pv_tracker *t, int hold_blocks, double glide);
int vp_pv_tracker_process_blocks_device(vp_pv_tracker *t, const float *d_in, const int *d_key, int *d_period, double *d_ratio, int n_blocks,
                                        void *hip_stream);
/* vp_pv_tracker_process_blocks_device followed by vp_pv_process_blocks_curve_device along its table, on the same stream: the output has
 * the bits of those two calls.  d_ratio is required (result and scratch), d_period optional.  VP_ERR_GEOMETRY if S, N or the device
 * differ between the two handles.  vp_pv_reset does not reach the tracker and vp_pv_tracker_reset does not reach the shifter: a caller
 * that restarts a stream resets both. */
int vp_pv_autotune_blocks_device(vp_pv *p, vp_pv_tracker *t, const float *d_in, float *d_out, const int *d_key, int *d_period, double *d_ratio,
                                 int n_blocks, void *hip_stream);
/* vp_pv_tracker_process_blocks_device followed by vp_pv_process_blocks_formant_device along its table, on the same stream: the bits of
 * those two calls.  Arguments as vp_pv_autotune_blocks_device's plus d_formant and lifter. */
int vp_pv_autotune_blocks_formant_device(vp_pv *p, vp_pv_tracker *t, const float *d_in, float *d_out, const int *d_key, int *d_period,
                                         double *d_ratio, const double *d_formant, int lifter, int n_blocks, void *hip_stream);
/* The streaming tracker's KEY-AWARE VOICES (kernels vp_k_yin_track_voices_stream and vp_k_track_follow_voices): the raw decision of
 * vp_pv_tracker_process_blocks_device, vp_stft_track_harmony's voice stage on it, then the follow stage per voice -- the table
 * vp_hz_process_blocks_device takes.  The definition is tests/pv_harmkey_stream_reference.py; period and ratio equal it bit for bit.
 *   per (stream, voice) tgt = 1.0, cur = 1.0 and one age = 0 per stream; per block:
 *     period > 0: tgt[v] = raw[v], age = 0;  else: age = min(age + 1, INT_MAX), and tgt[v] = unvoiced[s][v] once age > H;
 *     cur[v] = tgt[v] when g == 1.0, else cur[v] + g * (tgt[v] - cur[v]);  ratio[b][s][v] = cur[v].
 * With every degree 0 and unvoiced 1.0 (or NULL) a voice's column is vp_pv_tracker_process_blocks_device's table, bit for bit.  Ring and
 * counter are the handle's: a block goes through exactly ONE of the two process calls.  The voices' follow state is separate from the
 * mono call's (each call advances its own and leaves the other's alone); vp_pv_tracker_reset clears both, vp_pv_tracker_set_follow
 * governs both.  It is allocated at create with everything else.  n_voices (1 .. VP_HARM_MAX_VOICES) may differ from call to call; the
 * voices a call does not name keep their state.  How blocks are grouped into calls does not change a bit.
 * d_degree: device int [S][n_voices], required; d_unvoiced: device double [S][n_voices] or NULL = 1.0 (a NaN or an infinity counts as
 * 1.0); d_period: device int [n_blocks][S] or NULL; d_ratio: device double [n_blocks][S][n_voices] or NULL; not both NULL.  Everything
 * else, and the errors (all VP_ERR_INVALID_ARG, before the device is touched), as vp_pv_tracker_process_blocks_device's. */
int vp_pv_tracker_process_blocks_voices_device(vp_pv_tracker *t, const float *d_in, const int *d_key, int n_voices, const int *d_degree,
                                               const double *d_unvoiced, int *d_period, double *d_ratio, int n_blocks, void *hip_stream);
/* vp_pv_tracker_process_blocks_voices_device with the harmonizer handle's voice count, followed by vp_hz_process_blocks_device along its
 * table, on the same stream: the output has the bits of those two calls.  d_ratio is required (result and scratch), d_period optional.
 * VP_ERR_GEOMETRY if S, N or the device differ between the two handles.  vp_hz_reset does not reach the tracker and vp_pv_tracker_reset
 * does not reach the harmonizer: a caller that restarts a stream resets both. */
int vp_hz_autoharm_blocks_device(vp_hz *h, vp_pv_tracker *t, const float *d_in, float *d_out, const int *d_key, const int *d_degree,
                                 const double *d_unvoiced, const double *d_gain, const double *d_dry, int *d_period, double *d_ratio,
                                 int n_blocks, void *hip_stream);
/* The streaming FINE tracker (kernels vp_k_yin_track_stream_fine and vp_k_yin_track_voices_stream_fine): the raw decision per block is
 * vp_stft_track_pitch_fine's for the same window, the follow stage is unchanged (it reads the int period only as the voiced flag).  The
 * definition is tests/pv_track_fine_stream_reference.py.  vp_pv_tracker_set_mode(VP_TRACK_INTEGER, the default, or VP_TRACK_FINE;
 * anything else VP_ERR_INVALID_ARG) selects the tracker of the five process calls above from the next call on; it touches no stream
 * state (ring, counters, follow state), so a stream may change mode between two calls.
 * vp_pv_tracker_process_blocks_fine_device is vp_pv_tracker_process_blocks_device with the fine tracker whatever the mode, and
 * d_period_fine: device double [n_blocks][S] or NULL, the refined period of the raw decision before the follow stage -- 0.0 on unvoiced
 * blocks and while the ring fills.  The checks are vp_pv_tracker_process_blocks_device's, unchanged: d_period and d_ratio may not both be
 * NULL (VP_ERR_INVALID_ARG), also when d_period_fine is given -- the refined period is an addition to the call's tables, not a third
 * alternative. */
int vp_pv_tracker_set_mode(vp_pv_tracker *t, int mode);
int vp_pv_tracker_get_mode(const vp_pv_tracker *t);                     /* the mode, or VP_ERR_INVALID_ARG on NULL */
int vp_pv_tracker_process_blocks_fine_device(vp_pv_tracker *t, const float *d_in, const int *d_key, int *d_period, double *d_period_fine,
                                             double *d_ratio, int n_blocks, void *hip_stream);

const char *vp_error_string(int code);
const char *vp_last_error(const vp_handle *h);
int vp_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VP_AMD_H */
