// vp_stft.h -- the fused STFT round trip (csrc/vp_stft.hip): arguments and launcher.
// No reference counterpart (the reference has no FFT: SURVEY.md section 0); BASELINE.json's north_star names these kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#define VP_STFT_WAVES 4                 // wavefronts per workgroup = frames per round

struct VpStftArgs {
    const float *in;                    // [S][T]
    float *out;                         // [S][T]
    float *mag;                         // [S][nFrames][F/2 + 1] or nullptr
    const double *win;                  // [F] sqrt-Hann (periodic), analysis = synthesis
    const double *tw1;                  // [64][8][2]  W_64^(m0 (lane >> 3))            second step of the 512-point transform
    const double *tw2;                  // [64][8][2]  W_512^(a lane)                    third step
    const double *tws;                  // [64][NP][2] W_(2F)^... real-input split / merge: W_F^(64 q + lane), NP = F / 256 pairs per lane
    const double *twTop;                // [64][8][2]  W_1024^(64 q + lane): the radix-2 step on top of two 512-point transforms (F = 2048), else nullptr
    double pvRatio;                     // pitch ratio of the phase-vocoder stage
    double c;                           // scale / (F/2): overlap-add normalisation and the inverse transform's 1/N, folded into the merge
    int T, nFrames, nHops, nRounds;     // samples per stream; frames; hops of output (ceil(T / hop)); rounds of VP_STFT_WAVES frames
    int roundsPerRun, haloRounds;       // a workgroup owns roundsPerRun rounds of one stream (+ haloRounds recomputed in front)
    int F, hop, O;                      // frame, hop, overlap factor F / hop
    int aligned;                        // rows and hops 8-byte aligned: float2 loads
    int pv;                             // 1: phase-vocoder stage between the transforms (one workgroup per stream), 0: identity
    int f32;                            // 1: transform, split and merge in single precision (vp_k_stft_fused32 / vp_k_stft_fused2k32; no phase-vocoder stage)
};

size_t vp_stft_lds_bytes(int F, int hop, int f32 = 0);
// dynamic LDS of the 2048-point phase-vocoder build (vp_k_stft_pv2k) at this hop: slots, carry and the stage's arrays
size_t vp_stft_pv2k_lds_bytes(int hop);
// enqueues the fused kernel (grid = runs x streams); returns hipGetLastError()
hipError_t vp_stft_launch(const VpStftArgs &a, int nStreams, int nRuns, hipStream_t st);
int vp_stft_supported(int F, int hop);
// once per handle, on the handle's device (current device): the dynamic-LDS ceiling of the builds that need more than 64 KB
hipError_t vp_stft_prepare_device();
// the phase-vocoder builds that read the ratio per frame from d_ratio [nStreams][nFrames] (vp_k_stft_pv_curve / vp_k_stft_pv2k_curve, by
// a.F; csrc/vp_stft_curve.inc): one workgroup per stream, a.roundsPerRun = a.nRounds; and their dynamic-LDS ceiling, as above
hipError_t vp_stft_launch_curve(const VpStftArgs &a, const double *d_ratio, int nStreams, hipStream_t st);
hipError_t vp_stft_curve_prepare_device();
// the phase-vocoder builds that read frame f of stream s at input sample d_pos[s][f] (int32 [nStreams][nFrames], clamped to [0, nIn - F])
// of an input row of nIn samples and write it at output sample f hop of a row of a.T samples (vp_k_stft_pv_stretch /
// vp_k_stft_pv2k_stretch, by a.F; csrc/vp_stft_stretch.inc): one workgroup per stream, a.roundsPerRun = a.nRounds, a.aligned unused; and
// their dynamic-LDS ceiling, as above
hipError_t vp_stft_launch_stretch(const VpStftArgs &a, const int *d_pos, int nIn, int nStreams, hipStream_t st);
hipError_t vp_stft_stretch_prepare_device();
// the 1024-point ratio-curve build with the cepstral formant correction (vp_k_stft_pv_formant; csrc/vp_stft_formant.inc): d_ratio as in
// vp_stft_launch_curve, d_formant [nStreams] formant ratios or nullptr (1), nc the lifter length in samples (4 .. 64); a.F == 1024
hipError_t vp_stft_launch_formant(const VpStftArgs &a, const double *d_ratio, const double *d_formant, int nc, int nStreams, hipStream_t st);
hipError_t vp_stft_formant_prepare_device();
// the 1024-point ratio-curve build with peak locking (vp_k_stft_pv_lock; csrc/vp_stft_lock.inc): d_ratio as in vp_stft_launch_curve;
// a.F == 1024.  Its dynamic LDS at this hop: the curve build's plus the masks, owners and map of the locked stage
hipError_t vp_stft_launch_lock(const VpStftArgs &a, const double *d_ratio, int nStreams, hipStream_t st);
hipError_t vp_stft_lock_prepare_device();
size_t vp_stft_lock_lds_bytes(int hop);
// the peak-locked build with sub-bin region offsets (vp_k_stft_pv_lockf; csrc/vp_stft_lockf.inc): arguments and dynamic LDS as
// vp_stft_launch_lock's (the offsets lie in free slots of the locked stage's rows)
hipError_t vp_stft_launch_lockf(const VpStftArgs &a, const double *d_ratio, int nStreams, hipStream_t st);
hipError_t vp_stft_lockf_prepare_device();
size_t vp_stft_lockf_lds_bytes(int hop);
// the peak-locked build with frames at given positions (vp_k_stft_pv_stretch_lock; csrc/vp_stft_stretch_lock.inc): d_ratio as in
// vp_stft_launch_lock, d_pos and nIn as in vp_stft_launch_stretch; a.F == 1024.  Its dynamic LDS is vp_stft_lock_lds_bytes(a.hop)
hipError_t vp_stft_launch_stretch_lock(const VpStftArgs &a, const double *d_ratio, const int *d_pos, int nIn, int nStreams, hipStream_t st);
hipError_t vp_stft_stretch_lock_prepare_device();
// the 1024-point cross-synthesis build (vp_k_stft_cross; csrc/vp_stft_cross.inc): a.in is the carrier, d_voice [nStreams][a.T] the signal whose
// spectral envelope it takes, d_depth [nStreams] or nullptr (1), nc the lifter length (4 .. 64); grid = nRuns x nStreams as vp_stft_launch,
// always double, dynamic LDS vp_stft_lds_bytes(1024, hop) (under 64 KB: no ceiling to raise); a.F == 1024
hipError_t vp_stft_launch_cross(const VpStftArgs &a, const float *d_voice, const double *d_depth, int nc, int nStreams, int nRuns, hipStream_t st);

// ---- streaming phase vocoder (vp_pv_*): one workgroup per stream and call, state in HBM between calls -----------------------------
#define VP_PV_MAX_UPDATES 16            // interval changes / resets carried in a process call's arguments
#define VP_PV_RING 4096                 // overlap-add ring in LDS (floats): the carry plus one round's frames at hop <= 512
// one stream's state, VP_PV_REC_BYTES each: previous-frame phases [513] | synthesis accumulator [513] | ratio | samples received (int64)
// (doubles) | input history [F] | overlap-add carry [F] (floats)
#define VP_PV_NB 513
#define VP_PV_RATIO (2 * VP_PV_NB)
#define VP_PV_COUNT (2 * VP_PV_NB + 1)
#define VP_PV_HIST_BYTES ((2 * VP_PV_NB + 2) * 8)
#define VP_PV_CARRY_BYTES (VP_PV_HIST_BYTES + 1024 * 4)
#define VP_PV_REC_BYTES (VP_PV_CARRY_BYTES + 1024 * 4)

struct VpPvUpdate {
    int stream;                         // -1: every stream
    int reset;                          // 1: the stream's signal state restarts (its interval stays)
    double ratio;                       // > 0: the new pitch ratio; 0: unchanged
};

struct VpPvArgs {
    const float *in;                    // [nBlocks][S][N]
    float *out;                         // [nBlocks][S][N]
    unsigned char *state;               // [S][VP_PV_REC_BYTES]
    const double *win, *tw1, *tw2, *tws;   // the one-shot's tables (VpStftArgs)
    double c;                           // the one-shot's normalisation
    int S, N, nBlocks, hop, O, L;       // streams, block, blocks in this call, hop, F / hop, latency F - gcd(N, hop)
    int nUpd;
    VpPvUpdate upd[VP_PV_MAX_UPDATES];
};

size_t vp_pv_lds_bytes();
// the streaming kernel (grid = S workgroups); nBlocks = 0 launches the small kernel that only applies the updates
hipError_t vp_pv_launch(const VpPvArgs &a, hipStream_t st);
hipError_t vp_pv_prepare_device();
// the streaming kernel with one ratio per block and stream, d_ratio [a.nBlocks][a.S] (vp_k_pv_stream_curve; a.nBlocks > 0)
hipError_t vp_pv_launch_curve(const VpPvArgs &a, const double *d_ratio, hipStream_t st);
hipError_t vp_pv_curve_prepare_device();
// ... and with the cepstral formant correction (vp_k_pv_stream_formant): d_formant [a.S] or nullptr (1), nc the lifter length (4 .. 64)
hipError_t vp_pv_launch_formant(const VpPvArgs &a, const double *d_ratio, const double *d_formant, int nc, hipStream_t st);
hipError_t vp_pv_formant_prepare_device();
// the curve call with peak locking (vp_k_pv_stream_lock): theta in the record's accumulator array, the record unchanged
hipError_t vp_pv_launch_lock(const VpPvArgs &a, const double *d_ratio, hipStream_t st);
hipError_t vp_pv_lock_prepare_device();
size_t vp_pv_lock_lds_bytes();
// ... and with sub-bin region offsets (vp_k_pv_stream_lockf): state, record and LDS as the locked call's
hipError_t vp_pv_launch_lockf(const VpPvArgs &a, const double *d_ratio, hipStream_t st);
hipError_t vp_pv_lockf_prepare_device();
size_t vp_pv_lockf_lds_bytes();

// ---- streaming cross-synthesis (vp_xs_*): vp_k_pv_stream's bookkeeping with two inputs and no phases (csrc/vp_stft_cross.inc) ------------
// one stream's state, VP_XS_REC_BYTES each: samples received (int64) | voice history [1024] | carrier history [1024] | overlap-add carry
// [1024] (floats)
#define VP_XS_VOICE_BYTES 8
#define VP_XS_CARRIER_BYTES (VP_XS_VOICE_BYTES + 1024 * 4)
#define VP_XS_CARRY_BYTES (VP_XS_CARRIER_BYTES + 1024 * 4)
#define VP_XS_REC_BYTES (VP_XS_CARRY_BYTES + 1024 * 4)

struct VpXsArgs {
    const float *voice, *carrier;       // [nBlocks][S][N]
    float *out;                         // [nBlocks][S][N]
    unsigned char *state;               // [S][VP_XS_REC_BYTES]
    const double *win, *tw1, *tw2, *tws;   // the one-shot's tables (VpStftArgs)
    const double *depth;                // [S] or nullptr (1)
    double c;                           // the one-shot's normalisation
    int S, N, nBlocks, hop, L, nc;      // streams, block, blocks in this call, hop, latency F - gcd(N, hop), lifter length
    int nUpd;
    VpPvUpdate upd[VP_PV_MAX_UPDATES];  // pending resets (ratio 0)
};

size_t vp_xs_lds_bytes();
// the streaming kernel (grid = S workgroups); nBlocks = 0 launches the small kernel that only applies the resets
hipError_t vp_xs_launch(const VpXsArgs &a, hipStream_t st);

// ---- the harmonizer (vp_stft_harmonize, vp_hz_*; csrc/vp_stft_harm.inc): V peak-locked voices and the dry signal from one analysis --------
#define VP_HARM_MAX_VOICES 4
// the one-shot build (vp_k_stft_harm): d_ratio [nStreams][nVoices][a.nFrames], d_gain [nStreams][nVoices] or nullptr (1), d_dry [nStreams] or
// nullptr (0); one workgroup per stream, a.F == 1024.  Its dynamic LDS at this hop: the locked build's plus three more angle arrays
hipError_t vp_stft_launch_harm(const VpStftArgs &a, const double *d_ratio, const double *d_gain, const double *d_dry, int nVoices, int nStreams, hipStream_t st);
hipError_t vp_stft_harm_prepare_device();
size_t vp_stft_harm_lds_bytes(int hop);
// one stream's state of the streaming build, VP_HZ_REC_BYTES each: previous-frame phases [513] | samples received (int64) (doubles) |
// input history [1024] | overlap-add carry [1024] (floats) | theta [VP_HARM_MAX_VOICES][513] (doubles)
#define VP_HZ_COUNT VP_PV_NB
#define VP_HZ_HIST_BYTES ((VP_PV_NB + 1) * 8)
#define VP_HZ_CARRY_BYTES (VP_HZ_HIST_BYTES + 1024 * 4)
#define VP_HZ_THETA_BYTES (VP_HZ_CARRY_BYTES + 1024 * 4)
#define VP_HZ_REC_BYTES (VP_HZ_THETA_BYTES + VP_HARM_MAX_VOICES * VP_PV_NB * 8)
// the streaming kernel (vp_k_hz_stream; grid = a.S workgroups): a.state holds VP_HZ records, a.upd resets only; d_ratio [a.nBlocks][a.S][nVoices],
// d_gain and d_dry as above; a.nBlocks = 0 launches the small kernel that only applies the resets
hipError_t vp_hz_launch(const VpPvArgs &a, const double *d_ratio, const double *d_gain, const double *d_dry, int nVoices, hipStream_t st);
hipError_t vp_hz_prepare_device();
size_t vp_hz_lds_bytes();

// ---- the transient-preserving locked time stretch (vp_stft_onset_flux, vp_stft_time_stretch_locked_reset) ---------------------------------
// the onset flux (vp_k_stft_onset_flux; csrc/vp_stft_onset.inc): a.in rows of nIn samples, d_flux and d_mass double [nStreams][nG],
// nG = (nIn - a.F) / a.hop + 1; grid = chunks of vp_stft_onset_chunk(nG, nStreams) consecutive frames x streams; a.F == 1024
hipError_t vp_stft_launch_onset(const VpStftArgs &a, int nIn, int nStreams, double *d_flux, double *d_mass, hipStream_t st);
hipError_t vp_stft_onset_prepare_device();
size_t vp_stft_onset_lds_bytes();
int vp_stft_onset_chunk(int nG, int nStreams);
// the locked time stretch with a phase reset on the frames d_reset [nStreams][a.nFrames] flags, any non-zero byte
// (vp_k_stft_pv_stretch_lock_reset; csrc/vp_stft_stretch_reset.inc): everything else as vp_stft_launch_stretch_lock, its dynamic LDS too
hipError_t vp_stft_launch_stretch_lock_reset(const VpStftArgs &a, const double *d_ratio, const int *d_pos, int nIn, const unsigned char *d_reset, int nStreams,
                                             hipStream_t st);
hipError_t vp_stft_stretch_reset_prepare_device();
