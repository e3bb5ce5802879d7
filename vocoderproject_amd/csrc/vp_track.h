// vp_track.h -- the batch pitch tracker of the phase-vocoder path (csrc/vp_track.hip): arguments and launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#define VP_TRACK_WAVES 4                // wavefronts per workgroup = frames per workgroup
#define VP_TRACK_FMIN 100.0             // PluginProcessor.cpp:148
#define VP_TRACK_FMAX 800.0
#define VP_TRACK_LAGS 8                 // consecutive lags per lane: 64 x 8 = 512 >= tauMax

struct VpTrackArgs {
    const float *in;                    // [S][T]
    const int *key;                     // [S] or nullptr (chromatic); values outside 0..12 count as 12
    int *period;                        // [S][nFrames] or nullptr
    double *ratio;                      // [S][nFrames] or nullptr
    const double *notes;                // [13][VP_NOTES_STRIDE] (Notes::buildFreqVect per key, the popped element behind each table)
    const int *notesN;                  // [13]
    double fs;
    int S, T, F, hop, nFrames;
    int tauMax, tau0;                   // ceil(fs / fMin) <= 512, floor(fs / fMax)
};

// dynamic LDS of a workgroup at frame length F
size_t vp_track_lds_bytes(int F);
// enqueues vp_k_yin_track (grid = ceil(S nFrames / VP_TRACK_WAVES)); returns hipGetLastError()
hipError_t vp_track_launch(const VpTrackArgs &a, hipStream_t st);

// ---- the streaming tracker (vp_pv_tracker_*): the same decision per block and stream, from the last F + tauMax samples received ----------
#define VP_TRKS_GROUP 16                // streams per workgroup of the follow kernel
#define VP_TRKS_MAX_UPDATES 16          // resets per update launch

struct VpTrackStreamArgs {
    const float *in;                    // [nBlocks][S][N] the call's slab
    const int *key;                     // as VpTrackArgs
    int *period;                        // [nBlocks][S] raw decisions (never null: the handle lends scratch)
    double *ratio;                      // [nBlocks][S]
    const double *notes;
    const int *notesN;
    const float *ring;                  // [S][F + tauMax]: sample i of a stream (counted from its last reset) at slot i % (F + tauMax)
    const long long *count;             // [S] samples received before this call
    double fs;
    int S, N, F, nBlocks;
    int tauMax, tau0;
};

struct VpTrackFollowArgs {
    const float *in;                    // the same slab
    const int *period;                  // [nBlocks][S] raw
    double *ratio;                      // [nBlocks][S] raw in, followed out
    float *ring;
    long long *count;
    double *tgt, *cur;                  // [S] the follow state
    int *age;                           // [S]
    double glide;
    int hold;
    int S, N, W, nBlocks;
};

struct VpTrackUpdArgs {
    long long *count;
    double *tgt, *cur;
    int *age;
    int S, n;
    int stream[VP_TRKS_MAX_UPDATES];    // -1: every stream
};

// ---- key-aware voices (vp_stft_track_harmony, vp_pv_tracker_process_blocks_voices_device): the same decision, then V in-key ratios -----
#define VP_TRACK_MAX_VOICES 4           // = VP_HARM_MAX_VOICES (include/vp_amd.h; vp_capi.hip asserts it)
#define VP_TRACK_HARM_FMIN 25.0         // the harmony tables: the tracker's recurrence through a wider filter, so that the tracker's table
#define VP_TRACK_HARM_FMAX 3200.0       // is a slice of the key's harmony table and twelve steps either side of it exist (or clamp at 0)
#define VP_TRACK_MAX_DEGREE 12

struct VpTrackVoices {
    const double *harm;                 // [13][VP_NOTES_STRIDE] the harmony table per key
    const int *harmOff;                 // [13] index of the tracker table's entry 0 in the harmony table.  Where the host builds the tables
                                        // it checks off + n + 12 <= hN - 1 (hN: the harmony table's entries): no index leaves a table upwards
    const int *degree;                  // [S][V] steps of the key's table, clamped to -12 .. 12 by the kernel
    const double *unvoiced;             // [S][V] the ratio of an unvoiced frame, or nullptr (1.0); a NaN or an infinity counts as 1.0
    int V;                              // 1 .. VP_TRACK_MAX_VOICES
};

struct VpTrackFollowVoicesArgs {
    const float *in;                    // as VpTrackFollowArgs
    const int *period;                  // [nBlocks][S] raw
    double *ratio;                      // [nBlocks][S][V] raw in, followed out
    const double *unvoiced;             // [S][V] or nullptr: the target once the hold has run out
    float *ring;
    long long *count;
    double *tgt, *cur;                  // [S][VP_TRACK_MAX_VOICES] the voices' follow state (the mono state is VpTrackFollowArgs')
    int *age;                           // [S] one age per stream, shared by its voices
    double glide;
    int hold;
    int S, N, W, nBlocks, V;
};

// enqueue vp_k_yin_track_voices (period [S][nFrames] or nullptr, ratio [S][V][nFrames] or nullptr) and vp_k_yin_track_voices_stream
// (period [nBlocks][S], ratio [nBlocks][S][V], neither null), grids as their parents'; vp_k_track_follow_voices behind the latter;
// vp_k_track_reset_voices clears the voices' follow state of the streams an update names (a.count is not read, a.tgt / a.cur are
// [S][VP_TRACK_MAX_VOICES]).  Each returns hipGetLastError()
hipError_t vp_track_voices_launch(const VpTrackArgs &a, const VpTrackVoices &v, hipStream_t st);
hipError_t vp_track_voices_stream_launch(const VpTrackStreamArgs &a, const VpTrackVoices &v, hipStream_t st);
hipError_t vp_track_follow_voices_launch(const VpTrackFollowVoicesArgs &a, hipStream_t st);
hipError_t vp_track_reset_voices_launch(const VpTrackUpdArgs &a, hipStream_t st);

// enqueue vp_k_yin_track_stream (grid = ceil(S nBlocks / VP_TRACK_WAVES)), vp_k_track_follow (behind it on the same stream: it rewrites the
// ring the first one reads) and vp_k_track_reset; each returns hipGetLastError()
hipError_t vp_track_stream_launch(const VpTrackStreamArgs &a, hipStream_t st);
hipError_t vp_track_follow_launch(const VpTrackFollowArgs &a, hipStream_t st);
hipError_t vp_track_reset_launch(const VpTrackUpdArgs &a, hipStream_t st);

// ---- fine (sub-sample) trackers (csrc/vp_track_fine_kernels.inc): the same decisions, the period refined by a parabola through the
// normalised function's minimum and the note looked up on the refined pitch.  Arguments, grids and LDS as the integer launchers';
// periodFine ([S][nFrames] for the batch kernel, [nBlocks][S] for the streaming one) receives the refined period, or is nullptr.  The
// streaming launches are followed by vp_track_follow_launch / vp_track_follow_voices_launch as the integer ones are
hipError_t vp_track_fine_launch(const VpTrackArgs &a, double *periodFine, hipStream_t st);
hipError_t vp_track_voices_fine_launch(const VpTrackArgs &a, const VpTrackVoices &v, hipStream_t st);
hipError_t vp_track_stream_fine_launch(const VpTrackStreamArgs &a, double *periodFine, hipStream_t st);
hipError_t vp_track_voices_stream_fine_launch(const VpTrackStreamArgs &a, const VpTrackVoices &v, hipStream_t st);
