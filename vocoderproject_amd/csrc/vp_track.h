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

// enqueue vp_k_yin_track_stream (grid = ceil(S nBlocks / VP_TRACK_WAVES)), vp_k_track_follow (behind it on the same stream: it rewrites the
// ring the first one reads) and vp_k_track_reset; each returns hipGetLastError()
hipError_t vp_track_stream_launch(const VpTrackStreamArgs &a, hipStream_t st);
hipError_t vp_track_follow_launch(const VpTrackFollowArgs &a, hipStream_t st);
hipError_t vp_track_reset_launch(const VpTrackUpdArgs &a, hipStream_t st);
