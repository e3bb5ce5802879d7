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
