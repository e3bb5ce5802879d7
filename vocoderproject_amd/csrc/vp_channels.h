// vp_channels.h -- the channel-pointer pack kernels (csrc/vp_channels.hip): launchers.
// What an AudioBuffer<float> hands processBlock() is one pointer per channel (PluginProcessor.cpp:203; MyBuffer.cpp:74-105 reads them,
// null side-chain pointers included); the process plans take one packed slab.  These two kernels move between the forms.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#define VP_CH_THREADS 256               // one workgroup per (row, block): 256 lanes x 16 bytes = a 1024-sample block in one pass

// d_table[s * nIn + ch] -> d_packed [nBlocks][S][nIn][N]; block b of a row is its samples [sampleOffset + b N, sampleOffset + (b + 1) N).
// A null entry fills its rows of the slab with zeros.  Returns hipGetLastError().
hipError_t vp_channels_gather(const float *const *d_table, float *d_packed, int nIn, int S, int N, int nBlocks, size_t sampleOffset, hipStream_t st);
// d_packed [nBlocks][S][2][N] -> d_table[s * nOut + ch], ch < 2; channel 2 (nOut == 3) is filled with zeros; a null entry is skipped.
hipError_t vp_channels_scatter(const float *d_packed, float *const *d_table, int nOut, int S, int N, int nBlocks, size_t sampleOffset, hipStream_t st);
