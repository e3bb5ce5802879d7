// vp_channels.hip -- pointer table <-> packed slab, for the channel-pointer entry points (vp_process_block_channels*, vp_amd.h).
//
// The reference's MyBuffer::fillInputBuffers (MyBuffer.cpp:74-105) reads one pointer per channel and takes null side-chain
// pointers as silence (:93-102); fillOutputBuffer writes one pointer per channel behind buffer.clear() (:115).  The process plans
// of this library read and write packed slabs, so a channel call is: gather -> the plan, unchanged -> scatter.
//
// Mapping: one workgroup per (row, block).  The row pointer is the same for the whole workgroup: it is read once through a
// wave-uniform address and kept in scalar registers, and so is everything decided from it -- null (zero fill / skip) and the
// access width.  16-byte accesses need the row address, the slab offset and the block length to allow them; a row one float
// into its allocation or an odd N takes the dword loop.  The choice is per row, by a uniform branch: no lane of a wavefront
// ever takes a different loop from its neighbours.  Samples travel as bit patterns (no float instruction touches them: the
// build's denormal mode must not flush what the packed entry points would have read as it is).
#include "vp_channels.h"

#include <stdint.h>

// a value every lane holds alike, made provably so: the branches on it compile to scalar branches
__device__ static inline uintptr_t ch_uniform(uintptr_t v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(v & 0xffffffffu));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((uintptr_t)hi << 32) | lo;
}

// rows are device memory whatever the table says about them: global address space, so that the copies are global_load / global_store
// and not the flat forms a pointer rebuilt from an integer would get
typedef __attribute__((address_space(1))) unsigned ch_u32;
typedef unsigned ch_v4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) ch_v4 ch_u128;

// n dwords from src (0: zeros) to dst, both byte addresses; the caller's arguments are workgroup-uniform
__device__ static inline void ch_copy_row(uintptr_t dst, uintptr_t src, int n)
{
    const bool wide = (((dst | src) & 15) == 0) && (n & 3) == 0;
    if (wide) {
        ch_u128 *d4 = (ch_u128 *)dst;
        const ch_u128 *s4 = (const ch_u128 *)src;
        const int n4 = n >> 2;
        if (src) for (int i = threadIdx.x; i < n4; i += VP_CH_THREADS) d4[i] = s4[i];
        else for (int i = threadIdx.x; i < n4; i += VP_CH_THREADS) d4[i] = ch_v4{0u, 0u, 0u, 0u};
    } else {
        ch_u32 *d1 = (ch_u32 *)dst;
        const ch_u32 *s1 = (const ch_u32 *)src;
        if (src) for (int i = threadIdx.x; i < n; i += VP_CH_THREADS) d1[i] = s1[i];
        else for (int i = threadIdx.x; i < n; i += VP_CH_THREADS) d1[i] = 0u;
    }
}

// grid (S * nIn, nBlocks).  packed [nBlocks][S][nIn][N]
__global__ __launch_bounds__(VP_CH_THREADS) void vp_k_gather_channels(const float *const *__restrict__ table, float *packed, int nIn, int S, int N,
                                                                      int nBlocks, size_t sampleOffset)
{
    const int row = blockIdx.x, b = blockIdx.y;
    if (row >= S * nIn || b >= nBlocks) return;
    uintptr_t src = ch_uniform((uintptr_t)table[row]);
    if (src) src += (sampleOffset + (size_t)b * N) * sizeof(float);
    const uintptr_t dst = (uintptr_t)(packed + ((size_t)b * S * nIn + row) * N);
    ch_copy_row(dst, src, N);
}

// grid (S * nOut, nBlocks).  packed [nBlocks][S][2][N]; channel 2 of the table receives zeros (MyBuffer.cpp:115)
__global__ __launch_bounds__(VP_CH_THREADS) void vp_k_scatter_channels(const float *packed, float *const *__restrict__ table, int nOut, int S, int N,
                                                                       int nBlocks, size_t sampleOffset)
{
    const int row = blockIdx.x, b = blockIdx.y;
    if (row >= S * nOut || b >= nBlocks) return;
    uintptr_t dst = ch_uniform((uintptr_t)table[row]);
    if (!dst) return;                                                         // the caller does not want this channel
    dst += (sampleOffset + (size_t)b * N) * sizeof(float);
    const int s = row / nOut, ch = row - s * nOut;
    const uintptr_t src = ch < 2 ? (uintptr_t)(packed + (((size_t)b * S + s) * 2 + ch) * N) : 0;
    ch_copy_row(dst, src, N);
}

hipError_t vp_channels_gather(const float *const *d_table, float *d_packed, int nIn, int S, int N, int nBlocks, size_t sampleOffset, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_gather_channels, dim3((unsigned)(S * nIn), (unsigned)nBlocks), dim3(VP_CH_THREADS), 0, st, d_table, d_packed, nIn, S, N,
                       nBlocks, sampleOffset);
    return hipGetLastError();
}

hipError_t vp_channels_scatter(const float *d_packed, float *const *d_table, int nOut, int S, int N, int nBlocks, size_t sampleOffset, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_scatter_channels, dim3((unsigned)(S * nOut), (unsigned)nBlocks), dim3(VP_CH_THREADS), 0, st, d_packed, d_table, nOut, S, N,
                       nBlocks, sampleOffset);
    return hipGetLastError();
}
