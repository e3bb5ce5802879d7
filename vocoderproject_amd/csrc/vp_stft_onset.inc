// vp_stft_onset.inc -- the ONSET FLUX of the input's own frame grid: the transient-preserving stretch's first half (included by vp_stft.hip
// behind the phase-vocoder kernels and in front of vp_stft_stretch_reset.inc, the second half: the handle's window and twiddles, fft512_rx, rfft_split, stft_load_frame).
//
// The definition is tests/pv_transient_reference.py onset_flux: over the grid g hop of a row of nIn samples, nG = (nIn - F) / hop + 1,
//   M_g = |rfft(x[g hop : g hop + F] w)|, bins 0 .. 512;   mass[g] = sum_k M_g[k];
//   flux[0] = 0,  flux[g] = sum_k max(M_g[k] - M_(g-1)[k], 0)       (the rectified spectral flux).
// The host picks the onsets from the two tables (vp_onset_pick) and plans the positions around them (vp_stretch_positions_transient).
//
// Shape: one frame per wavefront, as everywhere here.  Frames are independent -- there is no recurrence over a stream -- so the grid is
// (chunks of consecutive frames, streams), sized to fill the chip.  In a round the workgroup's wavefronts take consecutive frames and hand
// their 513 magnitudes to the next through LDS (slot w + 1: wavefront w's frame of this round; slot 0: the last frame of the round before).
// A chunk that does not start the row computes its first frame's predecessor ITSELF, as one more frame in front with its stores
// suppressed: one code path for every frame, so a frame's figures do not depend on the partition (tested: a row beside others has the bits
// of the row alone).  Chunks hold NWV m - 1 frames, so that predecessor and frames fill whole rounds.
// Sums in a fixed order: the lane's nine bins in index order (64 q + lane upwards, lane 0's bin 256, the mirrors 512 - 64 q - lane
// upwards), then one butterfly tree over the lanes (xor 32, 16, 8, 4, 2, 1).  A NaN stays a NaN through the rectifier, as numpy.maximum
// keeps it.  Rows have nIn samples: with an odd nIn the odd rows are 4-byte aligned only, and a frame takes float2 loads when ITS first
// sample is 8-byte aligned, as in vp_k_stft_pv_stretch.
//
// LDS (dynamic): the wavefronts' exchange buffers, then (NWV + 1) rows of 513 magnitudes: 53 KB.
// Out of scope: 2048-point frames, single precision, picking on the device.
#define VP_ONSET_CHUNK_MIN (4 * NWV - 1)                                       // frames of the shortest chunk
__host__ __device__ constexpr size_t onset_lds_bytes() { return (size_t)NWV * 8192 + (size_t)(NWV + 1) * VP_PV_NB * sizeof(double); }
size_t vp_stft_onset_lds_bytes() { return onset_lds_bytes(); }

// the sum over the wavefront's lanes by one fixed tree; every lane gets it
__device__ __forceinline__ double onset_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64 * NWV) void vp_k_stft_onset_flux(VpStftArgs A, int nIn, int nG, int chunk, double *flux, double *mass)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y;
    constexpr int N = 512, nb = N + 1;                                         // complex points = F / 2; bins
    const int hop = A.hop;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f64 *mags = (lds_f64 *)smem + NWV * 1024;                              // [NWV + 1][nb]
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)(onset_lds_bytes() / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
    __syncthreads();
#endif

    FftLane L;
    fft_lane_init(L, lane, A.tw1, A.tw2);
    d2 wa[8];                                                                  // (w[2n], w[2n + 1]), n = lane + 64 r
    d2 ws[4];                                                                  // W_1024^(64 q + lane)
#pragma unroll
    for (int r = 0; r < 8; r++) wa[r] = ((const d2 *)A.win)[lane + 64 * r];
#pragma unroll
    for (int q = 0; q < 4; q++) ws[q] = ((const d2 *)A.tws)[lane * 4 + q];
    const bool lane0 = lane == 0;

    // the chunk's frames [g0, g1) and, unless it starts the row, the predecessor of its first in front of them
    const int g0 = blockIdx.x * chunk, g1 = min(g0 + chunk, nG);
    const int gs = g0 > 0 ? g0 - 1 : 0;
    const int nRounds = (g1 - gs + NWV - 1) / NWV;
    const float *xs = A.in + (size_t)s * nIn;
    double *fl = flux + (size_t)s * nG, *ms = mass + (size_t)s * nG;
    // the frame's samples are requested a round ahead
    f2 xv[8];
    auto request = [&](int rd_) {
        const int g_ = gs + rd_ * NWV + wv;
        if (rd_ < nRounds && g_ < g1) {
            const float *x_ = xs + (size_t)g_ * hop;                           // in [xs, xs + nIn - F]: g_ < nG
            stft_load_frame(xv, x_, ((uintptr_t)x_ & 7) == 0, lane);
        }
    };
    request(0);
    for (int rd = 0; rd < nRounds; rd++) {
        const int g = gs + rd * NWV + wv;
        const bool live = g < g1;                                              // (wavefront-uniform)
        C8 z;
        RPairs X;
        double m[9];                                                           // the lane's magnitudes: 2 q the pair's k = 64 q + lane, 2 q + 1 its mirror, 8 bin 256
#pragma unroll
        for (int e = 0; e < 9; e++) m[e] = 0.0;
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; r++) { z.re[r] = (double)xv[r].x * wa[r].x; z.im[r] = (double)xv[r].y * wa[r].y; }
        }
        request(rd + 1);
        if (live) {
            fft512_rx(z, xb, L);
            rfft_split(z, xb, lane, (const d2 *)ws, X);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = 64 * q + lane;
                m[2 * q] = sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]);
                m[2 * q + 1] = sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]);
                mags[(wv + 1) * nb + k] = m[2 * q]; mags[(wv + 1) * nb + N - k] = m[2 * q + 1];
            }
            m[8] = lane0 ? sqrt(X.hr * X.hr + X.hi * X.hi) : 0.0;
            if (lane0) mags[(wv + 1) * nb + N / 2] = m[8];
        }
        __syncthreads();
        if (live && g >= g0) {                                                 // (the predecessor in front of the chunk stores nothing)
            // the lane's bins in index order: 64 q + lane upwards, bin 256 (lane 0), the mirrors 512 - 64 q - lane upwards (q = 3 .. 0)
            double sm = 0.0, sf = 0.0;
            const lds_f64 *prev = mags + wv * nb;                              // frame g - 1: the wavefront below, or slot 0
#pragma unroll
            for (int i = 0; i < 9; i++) {
                const int e = i < 4 ? 2 * i : i == 4 ? 8 : 2 * (8 - i) + 1;
                if (e == 8 && !lane0) continue;
                const int k = e == 8 ? N / 2 : (e & 1) ? N - (64 * (e >> 1) + lane) : 64 * (e >> 1) + lane;
                sm += m[e];
                if (g > 0) {
                    const double d = m[e] - prev[k];
                    sf += d < 0.0 ? 0.0 : d;                                   // (a NaN stays: numpy.maximum's rule)
                }
            }
            sm = onset_wave_sum(sm);
            sf = onset_wave_sum(sf);
            if (lane0) { ms[g] = sm; fl[g] = sf; }
        }
        __syncthreads();                                                       // (every wavefront has read its predecessor's row)
        if (live && wv == NWV - 1) {
            // the round's last frame is the next round's predecessor (a round with fewer live wavefronts is the chunk's last)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = 64 * q + lane;
                mags[k] = m[2 * q]; mags[N - k] = m[2 * q + 1];
            }
            if (lane0) mags[N / 2] = m[8];
        }
    }
}

hipError_t vp_stft_onset_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_stft_onset_flux, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

// frames per chunk: enough chunks for two workgroups per compute unit, chunks of NWV m - 1 frames and at least VP_ONSET_CHUNK_MIN
int vp_stft_onset_chunk(int nG, int nStreams)
{
    const int want = (2 * 256 + nStreams - 1) / nStreams;                      // chunks per stream
    const int per = (nG + want - 1) / want;                                    // frames per chunk for that many
    const int c = (per + 1 + NWV - 1) / NWV * NWV - 1;
    return c < VP_ONSET_CHUNK_MIN ? VP_ONSET_CHUNK_MIN : c;
}

hipError_t vp_stft_launch_onset(const VpStftArgs &a, int nIn, int nStreams, double *d_flux, double *d_mass, hipStream_t st)
{
    const int nG = (nIn - a.F) / a.hop + 1;
    const int chunk = vp_stft_onset_chunk(nG, nStreams);
    const dim3 grid((nG + chunk - 1) / chunk, nStreams), block(64 * NWV);
    hipLaunchKernelGGL(vp_k_stft_onset_flux, grid, block, onset_lds_bytes(), st, a, nIn, nG, chunk, d_flux, d_mass);
    return hipGetLastError();
}
