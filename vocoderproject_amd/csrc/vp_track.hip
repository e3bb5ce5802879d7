// vp_track.hip -- batch pitch tracker for the phase-vocoder path: YIN per STFT frame, the key's nearest note, one ratio per frame.
//
// The definition is tests/pv_track_reference.py: PitchProcess's own decision (computeYinTemp, PitchProcess.cpp:350-403; the
// threshold walk, :429-447; beta = closestFreq / pitch, :595-596) with the plugin's numbers (fMin 100, fMax 800, yinTol 0.25, the
// Notes tables), applied to every frame of a vp_stft handle on its own: frame f of a row of T samples reads the F + tauMax samples
// from b = min(f hop, T - (F + tauMax)) on.  The sums are the reference's, operation by operation (this translation unit is built
// with -ffp-contract=off): d[k] is its own left-to-right sum over i of (x[i] - x[i + k])^2 in double, the normalisation runs in
// increasing k, so period and ratio equal the CPU oracle's bit for bit.  Input samples that are float32 denormals are outside the
// tested domain: the library's default build (-fdenormal-fp-math=preserve-sign) widens them to 0.0, the oracle does not.
//
// One wavefront per frame, VP_TRACK_WAVES frames per workgroup, no workgroup barrier: every wavefront works in its own slice of LDS.
//   * the frame's samples are staged once as floats (widening is exact), eight samples to nine words: lane l reads x[i + 8 l + j], a
//     stride of eight words would put 32 lanes on four banks, nine words put them on 32;
//   * lane l owns the lags 8 l .. 8 l + 7.  Per eight steps of i it reads the next eight samples of its window (eight 4-byte reads) and
//     the eight x[i] every lane shares (broadcast reads), then runs 8 x 8 (subtract, multiply, add) on registers: 192 fp64
//     operations to 16 LDS reads;
//   * the running sum of the normalisation is serial by definition: lane after lane adds its eight sums to a carry handed on by
//     v_readlane;
//   * the walk runs on ballots over the normalised function read back lag-per-lane: the first lag under the tolerance is a
//     count of trailing zeros, the descent stops at the first lag whose successor is not smaller;
//   * the note table of the stream's key sits in two registers per lane (requested before the sums, so the round trip is over
//     when it is needed); std::lower_bound on it is a population count.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "vp_common.h"
#include "vp_track.h"

#define TRK_ROW 9                       // words per eight staged samples
#define TRK_MAXLAG (64 * VP_TRACK_LAGS)

typedef __attribute__((address_space(3))) float trk_lds_f32;
typedef __attribute__((address_space(3))) double trk_lds_f64;

__device__ __forceinline__ void trk_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// lane `l` (uniform) of v to every lane
__device__ __forceinline__ double trk_readlane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// bytes of one wavefront's slice: F / 8 + 64 rows of staged samples (lane 63 reads 64 rows past the frame's last); the
// normalised function (TRK_MAXLAG + 1 doubles) takes the same bytes once the sums are done
__host__ __device__ static inline int trk_wave_bytes(int F) { return (F / 8 + 64) * TRK_ROW * 4; }

size_t vp_track_lds_bytes(int F) { return (size_t)VP_TRACK_WAVES * trk_wave_bytes(F); }

__global__ __launch_bounds__(64 * VP_TRACK_WAVES) void vp_k_yin_track(VpTrackArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char trk_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int F = A.F, tauMax = A.tauMax, nRows = F / 8 + 64;
    trk_lds_f32 *xs = (trk_lds_f32 *)(trk_smem + (size_t)wave * trk_wave_bytes(F));
#ifdef VP_POISON_LDS
    for (int i = lane; i < nRows * TRK_ROW; i += 64) xs[i] = __builtin_nanf("0x5a5a");
    trk_wave_sync();
#endif
    const long long g = (long long)blockIdx.x * VP_TRACK_WAVES + wave;       // frame of the batch
    if (g >= (long long)A.S * A.nFrames) return;
    const int s = (int)(g / A.nFrames), f = (int)(g - (long long)s * A.nFrames);
    const int win = F + tauMax;
    const long long fh = (long long)f * A.hop;
    const int b = (int)(fh < (long long)(A.T - win) ? fh : (long long)(A.T - win));
    const float *row = A.in + (size_t)s * A.T + b;

    // the note table of the stream's key: freq[lane], freq[64 + lane]
    int key = A.key ? A.key[s] : 12;
    if (key < 0 || key > 12) key = 12;
    const double *freq = A.notes + (size_t)key * VP_NOTES_STRIDE;
    const int notesN = A.notesN[key];
    const double nf0 = freq[lane], nf1 = (lane + 64 < VP_NOTES_STRIDE) ? freq[lane + 64] : 0.0;

    // the window, zeros behind it (they only reach lags >= tauMax, which nothing reads)
    for (int p = lane; p < nRows * 8; p += 64) xs[p + (p >> 3)] = p < win ? row[p] : 0.0f;
    trk_wave_sync();

    // d[8 lane + j] = sum over i of (x[i] - x[i + 8 lane + j])^2, i ascending; w[m] = x[i0 + 8 lane + m]
    double acc[VP_TRACK_LAGS], w[2 * VP_TRACK_LAGS];
    const trk_lds_f32 *wl = xs + TRK_ROW * lane;
#pragma unroll
    for (int j = 0; j < VP_TRACK_LAGS; j++) { acc[j] = 0.0; w[j] = (double)wl[j]; }
    for (int blk = 0; blk < F / 8; blk++) {
        const trk_lds_f32 *nx = wl + TRK_ROW * (blk + 1), *vb = xs + TRK_ROW * blk;
        double v[8];
#pragma unroll
        for (int m = 0; m < 8; m++) { w[8 + m] = (double)nx[m]; v[m] = (double)vb[m]; }
#pragma unroll
        for (int u = 0; u < 8; u++) {
#pragma unroll
            for (int j = 0; j < VP_TRACK_LAGS; j++) {
                const double d = v[u] - w[u + j];
                acc[j] += d * d;
            }
        }
#pragma unroll
        for (int m = 0; m < 8; m++) w[m] = w[8 + m];
    }
    trk_wave_sync();                                                          // (the slice is rewritten below)

    // :395-403: d[0] = 1, tmp += d[k], d[k] *= k / tmp in increasing k -- tmp starts at 0 and 0 + d[1] is d[1], so lag 0 enters as 0
    if (lane == 0) acc[0] = 0.0;
    double cum[VP_TRACK_LAGS], carry = 0.0;
#pragma unroll
    for (int j = 0; j < VP_TRACK_LAGS; j++) cum[j] = 1.0;
    const int nOwners = (tauMax + VP_TRACK_LAGS - 1) / VP_TRACK_LAGS;
    for (int l = 0; l < nOwners; l++) {
        double t = carry;
        if (lane == l) {
#pragma unroll
            for (int j = 0; j < VP_TRACK_LAGS; j++) { t += acc[j]; cum[j] = t; }
        }
        carry = trk_readlane(t, l);
    }
    trk_lds_f64 *dn = (trk_lds_f64 *)xs;
#pragma unroll
    for (int j = 0; j < VP_TRACK_LAGS; j++) {
        const int k = VP_TRACK_LAGS * lane + j;
        const double q = (double)k / cum[j];
        double y = acc[j] * q;                                                // (silence: 0 * inf = NaN, which fails the tolerance test)
        if (k == 0) y = 1.0;
        if (k >= tauMax) y = 0.0;                                             // the guard slot d[tauMax] = 0; lags behind it are not read
        dn[k] = y;
    }
    if (lane == 0) dn[TRK_MAXLAG] = 0.0;                                      // (the guard slot at tauMax = 512)
    trk_wave_sync();

    // :429-447 on ballots, lag 64 q + lane: under[q] = d[k] < yinTol for tau0 <= k < tauMax, stop[q] = !(d[k + 1] < d[k])
    unsigned long long under[TRK_MAXLAG / 64], stop[TRK_MAXLAG / 64];
#pragma unroll
    for (int q = 0; q < TRK_MAXLAG / 64; q++) {
        const int k = 64 * q + lane;
        const double y0 = dn[k], y1 = dn[k + 1];
        under[q] = __ballot(k >= A.tau0 && k < tauMax && y0 < 0.25);
        stop[q] = __ballot(!(y1 < y0));
    }
    int first = INT_MAX;                                                      // first lag under the tolerance
#pragma unroll
    for (int q = TRK_MAXLAG / 64 - 1; q >= 0; q--)
        if (under[q]) first = 64 * q + (int)__builtin_ctzll(under[q]);
    int tau = 0;
    if (first != INT_MAX) {
        int ks = TRK_MAXLAG;                                                  // first lag >= first at which the descent stops
#pragma unroll
        for (int q = TRK_MAXLAG / 64 - 1; q >= 0; q--) {
            unsigned long long m = stop[q];
            if (64 * q + 63 < first) m = 0;
            else if (64 * q < first) m &= ~0ULL << (first - 64 * q);
            if (m) ks = 64 * q + (int)__builtin_ctzll(m);
        }
        // the walk leaves at tauMax - 1 without looking further (:438-439); started there, it looks once, at the guard slot
        if (first + 1 >= tauMax) tau = ks > first ? first + 1 : first;
        else tau = ks < tauMax - 1 ? ks : tauMax - 1;
    }
    tau = __builtin_amdgcn_readfirstlane(tau);

    double ratio = 1.0;
    if (tau > 0) {
        // Notes::getClosestFreq (Notes.cpp:79-110): lower_bound = entries below the pitch; idx == size reads the popped slot (:99)
        const double pitch = A.fs / tau;
        const int idx = __builtin_amdgcn_readfirstlane(__popcll(__ballot(lane < notesN && nf0 < pitch)) + __popcll(__ballot(lane + 64 < notesN && nf1 < pitch)));
        const double fi = idx >= 64 ? trk_readlane(nf1, idx & 63) : trk_readlane(nf0, idx & 63);
        double closest = fi;
        if (idx > 0) {
            const int im = idx - 1;
            const double fim = im >= 64 ? trk_readlane(nf1, im & 63) : trk_readlane(nf0, im & 63);
            if (!(fabs(fi - pitch) <= fabs(fim - pitch))) closest = fim;
        }
        ratio = closest / pitch;                                              // :595-596
    }
    if (lane == 0) {
        if (A.period) A.period[g] = tau;
        if (A.ratio) A.ratio[g] = ratio;
    }
}

hipError_t vp_track_launch(const VpTrackArgs &a, hipStream_t st)
{
    const long long frames = (long long)a.S * a.nFrames;
    const unsigned grid = (unsigned)((frames + VP_TRACK_WAVES - 1) / VP_TRACK_WAVES);
    hipLaunchKernelGGL(vp_k_yin_track, dim3(grid), dim3(64 * VP_TRACK_WAVES), vp_track_lds_bytes(a.F), st, a);
    return hipGetLastError();
}
