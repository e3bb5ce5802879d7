// vp_track.hip -- pitch trackers for the phase-vocoder path: YIN per STFT frame, the key's nearest note, one ratio per frame (the batch
// tracker), and the same decision per block of a stream with per-stream history (the streaming tracker, at the end of this file).
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

#include "vp_track_body.inc"
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

// ---- the streaming tracker: one decision per (block, stream) from the last F + tauMax samples the stream received --------------------
// The definition is tests/pv_track_stream_reference.py.  vp_k_yin_track_stream is vp_k_yin_track with another gather: window sample p of
// the decision of block b is the stream's sample n_b - W + p (n_b = count + (b + 1) N, W = F + tauMax), taken from the call's slab when the
// call brought it and from the stream's ring otherwise.  vp_k_track_follow runs behind it on the same stream: it follows the raw table
// (hold across unvoiced blocks, glide), advances the counters and only then overwrites the ring with the call's last samples.
__global__ __launch_bounds__(64 * VP_TRACK_WAVES) void vp_k_yin_track_stream(VpTrackStreamArgs A)
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
    const long long g = (long long)blockIdx.x * VP_TRACK_WAVES + wave;       // decision of the call: [block][stream]
    if (g >= (long long)A.S * A.nBlocks) return;
    const int b = (int)(g / A.S), s = (int)(g - (long long)b * A.S);
    const int win = F + tauMax, N = A.N;
    const int jEnd = (b + 1) * N;                                             // the block's end, counted from the call's first sample
    const long long nb = A.count[s] + jEnd;                                   // ... and from the stream's
    if (nb < win) {                                                           // not enough history yet: unvoiced, nothing is analysed
        if (lane == 0) { A.period[g] = 0; A.ratio[g] = 1.0; }
        return;
    }

    // the note table of the stream's key: freq[lane], freq[64 + lane]
    int key = A.key ? A.key[s] : 12;
    if (key < 0 || key > 12) key = 12;
    const double *freq = A.notes + (size_t)key * VP_NOTES_STRIDE;
    const int notesN = A.notesN[key];
    const double nf0 = freq[lane], nf1 = (lane + 64 < VP_NOTES_STRIDE) ? freq[lane + 64] : 0.0;

    // the window, zeros behind it.  Sample p lies jEnd - win + p samples into the call: in block blk at offset off when that is >= 0
    // (kept as a floored quotient, K blocks added before the division so that it divides a non-negative number), else in the ring at
    // slot (nb - win + p) % win = (nb % win + p) % win
    const int K = (win + N - 1) / N, q64 = 64 / N, r64 = 64 % N;
    const int jj = jEnd - win + K * N + lane;
    int blk = jj / N, off = jj - blk * N;
    blk -= K;
    const int r0 = (int)(nb % win);
    const float *ring = A.ring + (size_t)s * win;
    for (int p = lane; p < nRows * 8; p += 64) {
        float v = 0.0f;
        if (p < win) {
            const int slot = r0 + p < win ? r0 + p : r0 + p - win;
            v = blk >= 0 ? A.in[((size_t)blk * A.S + s) * N + off] : ring[slot];
        }
        xs[p + (p >> 3)] = v;
        blk += q64; off += r64;
        if (off >= N) { off -= N; blk++; }
    }
    trk_wave_sync();

#include "vp_track_body.inc"
    if (lane == 0) { A.period[g] = tau; A.ratio[g] = ratio; }
}

// the call's last cnt samples (from sample j0 of the slab on) of the workgroup's nS streams go to their rings, from slot0[stream] on
__device__ __forceinline__ void trk_ring_update(float *ring, const float *in, const int *slot0, int tid, int s0, int nS, int cnt, int j0, int S, int N, int W)
{
    for (int e = tid; e < nS * cnt; e += 256) {
        const int sl = e / cnt, k = e - sl * cnt, s = s0 + sl;
        const int j = j0 + k, blk = j / N, off = j - blk * N;
        const int slot = slot0[sl] + k < W ? slot0[sl] + k : slot0[sl] + k - W;
        ring[(size_t)s * W + slot] = in[((size_t)blk * S + s) * N + off];
    }
}

__global__ __launch_bounds__(256) void vp_k_track_follow(VpTrackFollowArgs A)
{
    __shared__ int slot0[VP_TRKS_GROUP];
    const int tid = threadIdx.x, s0 = blockIdx.x * VP_TRKS_GROUP;
    const int nS = A.S - s0 < VP_TRKS_GROUP ? A.S - s0 : VP_TRKS_GROUP;
    const int total = A.nBlocks * A.N;                                        // (<= 2^28: checked by the caller)
    const int cnt = total < A.W ? total : A.W, j0 = total - cnt;              // the call's last cnt samples go to the ring
    long long n0 = 0;
    if (tid < nS) {
        n0 = A.count[s0 + tid];
        slot0[tid] = (int)((n0 + j0) % A.W);
    }
    __syncthreads();                                                          // (every read of the counters lies before this)
    if (tid < nS) {
        // one lane per stream walks the blocks: rows of the tables are read across the lanes
        const int s = s0 + tid;
        double tgt = A.tgt[s], cur = A.cur[s];
        int age = A.age[s];
        for (int b = 0; b < A.nBlocks; b++) {
            const size_t i = (size_t)b * A.S + s;
            if (A.period[i] > 0) { tgt = A.ratio[i]; age = 0; }
            else {
                if (age < INT_MAX) age++;
                if (age > A.hold) tgt = 1.0;
            }
            if (A.glide == 1.0) cur = tgt;
            else {
                const double step = A.glide * (tgt - cur);                    // (product and add separate: -ffp-contract=off)
                cur = cur + step;
            }
            A.ratio[i] = cur;
        }
        A.tgt[s] = tgt; A.cur[s] = cur; A.age[s] = age;
        A.count[s] = n0 + total;
    }
    trk_ring_update(A.ring, A.in, slot0, tid, s0, nS, cnt, j0, A.S, A.N, A.W);
}

// a reset stream is a fresh one: no history, follow state (1.0, 0, 1.0)
__global__ __launch_bounds__(256) void vp_k_track_reset(VpTrackUpdArgs A)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= A.S) return;
    bool hit = false;
    for (int k = 0; k < A.n; k++) hit = hit || A.stream[k] < 0 || A.stream[k] == s;
    if (hit) { A.count[s] = 0; A.tgt[s] = 1.0; A.cur[s] = 1.0; A.age[s] = 0; }
}

hipError_t vp_track_stream_launch(const VpTrackStreamArgs &a, hipStream_t st)
{
    const long long n = (long long)a.S * a.nBlocks;
    const unsigned grid = (unsigned)((n + VP_TRACK_WAVES - 1) / VP_TRACK_WAVES);
    hipLaunchKernelGGL(vp_k_yin_track_stream, dim3(grid), dim3(64 * VP_TRACK_WAVES), vp_track_lds_bytes(a.F), st, a);
    return hipGetLastError();
}

hipError_t vp_track_follow_launch(const VpTrackFollowArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_track_follow, dim3((a.S + VP_TRKS_GROUP - 1) / VP_TRKS_GROUP), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t vp_track_reset_launch(const VpTrackUpdArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_track_reset, dim3((a.S + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---- key-aware voices (vp_stft_track_harmony, vp_pv_tracker_process_blocks_voices_device): the kernels above with the voice stage ------
#include "vp_track_voices_kernels.inc"

// ---- fine (sub-sample) trackers (VP_TRACK_FINE, vp_stft_track_pitch_fine): the kernels above with the parabolic stage -------------------
#include "vp_track_fine_kernels.inc"
