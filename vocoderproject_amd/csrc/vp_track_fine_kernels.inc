// vp_track_fine_kernels.inc -- the fine (sub-sample) pitch trackers, included at the end of csrc/vp_track.hip behind
// vp_track_voices_kernels.inc (whose helpers and staging it continues): vp_k_yin_track_fine, vp_k_yin_track_stream_fine,
// vp_k_yin_track_voices_fine, vp_k_yin_track_voices_stream_fine and their launchers.
// ---- fine trackers: the integer decision, then the parabola through the normalised function's minimum -------------------------------
// The definitions are tests/pv_track_fine_reference.py and tests/pv_track_fine_stream_reference.py.  Each kernel stages its window as
// its integer sibling does and runs the same vp_track_body.inc; behind it vp_track_fine.inc refines the period and repeats the note
// lookup on the refined pitch.  The voice stage is vp_track_voices.inc, unchanged, run on the refined period (see trk_fine_voices
// below), so a voice's note index comes from the refined pitch too.  Lane 0 also stores the refined period where a table is given.
// The follow and reset kernels behind the streaming ones are the integer trackers': they read the int period only as the voiced flag.

// vp_track_voices.inc reads the period as `tau` (the voiced test and `A.fs / tau`).  Here it is included where `tau` names the refined
// period, a double: the same statements then give fs / tauFine, and an unrefined frame divides by (double)tau as the integer kernels do.
// (vp_track_voices.inc's header names this second includer and what it may do with `tau`; the int period is stored before the block opens.)
#define TRK_FINE_VOICES_BEGIN { const double tau = tauFine;
#define TRK_FINE_VOICES_END }

template <bool VOICES>
__device__ __forceinline__ void trk_fine_batch(const VpTrackArgs &A, const VpTrackVoices &VC, double *periodFine)
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

    // the note table of the stream's key (and its harmony table): entry lane, entry 64 + lane
    int key = A.key ? A.key[s] : 12;
    if (key < 0 || key > 12) key = 12;
    const double *freq = A.notes + (size_t)key * VP_NOTES_STRIDE;
    const int notesN = A.notesN[key];
    const double nf0 = freq[lane], nf1 = (lane + 64 < VP_NOTES_STRIDE) ? freq[lane + 64] : 0.0;
    double hf0 = 0.0, hf1 = 0.0;
    int hOff = 0;
    if constexpr (VOICES) {
        const double *hfreq = VC.harm + (size_t)key * VP_NOTES_STRIDE;
        hOff = VC.harmOff[key];
        hf0 = hfreq[lane]; hf1 = (lane + 64 < VP_NOTES_STRIDE) ? hfreq[lane + 64] : 0.0;
    }

    // the window, zeros behind it (they only reach lags >= tauMax, which nothing reads)
    for (int p = lane; p < nRows * 8; p += 64) xs[p + (p >> 3)] = p < win ? row[p] : 0.0f;
    trk_wave_sync();

#include "vp_track_body.inc"
#include "vp_track_fine.inc"
    if (lane == 0) {
        if (A.period) A.period[g] = tau;
        if (periodFine) periodFine[g] = tauFine;
    }
    if constexpr (VOICES) {
        TRK_FINE_VOICES_BEGIN
#include "vp_track_voices.inc"
        if (lane < VC.V && A.ratio) A.ratio[((size_t)s * VC.V + lane) * A.nFrames + f] = vr;
        TRK_FINE_VOICES_END
    } else {
        if (lane == 0 && A.ratio) A.ratio[g] = ratio;
    }
}

template <bool VOICES>
__device__ __forceinline__ void trk_fine_stream(const VpTrackStreamArgs &A, const VpTrackVoices &VC, double *periodFine)
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
        if (lane == 0) {
            A.period[g] = 0;
            if (periodFine) periodFine[g] = 0.0;
            if constexpr (!VOICES) A.ratio[g] = 1.0;
        }
        if constexpr (VOICES)
            if (lane < VC.V) A.ratio[(size_t)g * VC.V + lane] = VC.unvoiced ? trk_unvoiced(VC.unvoiced[(size_t)s * VC.V + lane]) : 1.0;
        return;
    }

    // the note table of the stream's key (and its harmony table): entry lane, entry 64 + lane
    int key = A.key ? A.key[s] : 12;
    if (key < 0 || key > 12) key = 12;
    const double *freq = A.notes + (size_t)key * VP_NOTES_STRIDE;
    const int notesN = A.notesN[key];
    const double nf0 = freq[lane], nf1 = (lane + 64 < VP_NOTES_STRIDE) ? freq[lane + 64] : 0.0;
    double hf0 = 0.0, hf1 = 0.0;
    int hOff = 0;
    if constexpr (VOICES) {
        const double *hfreq = VC.harm + (size_t)key * VP_NOTES_STRIDE;
        hOff = VC.harmOff[key];
        hf0 = hfreq[lane]; hf1 = (lane + 64 < VP_NOTES_STRIDE) ? hfreq[lane + 64] : 0.0;
    }

    // the window, zeros behind it: vp_k_yin_track_stream's gather
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
#include "vp_track_fine.inc"
    if (lane == 0) {
        A.period[g] = tau;
        if (periodFine) periodFine[g] = tauFine;
    }
    if constexpr (VOICES) {
        TRK_FINE_VOICES_BEGIN
#include "vp_track_voices.inc"
        if (lane < VC.V) A.ratio[(size_t)g * VC.V + lane] = vr;
        TRK_FINE_VOICES_END
    } else {
        if (lane == 0) A.ratio[g] = ratio;
    }
}

__global__ __launch_bounds__(64 * VP_TRACK_WAVES) void vp_k_yin_track_fine(VpTrackArgs A, double *periodFine)
{
    trk_fine_batch<false>(A, VpTrackVoices{}, periodFine);
}

__global__ __launch_bounds__(64 * VP_TRACK_WAVES) void vp_k_yin_track_voices_fine(VpTrackArgs A, VpTrackVoices VC)
{
    trk_fine_batch<true>(A, VC, nullptr);
}

__global__ __launch_bounds__(64 * VP_TRACK_WAVES) void vp_k_yin_track_stream_fine(VpTrackStreamArgs A, double *periodFine)
{
    trk_fine_stream<false>(A, VpTrackVoices{}, periodFine);
}

__global__ __launch_bounds__(64 * VP_TRACK_WAVES) void vp_k_yin_track_voices_stream_fine(VpTrackStreamArgs A, VpTrackVoices VC)
{
    trk_fine_stream<true>(A, VC, nullptr);
}

static inline unsigned trk_fine_grid(long long decisions) { return (unsigned)((decisions + VP_TRACK_WAVES - 1) / VP_TRACK_WAVES); }

hipError_t vp_track_fine_launch(const VpTrackArgs &a, double *periodFine, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_yin_track_fine, dim3(trk_fine_grid((long long)a.S * a.nFrames)), dim3(64 * VP_TRACK_WAVES), vp_track_lds_bytes(a.F), st, a, periodFine);
    return hipGetLastError();
}

hipError_t vp_track_voices_fine_launch(const VpTrackArgs &a, const VpTrackVoices &v, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_yin_track_voices_fine, dim3(trk_fine_grid((long long)a.S * a.nFrames)), dim3(64 * VP_TRACK_WAVES), vp_track_lds_bytes(a.F), st, a, v);
    return hipGetLastError();
}

hipError_t vp_track_stream_fine_launch(const VpTrackStreamArgs &a, double *periodFine, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_yin_track_stream_fine, dim3(trk_fine_grid((long long)a.S * a.nBlocks)), dim3(64 * VP_TRACK_WAVES), vp_track_lds_bytes(a.F), st, a, periodFine);
    return hipGetLastError();
}

hipError_t vp_track_voices_stream_fine_launch(const VpTrackStreamArgs &a, const VpTrackVoices &v, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_yin_track_voices_stream_fine, dim3(trk_fine_grid((long long)a.S * a.nBlocks)), dim3(64 * VP_TRACK_WAVES), vp_track_lds_bytes(a.F), st, a, v);
    return hipGetLastError();
}
