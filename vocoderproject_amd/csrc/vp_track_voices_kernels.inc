// vp_track_voices_kernels.inc -- the key-aware voices of the pitch trackers, included at the end of csrc/vp_track.hip (whose helpers,
// staging and follow code it continues): vp_k_yin_track_voices, vp_k_yin_track_voices_stream, vp_k_track_follow_voices,
// vp_k_track_reset_voices and their launchers.
// ---- key-aware voices: the trackers' decision, then V ratios at scale degrees of the note it chose ------------------------------------
// The definitions are tests/pv_harmkey_reference.py and tests/pv_harmkey_stream_reference.py.  vp_k_yin_track_voices and
// vp_k_yin_track_voices_stream stage their windows as vp_k_yin_track and vp_k_yin_track_stream do and run the same vp_track_body.inc;
// behind it vp_track_voices.inc recovers the index c of the note the lookup chose and reads, per voice, the entry d steps from it in the
// key's harmony table (the tracker's recurrence through a 25 .. 3200 Hz filter: the tracker's table is a slice of it).  That table sits in
// two more registers per lane, requested with the note table.  Lane v < V stores voice v's ratio, lane 0 the period.
__device__ __forceinline__ double trk_unvoiced(double u) { return fabs(u) <= 1.7976931348623157e308 ? u : 1.0; }   // (a NaN fails the test)

__global__ __launch_bounds__(64 * VP_TRACK_WAVES) void vp_k_yin_track_voices(VpTrackArgs A, VpTrackVoices VC)
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

    // the note table of the stream's key and its harmony table: entry lane, entry 64 + lane of each
    int key = A.key ? A.key[s] : 12;
    if (key < 0 || key > 12) key = 12;
    const double *freq = A.notes + (size_t)key * VP_NOTES_STRIDE, *hfreq = VC.harm + (size_t)key * VP_NOTES_STRIDE;
    const int notesN = A.notesN[key], hOff = VC.harmOff[key];
    const double nf0 = freq[lane], nf1 = (lane + 64 < VP_NOTES_STRIDE) ? freq[lane + 64] : 0.0;
    const double hf0 = hfreq[lane], hf1 = (lane + 64 < VP_NOTES_STRIDE) ? hfreq[lane + 64] : 0.0;

    // the window, zeros behind it (they only reach lags >= tauMax, which nothing reads)
    for (int p = lane; p < nRows * 8; p += 64) xs[p + (p >> 3)] = p < win ? row[p] : 0.0f;
    trk_wave_sync();

#include "vp_track_body.inc"
#include "vp_track_voices.inc"
    (void)ratio;                                                              // (the mono ratio: voice 0 at degree 0 has its bits)
    if (lane == 0 && A.period) A.period[g] = tau;
    if (lane < VC.V && A.ratio) A.ratio[((size_t)s * VC.V + lane) * A.nFrames + f] = vr;
}

__global__ __launch_bounds__(64 * VP_TRACK_WAVES) void vp_k_yin_track_voices_stream(VpTrackStreamArgs A, VpTrackVoices VC)
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
        if (lane == 0) A.period[g] = 0;
        if (lane < VC.V) A.ratio[(size_t)g * VC.V + lane] = VC.unvoiced ? trk_unvoiced(VC.unvoiced[(size_t)s * VC.V + lane]) : 1.0;
        return;
    }

    // the note table of the stream's key and its harmony table: entry lane, entry 64 + lane of each
    int key = A.key ? A.key[s] : 12;
    if (key < 0 || key > 12) key = 12;
    const double *freq = A.notes + (size_t)key * VP_NOTES_STRIDE, *hfreq = VC.harm + (size_t)key * VP_NOTES_STRIDE;
    const int notesN = A.notesN[key], hOff = VC.harmOff[key];
    const double nf0 = freq[lane], nf1 = (lane + 64 < VP_NOTES_STRIDE) ? freq[lane + 64] : 0.0;
    const double hf0 = hfreq[lane], hf1 = (lane + 64 < VP_NOTES_STRIDE) ? hfreq[lane + 64] : 0.0;

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
#include "vp_track_voices.inc"
    (void)ratio;                                                              // (the mono ratio: voice 0 at degree 0 has its bits)
    if (lane == 0) A.period[g] = tau;
    if (lane < VC.V) A.ratio[(size_t)g * VC.V + lane] = vr;
}

// vp_k_track_follow with one lane per (stream, voice): the V lanes of a stream compute the stream's one age identically, voice 0 stores it
// and the counter; the voices a call does not name keep their state.  The ring update is vp_k_track_follow's
__global__ __launch_bounds__(256) void vp_k_track_follow_voices(VpTrackFollowVoicesArgs A)
{
    __shared__ int slot0[VP_TRKS_GROUP];
    const int tid = threadIdx.x, s0 = blockIdx.x * VP_TRKS_GROUP;
    const int nS = A.S - s0 < VP_TRKS_GROUP ? A.S - s0 : VP_TRKS_GROUP;
    const int total = A.nBlocks * A.N;                                        // (<= 2^28: checked by the caller)
    const int cnt = total < A.W ? total : A.W, j0 = total - cnt;              // the call's last cnt samples go to the ring
    const int sl = tid / VP_TRACK_MAX_VOICES, v = tid - sl * VP_TRACK_MAX_VOICES;
    const bool mine = sl < nS && v < A.V;
    long long n0 = 0;
    if (mine) {
        n0 = A.count[s0 + sl];
        if (v == 0) slot0[sl] = (int)((n0 + j0) % A.W);
    }
    __syncthreads();                                                          // (every read of the counters lies before this)
    if (mine) {
        const int s = s0 + sl;
        const size_t sv = (size_t)s * VP_TRACK_MAX_VOICES + v;
        const double u = A.unvoiced ? trk_unvoiced(A.unvoiced[(size_t)s * A.V + v]) : 1.0;
        double tgt = A.tgt[sv], cur = A.cur[sv];
        int age = A.age[s];
        for (int b = 0; b < A.nBlocks; b++) {
            const size_t i = (size_t)b * A.S + s;
            if (A.period[i] > 0) { tgt = A.ratio[i * A.V + v]; age = 0; }
            else {
                if (age < INT_MAX) age++;
                if (age > A.hold) tgt = u;
            }
            if (A.glide == 1.0) cur = tgt;
            else {
                const double step = A.glide * (tgt - cur);                    // (product and add separate: -ffp-contract=off)
                cur = cur + step;
            }
            A.ratio[i * A.V + v] = cur;
        }
        A.tgt[sv] = tgt; A.cur[sv] = cur;
        if (v == 0) { A.age[s] = age; A.count[s] = n0 + total; }              // (its voices are lanes of this wavefront: they read both above)
    }
    trk_ring_update(A.ring, A.in, slot0, tid, s0, nS, cnt, j0, A.S, A.N, A.W);
}

// the voices' follow state of a reset stream: (1.0, 0, 1.0) for every voice.  A.count is not read; A.tgt / A.cur are [S][VP_TRACK_MAX_VOICES]
__global__ __launch_bounds__(256) void vp_k_track_reset_voices(VpTrackUpdArgs A)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= A.S) return;
    bool hit = false;
    for (int k = 0; k < A.n; k++) hit = hit || A.stream[k] < 0 || A.stream[k] == s;
    if (hit) {
        for (int v = 0; v < VP_TRACK_MAX_VOICES; v++) { A.tgt[(size_t)s * VP_TRACK_MAX_VOICES + v] = 1.0; A.cur[(size_t)s * VP_TRACK_MAX_VOICES + v] = 1.0; }
        A.age[s] = 0;
    }
}

hipError_t vp_track_voices_launch(const VpTrackArgs &a, const VpTrackVoices &v, hipStream_t st)
{
    const long long frames = (long long)a.S * a.nFrames;
    const unsigned grid = (unsigned)((frames + VP_TRACK_WAVES - 1) / VP_TRACK_WAVES);
    hipLaunchKernelGGL(vp_k_yin_track_voices, dim3(grid), dim3(64 * VP_TRACK_WAVES), vp_track_lds_bytes(a.F), st, a, v);
    return hipGetLastError();
}

hipError_t vp_track_voices_stream_launch(const VpTrackStreamArgs &a, const VpTrackVoices &v, hipStream_t st)
{
    const long long n = (long long)a.S * a.nBlocks;
    const unsigned grid = (unsigned)((n + VP_TRACK_WAVES - 1) / VP_TRACK_WAVES);
    hipLaunchKernelGGL(vp_k_yin_track_voices_stream, dim3(grid), dim3(64 * VP_TRACK_WAVES), vp_track_lds_bytes(a.F), st, a, v);
    return hipGetLastError();
}

hipError_t vp_track_follow_voices_launch(const VpTrackFollowVoicesArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_track_follow_voices, dim3((a.S + VP_TRKS_GROUP - 1) / VP_TRKS_GROUP), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t vp_track_reset_voices_launch(const VpTrackUpdArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_track_reset_voices, dim3((a.S + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}
