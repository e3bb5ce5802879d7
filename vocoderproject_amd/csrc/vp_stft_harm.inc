// vp_stft_harm.inc -- the phase-vocoder HARMONIZER: several peak-locked voices and the dry signal from one analysis (included by
// vp_stft.hip behind the locked family, vp_stft_lock.inc and vp_stft_lockf.inc: the locked stage's carve, masks, pv_lock_nearest and pv_lock_bin).
//
// A caller who wants a chord over the dry voice ran V locked calls and one round trip and mixed the results: V + 1 reads of the input,
// forward transforms, peak searches, inverse transforms and overlap-adds.  The inverse transform and the overlap-add are linear, and the
// analysis of the locked stage (previous phases, peaks, owners, the peaks' true frequencies) does not depend on the ratio.  So here a frame
// is analysed ONCE; only the per-voice part of the stage runs V times (shifted peaks, gather indices, one angle array per voice), the
// voices' synthesis spectra and the untouched spectrum are summed in registers, and ONE inverse transform and overlap-add follow.  The
// definition is tests/pv_harm_reference.py: dry roundtrip(x) + sum_v gain[v] locked_roundtrip(x, ratio[v]).
//
// vp_k_stft_harm and vp_k_hz_stream are WRITTEN-OUT COPIES of vp_k_stft_pv_lock and vp_k_pv_stream_lock (docs/HISTORY.md, "One
// phase-vocoder stage for both kernels", for why copies): framing, transforms and overlap-add are the parents', statement for statement,
// and the streaming call's bookkeeping is the parents' pv_call_* helpers.  What differs is marked "harm:".  pv_lock_plan is split in two: hz_analyse (once per frame: peaks, owners, and
// the peaks' true frequency nu where the parent leaves the angle's advance for its one ratio) and hz_voice_plan (per voice: shifted peaks
// and the gather's indices, in the parents' `moved` mask and `back` map, reused voice after voice).  hz_turn forms the advance
// (nu (r - 1)) / O with the parent's operations in the parent's order, so that one voice with gain 1 and no dry part has the locked
// kernel's bits.
//
// harm: V is a run-time count (1 .. VP_HARM_MAX_VOICES); the voice loop is the OUTERMOST loop of the stage and is not unrolled, so that
// one set of src / pk / th is live whatever V is: NWV - 1 barriers per voice and round.  (All voices inside each wavefront's turn would
// need NWV - 1 barriers in all but V sets of registers, indexed by a run-time count: not built.)
//
// harm: LDS behind the locked carve: the angle arrays of voices 1 .. 3 (voice 0 turns PvLds::sum, as the parents' one voice does).
#define HZ_EXTRA_THETA (VP_HARM_MAX_VOICES - 1)
__host__ __device__ constexpr size_t hz_lds_bytes() { return (size_t)HZ_EXTRA_THETA * VP_PV_NB * sizeof(double); }

// harm: a gain as the kernels take it: a NaN or an infinity counts as 0, the rest is clamped to [-4, 4]
__device__ __forceinline__ double hz_gain(double g) { return __builtin_isfinite(g) ? fmin(fmax(g, -4.0), 4.0) : 0.0; }

// harm: entry v of four values held in registers, v a run-time count (wavefront-uniform)
__device__ __forceinline__ double hz_pick(const double (&a)[VP_HARM_MAX_VOICES], int v) { return v == 0 ? a[0] : v == 1 ? a[1] : v == 2 ? a[2] : a[3]; }

// harm: the part of pv_lock_plan that no ratio enters, once per frame, by one live wavefront (magnitudes, phases and the spectrum to LDS
// are the caller's, before its barrier): the peaks' mask, the owner of every bin (own[e] of the lane's bins, lk.own of all), and at every
// peak its true frequency nu in bins in place of its magnitude in the wavefront's `inc` row.  Returns whether the frame has a peak
// (wavefront-uniform).
__device__ __forceinline__ bool hz_analyse(const PvLds &pv, const PvLockLds &lk, int wv, int prevSlot, int ln, bool lane0, double invO, int O, int (&own)[9])
{
    constexpr int N = 512, nb = N + 1;
    lds_f64 *mrow = pv.inc + wv * nb;
    unsigned long long bal[9];
    bool isPk[9];
#pragma unroll
    for (int e = 0; e < 9; e++) {
        const int k = pv_lock_bin(e, ln);
        const double c = mrow[k];
        const double l1 = mrow[max(k - 1, 0)], l2 = mrow[max(k - 2, 0)], r1 = mrow[min(k + 1, N)], r2 = mrow[min(k + 2, N)];
        bool p = (e < 8 || lane0) && c > 0.0;
        p = p && (k < 1 || c > l1) && (k < 2 || c > l2) && (k + 1 > N || c >= r1) && (k + 2 > N || c >= r2);
        isPk[e] = p;
        bal[e] = __ballot(p);
    }
    unsigned long long any = 0ull;
#pragma unroll
    for (int e = 0; e < 9; e++) any |= bal[e];
#pragma unroll
    for (int e = 0; e < 9; e++) own[e] = 0;
    if (any == 0ull) return false;                                             // (all zeros, or nothing finite: the frame is silent)
    pv_lock_mask(lk.peaks, bal, lane0);
    wave_sync();                                                               // (and every lane has read its magnitudes)
#pragma unroll
    for (int e = 0; e < 9; e++) {
        if (!isPk[e]) continue;
        const int k = pv_lock_bin(e, ln);
        double d = pv.phPrev[(wv + 1) * nb + k] - pv.phPrev[prevSlot * nb + k] - (double)k * invO;
        d -= rint(d);
        const double nu = (double)k + d * (double)O;
        mrow[k] = nu;                                                          // harm: the advance is formed per voice, in hz_turn
    }
#pragma unroll
    for (int e = 0; e < 9; e++) {
        const int k = pv_lock_bin(e, ln);
        own[e] = pv_lock_nearest(lk.peaks, k);
        if (e < 8 || lane0) lk.own[k] = own[e];
    }
    wave_sync();
    return true;
}

// harm: the part of pv_lock_plan that one voice's ratio enters, by a wavefront whose frame has a peak: the shifted peaks (lk.moved, lk.back:
// the parents' arrays, overwritten voice after voice) and the gather's indices.  src[e]: the source bin of synthesis bin e or -1 (zero);
// pk[e]: the peak whose angle rotates it.
__device__ __forceinline__ void hz_voice_plan(const PvLockLds &lk, int ln, bool lane0, double ratio, int (&src)[9], int (&pk)[9])
{
    constexpr int N = 512;
    unsigned long long bal[9];
#pragma unroll
    for (int e = 0; e < 9; e++) { src[e] = -1; pk[e] = 0; }
    wave_sync();                                                               // (the previous voice's reads of back and moved are done)
#pragma unroll
    for (int e = 0; e < 9; e++) if (e < 8 || lane0) lk.back[pv_lock_bin(e, ln)] = -1;
    wave_sync();
#pragma unroll
    for (int e = 0; e < 9; e++) {
        const int k = pv_lock_bin(e, ln);
        if (!((e < 8 || lane0) && ((lk.peaks[k >> 6] >> (k & 63)) & 1ull))) continue;
        const int kp = (int)floor((double)k * ratio + 0.5);
        if (kp <= N) lk.back[kp] = k;                                          // (peaks are three bins apart: distinct for r >= 0.5)
    }
    wave_sync();
#pragma unroll
    for (int e = 0; e < 9; e++) bal[e] = __ballot((e < 8 || lane0) && lk.back[pv_lock_bin(e, ln)] >= 0);
    unsigned long long any = 0ull;
#pragma unroll
    for (int e = 0; e < 9; e++) any |= bal[e];
    pv_lock_mask(lk.moved, bal, lane0);
    wave_sync();
    if (any != 0ull) {
#pragma unroll
        for (int e = 0; e < 9; e++) {
            const int kk = pv_lock_bin(e, ln);
            const int ps = pv_lock_nearest(lk.moved, kk);
            const int pa = lk.back[ps];
            const int k = kk - (ps - pa);
            pk[e] = pa;
            src[e] = (k >= 0 && k <= N && lk.own[min(max(k, 0), N)] == pa) ? k : -1;
        }
    }
}

// harm: a wavefront's turn at one voice's theta, in frame order between the caller's barriers (pv_lock_turn with the advance formed here:
// product, product, sum, each rounded on its own as in the parent, where the advance passes through LDS)
__device__ __forceinline__ void hz_turn(lds_f64 *theta, const PvLds &pv, int wv, int ln, bool lane0, double ratio, double invO, const int (&own)[9],
                                        const int (&src)[9], const int (&pk)[9], double (&th)[9])
{
#pragma clang fp contract(off)
    constexpr int nb = 513;
    double t[9];
#pragma unroll
    for (int e = 0; e < 9; e++) {
        const double adv = (pv.inc[wv * nb + own[e]] * (ratio - 1.0)) * invO;  // r - 1 is exact on [0.5, 2], 1 / O a power of two
        t[e] = theta[own[e]] + adv;
        t[e] -= rint(t[e]);
    }
    wave_sync();                                                               // (other lanes read theta[P] of bins this lane overwrites)
#pragma unroll
    for (int e = 0; e < 9; e++) if (e < 8 || lane0) theta[pv_lock_bin(e, ln)] = t[e];
    wave_sync();
#pragma unroll
    for (int e = 0; e < 9; e++) th[e] = src[e] >= 0 ? theta[pk[e]] : 0.0;
}

// harm: pv_lock_gather, added to the sum with the voice's gain instead of stored: acc += g Y, Y's bins 0 and 512 real
__device__ __forceinline__ void hz_gather_add(const PvLds &pv, bool lane0, const int (&src)[9], const double (&th)[9], double g, RPairs &X)
{
#pragma unroll
    for (int e = 0; e < 9; e++) {
        if (e == 8 && !lane0) continue;
        double re = 0.0, im = 0.0;
        if (src[e] >= 0) {
            const d2 x = pv.ana[src[e]];
            double sn, cs;
            pv_sincos_turns(th[e], sn, cs);
            re = __builtin_fma(x.x, cs, -(x.y * sn));
            im = __builtin_fma(x.x, sn, x.y * cs);
        }
        if (e < 2 && lane0) im = 0.0;
        if (e == 8) { X.hr = __builtin_fma(g, re, X.hr); X.hi = __builtin_fma(g, im, X.hi); }
        else if (e & 1) { X.mr[e >> 1] = __builtin_fma(g, re, X.mr[e >> 1]); X.mi[e >> 1] = __builtin_fma(g, im, X.mi[e >> 1]); }
        else { X.kr[e >> 1] = __builtin_fma(g, re, X.kr[e >> 1]); X.ki[e >> 1] = __builtin_fma(g, im, X.ki[e >> 1]); }
    }
}

// harm: the sum starts as dry X, X as rfft_split left it (dry 1: X itself; dry 0: skipped, uniformly)
__device__ __forceinline__ void hz_dry(RPairs &X, double dry)
{
    if (dry == 0.0) {
#pragma unroll
        for (int q = 0; q < 4; q++) { X.kr[q] = 0.0; X.ki[q] = 0.0; X.mr[q] = 0.0; X.mi[q] = 0.0; }
        X.hr = 0.0; X.hi = 0.0;
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) { X.kr[q] *= dry; X.ki[q] *= dry; X.mr[q] *= dry; X.mi[q] *= dry; }
        X.hr *= dry; X.hi *= dry;
    }
}

// ratioTab [S][V][nFrames]; gainTab [S][V] or null (1); dryTab [S] or null (0)
__global__ __launch_bounds__(64 * NWV) void vp_k_stft_harm(VpStftArgs A, const double *ratioTab, const double *gainTab, const double *dryTab, int V)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 512;                                                     // complex points = F / 2
    const int F = A.F, hop = A.hop, O = A.O, T = A.T;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;
    lds_f32 *carry = (lds_f32 *)smem + NWV * 2048;                             // [(O - 1) hop]
    const PvLds pv = pv_lds_carve((lds_f64 *)smem + stft_lds_base(F, hop) / 8, wv);
    const PvLockLds lk = pv_lock_carve((lds_f64 *)smem + (stft_lds_base(F, hop) + pv_lds_bytes()) / 8, wv);
    lds_f64 *thetaX = (lds_f64 *)smem + (stft_lds_base(F, hop) + pv_lds_bytes() + pv_lock_lds_bytes()) / 8;   // harm: [3][513], voices 1 .. 3
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)((stft_lds_base(F, hop) + pv_lds_bytes() + pv_lock_lds_bytes() + hz_lds_bytes()) / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
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

    for (int i = tid; i < F - hop; i += 64 * NWV) carry[i] = 0.f;
    for (int i = tid; i < VP_PV_NB; i += 64 * NWV) { pv.phPrev[i] = 0.0; pv.sum[i] = 0.0; }
    for (int i = tid; i < HZ_EXTRA_THETA * VP_PV_NB; i += 64 * NWV) thetaX[i] = 0.0;   // harm:
    __syncthreads();

    const StftRun R = stft_run(A, run);
    const float *xs = A.in + (size_t)s * T;
    const double *rs = ratioTab + (size_t)s * V * A.nFrames;                  // harm: [V][nFrames]
    // harm: the stream's gains, once
    double gn[VP_HARM_MAX_VOICES];
#pragma unroll
    for (int v = 0; v < VP_HARM_MAX_VOICES; v++) gn[v] = (v < V && gainTab) ? hz_gain(gainTab[(size_t)s * V + v]) : 1.0;
    const double dry = dryTab ? hz_gain(dryTab[s]) : 0.0;
    // the frame's samples, and its ratios, are requested a round ahead
    f2 xv[8];
    double rq[VP_HARM_MAX_VOICES];
#pragma unroll
    for (int v = 0; v < VP_HARM_MAX_VOICES; v++) rq[v] = 1.0;
    auto request = [&](int rd_) {
        const int f_ = rd_ * NWV + wv;
        if (rd_ < R.r1 && f_ < A.nFrames) {
            stft_load_frame(xv, xs + (size_t)f_ * hop, A.aligned, lane);
#pragma unroll
            for (int v = 0; v < VP_HARM_MAX_VOICES; v++) if (v < V) rq[v] = rs[(size_t)v * A.nFrames + f_];
        }
    };
    request(R.r0);
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        C8 z;
        RPairs X;
        double rr[VP_HARM_MAX_VOICES];
#pragma unroll
        for (int v = 0; v < VP_HARM_MAX_VOICES; v++) rr[v] = pv_curve_clamp(rq[v]);
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; r++) { z.re[r] = (double)xv[r].x * wa[r].x; z.im[r] = (double)xv[r].y * wa[r].y; }
        }
        request(rd + 1);
        if (live) {
            fft512_rx(z, xb, L);
            rfft_split(z, xb, lane, (const d2 *)ws, X);
        }
        {
            // ---- harm: the stage: one analysis, then the voices' turns one voice after the other (to the merge)
            const int nb = N + 1;
            const double invO = 1.0 / (double)O;
            // (the lane number through a register the compiler cannot see through: vp_k_stft_pv2k)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            if (live) {
                // spectrum, magnitude and phase of the lane's bins, straight to LDS
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int k = 64 * q + ln, m = N - k;
                    pv.ana[k] = d2{X.kr[q], X.ki[q]}; pv.ana[m] = d2{X.mr[q], X.mi[q]};
                    pv.inc[wv * nb + k] = sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]); pv.phPrev[(wv + 1) * nb + k] = pv_phase_turns(X.ki[q], X.kr[q]);
                    pv.inc[wv * nb + m] = sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]); pv.phPrev[(wv + 1) * nb + m] = pv_phase_turns(X.mi[q], X.mr[q]);
                }
                if (lane0) {
                    pv.ana[N / 2] = d2{X.hr, X.hi};
                    pv.inc[wv * nb + N / 2] = sqrt(X.hr * X.hr + X.hi * X.hi); pv.phPrev[(wv + 1) * nb + N / 2] = pv_phase_turns(X.hi, X.hr);
                }
                hz_dry(X, dry);                                                // harm: X is the sum from here on
            }
            __syncthreads();
            int own[9];
            bool has = false;
            if (live) has = hz_analyse(pv, lk, wv, wv, ln, lane0, invO, O, own);
            // harm: every voice's theta is handed through the round in frame order, in place
#pragma nounroll
            for (int v = 0; v < V; v++) {
                const double ratio = hz_pick(rr, v), g = hz_pick(gn, v);
                lds_f64 *theta = v == 0 ? pv.sum : thetaX + (v - 1) * nb;
                int src[9], pk[9];
                double th[9];
#pragma unroll
                for (int e = 0; e < 9; e++) { src[e] = -1; pk[e] = 0; th[e] = 0.0; }
                if (live && has) hz_voice_plan(lk, ln, lane0, ratio, src, pk);
#pragma unroll
                for (int w = 0; w < NWV; w++) {
                    if (w > 0) __syncthreads();
                    if (live && has && wv == w) hz_turn(theta, pv, wv, ln, lane0, ratio, invO, own, src, pk, th);
                }
                if (live && has) hz_gather_add(pv, lane0, src, th, g, X);
            }
            // (every live wavefront is past its reads of the previous frame's phases: the turns' barriers, V >= 1, or program order when the
            // round's only live wavefront is wavefront 0)
            const int lastLive = min(NWV - 1, A.nFrames - 1 - rd * NWV);
            if (live && wv == lastLive) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int k = pv_lock_bin(e, ln);
                    pv.phPrev[k] = pv.phPrev[(wv + 1) * nb + k];
                }
            }
            // ---- harm: end of the stage
        }
        lds_f2 *slot = (lds_f2 *)(slots + wv * 2048);
        if (live) {
            rfft_merge_conj(z, xb, lane, (const d2 *)ws, X, A.c);
            fft512_rx(z, xb, L);
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f2{(float)(z.re[r] * wa[r].x), (float)(-(z.im[r] * wa[r].y))};
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f2{0.f, 0.f};
        }
        __syncthreads();
        stft_overlap_add(A, slots, carry, s, rd, rd >= R.rFirst, tid);
        __syncthreads();
    }
}

// ---- streaming: vp_k_pv_stream_lock with the stage above.  harm: a record of its own (VP_HZ_*, vp_stft.h): the previous phases, the
// sample count, history, carry and one theta array per voice, handed from the call's first live frame to its last whatever their
// wavefronts.  The call's bookkeeping is the pv_call_* helpers of vp_stft.hip.  ratioTab [nBlocks][S][V]; gainTab [S][V] or null (1);
// dryTab [S] or null (0)
__global__ __launch_bounds__(64 * NWV) void vp_k_hz_stream(VpPvArgs A, const double *ratioTab, const double *gainTab, const double *dryTab, int V)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x;
    constexpr int N = 512, F = 1024, nb = N + 1;
    const int hop = A.hop, O = A.O, NB = A.N, S = A.S;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;
    lds_f32 *ring = (lds_f32 *)smem + NWV * 2048;                              // [VP_PV_RING]
    lds_f32 *hist = ring + VP_PV_RING;                                         // [F]
    const PvLds pv = pv_lds_carve((lds_f64 *)(hist + F), wv);
    const PvLockLds lk = pv_lock_carve((lds_f64 *)smem + pv_stream_lds_bytes() / 8, wv);
    lds_f64 *thetaX = (lds_f64 *)smem + (pv_stream_lds_bytes() + pv_lock_lds_bytes()) / 8;   // harm: [3][513], voices 1 .. 3
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)((pv_stream_lds_bytes() + pv_lock_lds_bytes() + hz_lds_bytes()) / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
    __syncthreads();
#endif
    unsigned char *rec = A.state + (size_t)s * VP_HZ_REC_BYTES;                // harm:
    double *recD = (double *)rec, *recTheta = (double *)(rec + VP_HZ_THETA_BYTES);
    float *recHist = (float *)(rec + VP_HZ_HIST_BYTES), *recCarry = (float *)(rec + VP_HZ_CARRY_BYTES);

    double noRatio = 0.0;                                                      // harm: the record holds no ratio; the updates are resets
    long long n = ((const long long *)recD)[VP_HZ_COUNT];
    const bool rst = pv_scan_updates(A, s, noRatio);
    if (rst) n = 0;
    const PvCall C = pv_call_geometry(n, A.nBlocks * NB, hop, A.L);
    const int nf = C.nf;

    pv_call_load_hist(C, hist, recHist, tid);
    for (int i = tid; i < nb; i += 64 * NWV) { pv.phPrev[i] = rst ? 0.0 : recD[i]; pv.sum[i] = rst ? 0.0 : recTheta[i]; }
    for (int i = tid; i < HZ_EXTRA_THETA * nb; i += 64 * NWV) thetaX[i] = rst ? 0.0 : recTheta[nb + i];   // harm:
    pv_call_load_ring(C, ring, recCarry, rst, tid);

    FftLane Lf;
    fft_lane_init(Lf, lane, A.tw1, A.tw2);
    d2 wa[8];
    d2 ws[4];
#pragma unroll
    for (int r = 0; r < 8; r++) wa[r] = ((const d2 *)A.win)[lane + 64 * r];
#pragma unroll
    for (int q = 0; q < 4; q++) ws[q] = ((const d2 *)A.tws)[lane * 4 + q];
    const bool lane0 = lane == 0;
    // harm: the stream's gains, once
    double gn[VP_HARM_MAX_VOICES];
#pragma unroll
    for (int v = 0; v < VP_HARM_MAX_VOICES; v++) gn[v] = (v < V && gainTab) ? hz_gain(gainTab[(size_t)s * V + v]) : 1.0;
    const double dry = dryTab ? hz_gain(dryTab[s]) : 0.0;
    __syncthreads();

    const float *xs = A.in + (size_t)s * NB;
    float *ys = A.out + (size_t)s * NB;
    const int nRounds = pv_call_rounds(C);
    int cb = C.er;
    f2 xv[8];
    double rq[VP_HARM_MAX_VOICES];
#pragma unroll
    for (int v = 0; v < VP_HARM_MAX_VOICES; v++) rq[v] = 1.0;
    auto request = [&](int k_) {
        const int fr_ = C.fr0 + NWV * k_ + wv;
        if (k_ < nRounds && fr_ >= 0 && fr_ < nf) {
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int rel = fr_ * hop + 2 * (lane + 64 * r);
                xv[r] = f2{pv_call_sample(C, hist, xs, NB, S, rel), pv_call_sample(C, hist, xs, NB, S, rel + 1)};
            }
            const unsigned blk = (unsigned)(fr_ * hop + F - 1 - C.H) / (unsigned)NB; // the block in which the frame's last sample arrives
#pragma unroll
            for (int v = 0; v < VP_HARM_MAX_VOICES; v++) if (v < V) rq[v] = ratioTab[((size_t)blk * S + s) * V + v];   // harm:
        }
    };
    request(0);
    for (int k = 0; k < nRounds; k++) {
        const int frW0 = C.fr0 + NWV * k;
        const int fr = frW0 + wv;
        const bool live = fr >= 0 && fr < nf;                                  // (wavefront-uniform)
        const int wFirst = max(0, -frW0), wLast = min(NWV - 1, nf - 1 - frW0);
        C8 z;
        RPairs X;
        double rr[VP_HARM_MAX_VOICES];
#pragma unroll
        for (int v = 0; v < VP_HARM_MAX_VOICES; v++) rr[v] = pv_curve_clamp(rq[v]);
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; r++) { z.re[r] = (double)xv[r].x * wa[r].x; z.im[r] = (double)xv[r].y * wa[r].y; }
        }
        request(k + 1);
        if (live) {
            fft512_rx(z, xb, Lf);
            rfft_split(z, xb, lane, (const d2 *)ws, X);
        }
        {
            // ---- harm: the stage (vp_k_stft_harm's), to the merge
            const double invO = 1.0 / (double)O;
            const int prevSlot = wv == wFirst ? 0 : wv;
            int ln = lane;
            asm volatile("" : "+v"(ln));
            if (live) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int k_ = 64 * q + ln, m = N - k_;
                    pv.ana[k_] = d2{X.kr[q], X.ki[q]}; pv.ana[m] = d2{X.mr[q], X.mi[q]};
                    pv.inc[wv * nb + k_] = sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]); pv.phPrev[(wv + 1) * nb + k_] = pv_phase_turns(X.ki[q], X.kr[q]);
                    pv.inc[wv * nb + m] = sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]); pv.phPrev[(wv + 1) * nb + m] = pv_phase_turns(X.mi[q], X.mr[q]);
                }
                if (lane0) {
                    pv.ana[N / 2] = d2{X.hr, X.hi};
                    pv.inc[wv * nb + N / 2] = sqrt(X.hr * X.hr + X.hi * X.hi); pv.phPrev[(wv + 1) * nb + N / 2] = pv_phase_turns(X.hi, X.hr);
                }
                hz_dry(X, dry);                                                // harm: X is the sum from here on
            }
            __syncthreads();
            int own[9];
            bool has = false;
            if (live) has = hz_analyse(pv, lk, wv, prevSlot, ln, lane0, invO, O, own);
            // harm: every voice's theta continues from the state at the call's first live frame and is left by its last
#pragma nounroll
            for (int v = 0; v < V; v++) {
                const double ratio = hz_pick(rr, v), g = hz_pick(gn, v);
                lds_f64 *theta = v == 0 ? pv.sum : thetaX + (v - 1) * nb;
                int src[9], pk[9];
                double th[9];
#pragma unroll
                for (int e = 0; e < 9; e++) { src[e] = -1; pk[e] = 0; th[e] = 0.0; }
                if (live && has) hz_voice_plan(lk, ln, lane0, ratio, src, pk);
#pragma unroll
                for (int w = 0; w < NWV; w++) {
                    if (w > 0) __syncthreads();
                    if (live && has && wv == w) hz_turn(theta, pv, wv, ln, lane0, ratio, invO, own, src, pk, th);
                }
                if (live && has) hz_gather_add(pv, lane0, src, th, g, X);
            }
            if (live && wv == wLast) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int k_ = pv_lock_bin(e, ln);
                    pv.phPrev[k_] = pv.phPrev[(wv + 1) * nb + k_];
                }
            }
            // ---- harm: end of the stage
        }
        lds_f2 *slot = (lds_f2 *)(slots + wv * 2048);
        if (live) {
            rfft_merge_conj(z, xb, lane, (const d2 *)ws, X, A.c);
            fft512_rx(z, xb, Lf);
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f2{(float)(z.re[r] * wa[r].x), (float)(-(z.im[r] * wa[r].y))};
        }
        __syncthreads();
        cb = pv_call_round_tail(C, ring, slots, ys, NB, S, hop, frW0, wFirst, wLast, cb, tid);
        __syncthreads();
    }
    pv_call_emit(C, ring, ys, NB, S, cb, C.er + C.M, tid);                     // the flush

    pv_call_store_hist(C, recHist, hist, xs, NB, S, hop, tid);
    pv_call_store_carry(C, recCarry, ring, tid);
    __syncthreads();
    for (int i = tid; i < nb; i += 64 * NWV) { recD[i] = pv.phPrev[i]; recTheta[i] = pv.sum[i]; }
    for (int i = tid; i < HZ_EXTRA_THETA * nb; i += 64 * NWV) recTheta[nb + i] = thetaX[i];   // harm:
    if (tid == 0) ((long long *)recD)[VP_HZ_COUNT] = C.R;
}

// the pending resets alone (a call with more than VP_PV_MAX_UPDATES of them enqueues this first, on the same stream)
__global__ __launch_bounds__(256) void vp_k_hz_update(VpPvArgs A)
{
    const int s = blockIdx.x;
    unsigned char *rec = A.state + (size_t)s * VP_HZ_REC_BYTES;
    double *recD = (double *)rec, *recTheta = (double *)(rec + VP_HZ_THETA_BYTES);
    double noRatio = 0.0;
    if (!pv_scan_updates(A, s, noRatio)) return;
    float *recCarry = (float *)(rec + VP_HZ_CARRY_BYTES);
    for (int i = threadIdx.x; i < VP_PV_NB; i += 256) recD[i] = 0.0;
    for (int i = threadIdx.x; i < VP_HARM_MAX_VOICES * VP_PV_NB; i += 256) recTheta[i] = 0.0;
    for (int i = threadIdx.x; i < 1024; i += 256) recCarry[i] = 0.f;
    if (threadIdx.x == 0) ((long long *)recD)[VP_HZ_COUNT] = 0;
}

hipError_t vp_stft_harm_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_stft_harm, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

size_t vp_stft_harm_lds_bytes(int hop) { return vp_stft_lock_lds_bytes(hop) + hz_lds_bytes(); }
size_t vp_hz_lds_bytes() { return vp_pv_lock_lds_bytes() + hz_lds_bytes(); }

hipError_t vp_stft_launch_harm(const VpStftArgs &a, const double *d_ratio, const double *d_gain, const double *d_dry, int nVoices, int nStreams, hipStream_t st)
{
    const dim3 grid(1, nStreams), block(64 * NWV);                             // (one run: every theta is a recurrence over the stream's frames)
    hipLaunchKernelGGL(vp_k_stft_harm, grid, block, vp_stft_harm_lds_bytes(a.hop), st, a, d_ratio, d_gain, d_dry, nVoices);
    return hipGetLastError();
}

hipError_t vp_hz_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_hz_stream, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_hz_launch(const VpPvArgs &a, const double *d_ratio, const double *d_gain, const double *d_dry, int nVoices, hipStream_t st)
{
    if (a.nBlocks == 0) hipLaunchKernelGGL(vp_k_hz_update, dim3(a.S), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(vp_k_hz_stream, dim3(a.S), dim3(64 * NWV), vp_hz_lds_bytes(), st, a, d_ratio, d_gain, d_dry, nVoices);
    return hipGetLastError();
}
