// vp_stft_stretch_lock.inc -- the PEAK-LOCKED phase-vocoder kernel with frames analysed at CALLER-GIVEN POSITIONS: the locked time stretch
// (included by vp_stft.hip behind vp_stft_stretch.inc and vp_stft_lock.inc: pv_stretch_frame, and the locked stage's carve, masks, turns and
// gather).
//
// Peak locking was introduced for time-scale modification (Laroche & Dolson 1999); vp_k_stft_pv_lock has it on the fixed grid only.  Here
// frame f of stream s is read at input sample q_f = clamp(pos[s][f], 0, nIn - F) of a row of nIn samples, as vp_k_stft_pv_stretch reads it,
// and still overlap-added at output sample f hop.  The definition is tests/pv_stretch_lock_reference.py: tests/pv_lock_reference.py's stage
// with the analysis advance D_0 = hop, D_f = clamp(q_f - q_(f-1), 1, F)
//   in the unwrap    nominal term (k D) / F (the integer product times the power of two 1 / F: exact), true frequency nu = k + d (F / D);
//   in the rotation  a partial's analysis phase advances nu D / F turns from frame to frame and the synthesis must advance r nu hop / F, so
//                    a peak's region turns by nu (r hop - D) / F more per frame (r hop is exact: hop is a power of two).
// At pos[f] = f hop the unwrap's terms are the parent's k (1 / O) and O, the rotation's factor (r hop - hop) / F is the parent's (r - 1) / O
// (a power of two apart from r - 1, which is exact on [0.5, 2]): that table gives vp_stft_pitch_shift_locked's bits (tested).
//
// vp_k_stft_pv_stretch_lock is a WRITTEN-OUT COPY of vp_k_stft_pv_lock, statement for statement, with vp_k_stft_pv_stretch's changes, and a
// kernel of its own (vp_stft_curve.inc says why copies).  What differs from vp_k_stft_pv_lock is marked "stretch:".  pv_lock_mask,
// pv_lock_nearest, pv_lock_turn, pv_lock_gather and pv_lock_carve are used as they are; pv_lock_plan has the fixed grid's unwrap and
// advance written into it, so its copy with the frame's advance stands here.  No LDS of its own: vp_stft_lock_lds_bytes(hop).

// stretch: pv_lock_plan with the frame's analysis advance `delta` (1 .. F) in the unwrap and in the peaks' advance of the angle; perDelta is
// F / delta, invF the power of two 1 / F.  Everything else is pv_lock_plan's, statement for statement.
__device__ __forceinline__ bool pv_stretch_lock_plan(const PvLds &pv, const PvLockLds &lk, int wv, int prevSlot, int ln, bool lane0, double ratio, int delta, int hop,
                                                     double invF, double perDelta, int (&own)[9], int (&src)[9], int (&pk)[9])
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
    for (int e = 0; e < 9; e++) { own[e] = 0; src[e] = -1; pk[e] = 0; }
    if (any == 0ull) return false;                                             // (all zeros, or nothing finite: the frame is silent)
    pv_lock_mask(lk.peaks, bal, lane0);
#pragma unroll
    for (int e = 0; e < 9; e++) if (e < 8 || lane0) lk.back[pv_lock_bin(e, ln)] = -1;
    wave_sync();                                                               // (and every lane has read its magnitudes)
    const double turn = ((ratio * (double)hop) - (double)delta) * invF;        // stretch: (r hop - D) / F; r hop is exact, at D = hop (r - 1) / O
#pragma unroll
    for (int e = 0; e < 9; e++) {
        if (!isPk[e]) continue;
        const int k = pv_lock_bin(e, ln);
        double d = pv.phPrev[(wv + 1) * nb + k] - pv.phPrev[prevSlot * nb + k] - (double)(k * delta) * invF;   // stretch: the exact (k D) / F
        d -= rint(d);
        const double nu = (double)k + d * perDelta;                            // stretch: where the parent has O
        mrow[k] = nu * turn;                                                   // stretch: the synthesis advances r nu hop / F, the analysis nu D / F
        const int kp = (int)floor((double)k * ratio + 0.5);
        if (kp <= N) lk.back[kp] = k;                                          // (peaks are three bins apart: distinct for r >= 0.5)
    }
    wave_sync();
#pragma unroll
    for (int e = 0; e < 9; e++) {
        const int k = pv_lock_bin(e, ln);
        bal[e] = __ballot((e < 8 || lane0) && lk.back[k] >= 0);
        own[e] = pv_lock_nearest(lk.peaks, k);
        if (e < 8 || lane0) lk.own[k] = own[e];
    }
    any = 0ull;
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
    return true;
}

__global__ __launch_bounds__(64 * NWV) void vp_k_stft_pv_stretch_lock(VpStftArgs A, const double *ratioTab, const int *posTab, int nIn)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 512;                                                     // complex points = F / 2
    const int F = A.F, hop = A.hop;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;
    lds_f32 *carry = (lds_f32 *)smem + NWV * 2048;                             // [(O - 1) hop]
    const PvLds pv = pv_lds_carve((lds_f64 *)smem + stft_lds_base(F, hop) / 8, wv);
    const PvLockLds lk = pv_lock_carve((lds_f64 *)smem + (stft_lds_base(F, hop) + pv_lds_bytes()) / 8, wv);
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)((stft_lds_base(F, hop) + pv_lds_bytes() + pv_lock_lds_bytes()) / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
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
    __syncthreads();

    const StftRun R = stft_run(A, run);
    const float *xs = A.in + (size_t)s * nIn;                                  // stretch: the input row is nIn samples, the output row T
    const double *rs = ratioTab + (size_t)s * A.nFrames;
    const int *ps = posTab + (size_t)s * A.nFrames;                            // stretch: the stream's row
    const int qMax = nIn - F;
    // the frame's samples, its ratio, and (stretch:) its position and advance are requested a round ahead
    f2 xv[8];
    double rq = 1.0;
    int dq = hop;
    auto request = [&](int rd_) {
        const int f_ = rd_ * NWV + wv;
        if (rd_ < R.r1 && f_ < A.nFrames) {
            int q_;
            pv_stretch_frame(ps, f_, qMax, hop, F, q_, dq);
            const float *x_ = xs + q_;                                         // stretch: in [xs, xs + nIn - F]
            stft_load_frame(xv, x_, ((uintptr_t)x_ & 7) == 0, lane);           // stretch: (float2 loads when THIS frame is 8-byte aligned)
            rq = rs[f_];
        }
    };
    request(R.r0);
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        C8 z;
        RPairs X;
        const double ratio = pv_curve_clamp(rq);
        const int delta = dq;                                                  // stretch: this frame's analysis advance (wavefront-uniform), 1 .. F
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
            // ---- the peak-locked stage, phases in TURNS (to the merge): vp_k_stft_pv_lock's, with the frame's advance in the plan
            const int nb = N + 1;
            const double invF = 1.0 / (double)F;                               // stretch: (k delta) invF is the exact quotient (F a power of two)
            const double perDelta = (double)F / (double)delta;                 // stretch: where the parent has O (one uniform division)
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
            }
            __syncthreads();
            int own[9], src[9], pk[9];
            bool has = false;
            if (live) has = pv_stretch_lock_plan(pv, lk, wv, wv, ln, lane0, ratio, delta, hop, invF, perDelta, own, src, pk);   // stretch:
            // theta is handed through the round in frame order, in place
            double th[9];
#pragma unroll
            for (int e = 0; e < 9; e++) th[e] = 0.0;
#pragma unroll
            for (int w = 0; w < NWV; w++) {
                if (w > 0) __syncthreads();
                if (live && has && wv == w) pv_lock_turn(pv, wv, ln, lane0, own, src, pk, th);
            }
            if (live) pv_lock_gather(pv, lane0, src, th, X);
            // (every live wavefront is past its reads of the previous frame's phases: the turns' barriers, or program order when the
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
            // ---- end of the stage
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

hipError_t vp_stft_stretch_lock_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_stft_pv_stretch_lock, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_stft_launch_stretch_lock(const VpStftArgs &a, const double *d_ratio, const int *d_pos, int nIn, int nStreams, hipStream_t st)
{
    const dim3 grid(1, nStreams), block(64 * NWV);                             // (one run: theta is a recurrence over the stream's frames)
    hipLaunchKernelGGL(vp_k_stft_pv_stretch_lock, grid, block, vp_stft_lock_lds_bytes(a.hop), st, a, d_ratio, d_pos, nIn);
    return hipGetLastError();
}
