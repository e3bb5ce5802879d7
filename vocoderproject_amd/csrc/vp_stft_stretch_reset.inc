// vp_stft_stretch_reset.inc -- the locked time stretch with a PHASE RESET on flagged frames: the transient-preserving stretch's second half
// (included by vp_stft.hip behind vp_stft_onset.inc, the first half, and vp_stft_stretch_lock.inc: pv_stretch_lock_plan, and through it the locked stage's carve, masks, turns
// and gather).
//
// A frame that holds an attack is synthesised by vp_k_stft_pv_stretch_lock with angles carried over from before the attack, and its
// neighbours are read D != hop apart but written hop apart: the attack leaves as a blur with pre-echo.  The standard remedy has two
// parts: the position table reads a span of frames around each onset exactly hop apart (vp_stretch_positions_transient plans it on the
// host), and the span's first frame RESTARTS the angles.  The definition is tests/pv_transient_reference.py: stretch_locked_roundtrip with
// one change in rule 4 -- on a frame with reset[s][f] != 0, th[P] = 0 for every peak P.  pprev, theta[k] = th[own[k]] and the silent frame
// (Y = 0, theta left, flagged or not) are unchanged.  At ratio 1 and D = hop the peaks' advance nu (r hop - D) / F is exactly 0, so theta
// stays 0 through the span and every region is rotated by the angle 0: the stage is the identity there and the span's frames leave with the
// input's spectrum.  In the definition that is bit for bit.  Here pv_lock_gather, used as it is, turns by pv_sincos_turns(0) =
// (0, 1 + 2^-52) -- the cosine fit's constant term --, so a bin may differ from the input's in the last place of the DOUBLE; the float32
// output behind a reset has vp_stft_roundtrip's bits on every sample the GPU test compares (tests/test_gpu_pv_transient.py).
//
// vp_k_stft_pv_stretch_lock_reset is a WRITTEN-OUT COPY of vp_k_stft_pv_stretch_lock, statement for statement, and a kernel of its own
// (vp_stft_curve.inc says why copies: the parent's registers and schedule stay what its resource test pins).  What differs is marked
// "reset:".  pv_lock_mask, pv_lock_nearest, pv_lock_turn, pv_lock_gather, pv_lock_carve and pv_stretch_lock_plan are used as they are.  No
// LDS of its own: vp_stft_lock_lds_bytes(hop).  An all-zero table gives vp_stft_time_stretch_locked's bits (tested).
//
// Out of scope: a streaming form, 2048-point frames, sub-bin offsets, single precision, resets in the pitch-shift-only calls.

// reset: a flagged frame's turn at theta (pv.sum), where pv_lock_turn stands for the others: every bin's angle is 0 -- theta[k] =
// th[own[k]] with th[P] = 0 for every peak -- and so is the angle that rotates each of the lane's synthesis bins.  Between the caller's
// barriers, in frame order, like pv_lock_turn; no lane reads what another writes.
__device__ __forceinline__ void pv_reset_turn(const PvLds &pv, int ln, bool lane0, double (&th)[9])
{
#pragma unroll
    for (int e = 0; e < 9; e++) if (e < 8 || lane0) pv.sum[pv_lock_bin(e, ln)] = 0.0;
#pragma unroll
    for (int e = 0; e < 9; e++) th[e] = 0.0;
}

__global__ __launch_bounds__(64 * NWV) void vp_k_stft_pv_stretch_lock_reset(VpStftArgs A, const double *ratioTab, const int *posTab, int nIn, const unsigned char *resetTab)
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
    const float *xs = A.in + (size_t)s * nIn;                                  // the input row is nIn samples, the output row T
    const double *rs = ratioTab + (size_t)s * A.nFrames;
    const int *ps = posTab + (size_t)s * A.nFrames;                            // the stream's row
    const unsigned char *fs = resetTab + (size_t)s * A.nFrames;                // reset: the stream's row of flags, one byte per frame
    const int qMax = nIn - F;
    // the frame's samples, its ratio, its position and advance, and (reset:) its flag are requested a round ahead
    f2 xv[8];
    double rq = 1.0;
    int dq = hop;
    int fq = 0;                                                                // reset: the requested frame's flag byte
    auto request = [&](int rd_) {
        const int f_ = rd_ * NWV + wv;
        if (rd_ < R.r1 && f_ < A.nFrames) {
            int q_;
            pv_stretch_frame(ps, f_, qMax, hop, F, q_, dq);
            const float *x_ = xs + q_;                                         // in [xs, xs + nIn - F]
            stft_load_frame(xv, x_, ((uintptr_t)x_ & 7) == 0, lane);           // (float2 loads when THIS frame is 8-byte aligned)
            rq = rs[f_];
            fq = fs[f_];                                                       // reset:
        }
    };
    request(R.r0);
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        C8 z;
        RPairs X;
        const double ratio = pv_curve_clamp(rq);
        const int delta = dq;                                                  // this frame's analysis advance (wavefront-uniform), 1 .. F
        const bool flagged = fq != 0;                                          // reset: any non-zero byte is a set flag (wavefront-uniform)
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
            // ---- the peak-locked stage, phases in TURNS (to the merge): vp_k_stft_pv_stretch_lock's, with the flagged frames' turn
            const int nb = N + 1;
            const double invF = 1.0 / (double)F;                               // (k delta) invF is the exact quotient (F a power of two)
            const double perDelta = (double)F / (double)delta;                 // where vp_k_stft_pv_lock has O (one uniform division)
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
            if (live) has = pv_stretch_lock_plan(pv, lk, wv, wv, ln, lane0, ratio, delta, hop, invF, perDelta, own, src, pk);
            // theta is handed through the round in frame order, in place
            double th[9];
#pragma unroll
            for (int e = 0; e < 9; e++) th[e] = 0.0;
#pragma unroll
            for (int w = 0; w < NWV; w++) {
                if (w > 0) __syncthreads();
                if (live && has && wv == w && flagged) pv_reset_turn(pv, ln, lane0, th);                          // reset: a flagged frame with a peak zeroes every bin's angle ...
                if (live && has && wv == w && !flagged) pv_lock_turn(pv, wv, ln, lane0, own, src, pk, th);      // reset: ... every other frame takes the parent's turn
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

hipError_t vp_stft_stretch_reset_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_stft_pv_stretch_lock_reset, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_stft_launch_stretch_lock_reset(const VpStftArgs &a, const double *d_ratio, const int *d_pos, int nIn, const unsigned char *d_reset, int nStreams,
                                             hipStream_t st)
{
    const dim3 grid(1, nStreams), block(64 * NWV);                             // (one run: theta is a recurrence over the stream's frames)
    hipLaunchKernelGGL(vp_k_stft_pv_stretch_lock_reset, grid, block, vp_stft_lock_lds_bytes(a.hop), st, a, d_ratio, d_pos, nIn, d_reset);
    return hipGetLastError();
}
