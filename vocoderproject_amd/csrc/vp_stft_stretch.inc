// vp_stft_stretch.inc -- the phase-vocoder kernels with frames analysed at CALLER-GIVEN POSITIONS: time stretch (included at the end of
// vp_stft.hip: its helpers, tables and carves).
//
// vp_k_stft_fused<true, false> and vp_k_stft_pv2k read frame f at input sample f hop and write it at output sample f hop; the unwrap's
// nominal advance k / O welds them to that grid.  The builds below read frame f of stream s at input sample q_f = clamp(pos[s][f], 0,
// nIn - F) of a row of nIn samples and still overlap-add it at output sample f hop of a row of T samples.  The definition is
// tests/pv_stretch_reference.py: tests/stft_reference.py's stage with the analysis advance Delta_0 = hop, Delta_f = clamp(q_f - q_(f-1), 1, F)
// in the unwrap -- nominal term (k Delta) / F (the integer product times the power of two 1 / F: exact), true frequency k + d (F / Delta) --
// and the synthesis increment sf / O as it was (the synthesis hop is hop).  At pos[f] = f hop both terms are the parents' k (1 / O) and O,
// the operations per bin and their order are the parents', so that table gives vp_stft_pitch_shift's bits (tested).
//
// They are WRITTEN-OUT COPIES of the two kernels, statement for statement, and kernels of their own, as the curve builds are
// (vp_stft_curve.inc says why).  What differs is marked "stretch:".
//
// q_f and q_(f-1) are two uniform loads per wavefront and frame, requested with the frame's samples (a round ahead where the parent
// requests those a round ahead); every wavefront loads its own q_(f-1), nothing is passed between wavefronts.  Positions and nIn may be
// odd: the vector load (float2 at 1024 points, float4 at 2048) is taken per frame, when that frame's address is aligned to it.  No LDS of
// their own.

// stretch: frame f's position and analysis advance from the stream's row of the table
__device__ __forceinline__ void pv_stretch_frame(const int *ps, int f, int qMax, int hop, int F, int &q, int &delta)
{
    q = min(max(ps[f], 0), qMax);
    delta = f > 0 ? min(max(q - min(max(ps[f - 1], 0), qMax), 1), F) : hop;
}

__global__ __launch_bounds__(64 * NWV) void vp_k_stft_pv_stretch(VpStftArgs A, const int *posTab, int nIn)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 512;                                                     // complex points = F / 2
    const int F = A.F, hop = A.hop, O = A.O;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;
    lds_f32 *carry = (lds_f32 *)smem + NWV * 2048;                             // [(O - 1) hop]
    const PvLds pv = pv_lds_carve((lds_f64 *)smem + stft_lds_base(F, hop) / 8, wv);
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)((stft_lds_base(F, hop) + pv_lds_bytes()) / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
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
    const int *ps = posTab + (size_t)s * A.nFrames;                            // stretch: the stream's row
    const int qMax = nIn - F;
    // the frame's samples, and its position and advance, are requested a round ahead
    f2 xv[8];
    int dq = hop;
    auto request = [&](int rd_) {
        const int f_ = rd_ * NWV + wv;
        if (rd_ < R.r1 && f_ < A.nFrames) {
            int q_;
            pv_stretch_frame(ps, f_, qMax, hop, F, q_, dq);
            const float *x_ = xs + q_;                                         // stretch: in [xs, xs + nIn - F]
            stft_load_frame(xv, x_, ((uintptr_t)x_ & 7) == 0, lane);           // (float2 loads when THIS frame is 8-byte aligned)
        }
    };
    request(R.r0);
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        C8 z;
        RPairs X;
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
            // ---- phase-vocoder stage, phases in TURNS: vp_k_stft_fused<true, false>'s, with the frame's advance in the unwrap
            const int nb = N + 1;
            const double invO = 1.0 / (double)O;
            const double invF = 1.0 / (double)F;                               // stretch: (k delta) invF is the exact quotient (F a power of two)
            const double perDelta = (double)F / (double)delta;                 // stretch: where the parent has O (one uniform division)
            const double invRatio = 1.0 / A.pvRatio;
            double ph[9];
            int kb[9];
            double mg[9];
            if (live) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    kb[2 * q] = 64 * q + lane; kb[2 * q + 1] = N - kb[2 * q];
                    mg[2 * q] = sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]); ph[2 * q] = pv_phase_turns(X.ki[q], X.kr[q]);
                    mg[2 * q + 1] = sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]); ph[2 * q + 1] = pv_phase_turns(X.mi[q], X.mr[q]);
                }
                kb[8] = N / 2; mg[8] = sqrt(X.hr * X.hr + X.hi * X.hi); ph[8] = pv_phase_turns(X.hi, X.hr);            // lane 0 only
#pragma unroll
                for (int e = 0; e < 9; e++) if (e < 8 || lane0) pv.phPrev[(wv + 1) * nb + kb[e]] = ph[e];
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int k = kb[e];
                    double d = ph[e] - pv.phPrev[wv * nb + k] - (double)(k * delta) * invF;
                    d -= rint(d);
                    pv.ana[k] = d2{mg[e], (double)k + d * perDelta};
                }
                wave_sync();
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int kk = kb[e];
                    const int kc = (int)((double)kk * invRatio);
                    double sm = 0.0, sf = 0.0;
                    d2 cand[5];
#pragma unroll
                    for (int c_ = 0; c_ < 5; c_++) cand[c_] = pv.ana[min(max(kc - 2 + c_, 0), N)];
#pragma unroll
                    for (int c_ = 0; c_ < 5; c_++) {
                        const int k = kc - 2 + c_;
                        if (k >= 0 && k <= N && (int)floor((double)k * A.pvRatio + 0.5) == kk) { sm += cand[c_].x; sf = cand[c_].y * A.pvRatio; }
                    }
                    mg[e] = sm;
                    pv.inc[wv * nb + kk] = sf * invO;                           // (the synthesis hop is hop: unchanged)
                }
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int kk = kb[e];
                    double sp = pv.sum[kk];
                    for (int w = 0; w <= wv; w++) sp += pv.inc[w * nb + kk];
                    ph[e] = sp;
                    double sn, cs;
                    pv_sincos_turns(sp, sn, cs);
                    const double re = mg[e] * cs, im = mg[e] * sn;
                    if (e == 8) { X.hr = re; X.hi = im; }
                    else if (e & 1) { X.mr[e >> 1] = re; X.mi[e >> 1] = im; }
                    else { X.kr[e >> 1] = re; X.ki[e >> 1] = im; }
                }
                if (lane0) { X.ki[0] = 0.0; X.mi[0] = 0.0; }
            }
            __syncthreads();
            const int lastLive = min(NWV - 1, A.nFrames - 1 - rd * NWV);
            if (live && wv == lastLive) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    pv.phPrev[kb[e]] = pv.phPrev[(wv + 1) * nb + kb[e]];
                    pv.sum[kb[e]] = ph[e] - rint(ph[e]);
                }
            }
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

// ---- 2048-point frames: vp_k_stft_pv2k at given positions.  That kernel loads a frame's samples in the frame's own round (no registers to
// hold them a round ahead); the two positions are requested in front of them, two transforms in front of the advance's first use.
__global__ __launch_bounds__(64 * NWV) void vp_k_stft_pv2k_stretch(VpStftArgs A, const int *posTab, int nIn)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 1024, nb = VP_PV2K_NB;
    const int F = A.F, hop = A.hop, O = A.O;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;
    lds_f32 *carry = (lds_f32 *)smem + NWV * 2048;
    lds_d2 *ana = (lds_d2 *)smem + stft_lds_base(F, hop) / 16 + (size_t)wv * nb;
    lds_f64 *an = (lds_f64 *)ana;
    lds_f64 *phPrev = (lds_f64 *)((lds_d2 *)smem + stft_lds_base(F, hop) / 16 + (size_t)NWV * nb);
    lds_f64 *sum = phPrev + (NWV + 1) * nb;
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)((stft_lds_base(F, hop) + pv2k_lds_bytes()) / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
    __syncthreads();
#endif
    FftAddr L;
    fft_addr_init(L, lane);
    const d2 *tw1p = (const d2 *)A.tw1 + lane * 8, *tw2p = (const d2 *)A.tw2 + lane * 8;
    const d2 *wtop = (const d2 *)A.twTop + lane * 8, *ws = (const d2 *)A.tws + lane * 8;
    const bool lane0 = lane == 0;
    for (int i = tid; i < F - hop; i += 64 * NWV) carry[i] = 0.f;
    for (int i = tid; i < nb; i += 64 * NWV) { phPrev[i] = 0.0; sum[i] = 0.0; }
    __syncthreads();

    const StftRun R = stft_run(A, run);
    const float *xs = A.in + (size_t)s * nIn;                                  // stretch: the input row is nIn samples, the output row T
    const int *ps = posTab + (size_t)s * A.nFrames;                            // stretch: the stream's row
    const int qMax = nIn - F;
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) f4 lds_f4;
    const double invO = 1.0 / (double)O;
    const double invF = 1.0 / (double)F;                                       // stretch: (k delta) invF is the exact quotient (F a power of two)
    const double invRatio = 1.0 / A.pvRatio;
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        const int lastLive = min(NWV - 1, A.nFrames - 1 - rd * NWV);
        lds_f4 *slot = (lds_f4 *)(slots + wv * 2048);
        C8 e;
        double hr[8], hi[8];
        RPairsN<8> X;
        int delta = hop;                                                       // stretch: this frame's analysis advance (wavefront-uniform), 1 .. F
        if (live) {
            int q_;
            pv_stretch_frame(ps, f, qMax, hop, F, q_, delta);
            const float *x = xs + q_;                                          // stretch: in [xs, xs + nIn - F]
            const bool al = ((uintptr_t)x & 15) == 0;                          // (float4 loads when THIS frame is 16-byte aligned)
            C8 o;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int m = lane + 64 * r;
                f4 v;
                if (al) v = *(const f4 *)(x + 4 * m);
                else v = f4{x[4 * m], x[4 * m + 1], x[4 * m + 2], x[4 * m + 3]};
                const d2 w0 = ((const d2 *)A.win)[2 * m], w1 = ((const d2 *)A.win)[2 * m + 1];
                e.re[r] = (double)v.x * w0.x; e.im[r] = (double)v.y * w0.y;
                o.re[r] = (double)v.z * w1.x; o.im[r] = (double)v.w * w1.y;
            }
            fft512_rx(e, xb, L, tw1p, tw2p);
            fft512_rx(o, xb, L, tw1p, tw2p);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const d2 wt = wtop[q];
                const double tr = __builtin_fma(o.re[q], wt.x, -(o.im[q] * wt.y)), ti = __builtin_fma(o.re[q], wt.y, o.im[q] * wt.x);
                hr[q] = e.re[q] - tr; hi[q] = e.im[q] - ti;
                e.re[q] += tr; e.im[q] += ti;
            }
            rfft_split_n<8>(e.re, e.im, hr, hi, xb, lane, ws, X);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int k = 64 * q + lane, m = N - k;
                an[2 * k] = sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]); phPrev[(wv + 1) * nb + k] = pv_phase_turns(X.ki[q], X.kr[q]);
                an[2 * m] = sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]); phPrev[(wv + 1) * nb + m] = pv_phase_turns(X.mi[q], X.mr[q]);
            }
            if (lane0) { an[2 * (N / 2)] = sqrt(X.hr * X.hr + X.hi * X.hi); phPrev[(wv + 1) * nb + N / 2] = pv_phase_turns(X.hi, X.hr); }
        }
        __syncthreads();
        const double perDelta = (double)F / (double)delta;                     // stretch: where the parent has O (one uniform division)
        // (the lane number through a register the compiler cannot see through: vp_k_stft_pv2k)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        double mg[17], sp[17];
        if (live) {
#pragma unroll
            for (int b = 0; b < 17; b++) {
                if (b == 16 && !lane0) continue;
                const int k = pv2k_bin(b, ln);
                double d = phPrev[(wv + 1) * nb + k] - phPrev[wv * nb + k] - (double)(k * delta) * invF;
                d -= rint(d);
                an[2 * k + 1] = (double)k + d * perDelta;
            }
            wave_sync();
#pragma unroll
            for (int b = 0; b < 17; b++) {
                if (b == 16 && !lane0) continue;
                const int kk = pv2k_bin(b, ln);
                const int kc = (int)((double)kk * invRatio);
                double sm = 0.0, sf = 0.0;
                d2 cand[5];
#pragma unroll
                for (int c_ = 0; c_ < 5; c_++) cand[c_] = ana[min(max(kc - 2 + c_, 0), N)];
#pragma unroll
                for (int c_ = 0; c_ < 5; c_++) {
                    const int k = kc - 2 + c_;
                    if (k >= 0 && k <= N && (int)floor((double)k * A.pvRatio + 0.5) == kk) { sm += cand[c_].x; sf = cand[c_].y * A.pvRatio; }
                }
                mg[b] = sm;
                sp[b] = sf * invO;                                             // (the synthesis hop is hop: unchanged)
            }
        }
#pragma unroll
        for (int w = 0; w < NWV; w++) {
            if (w > 0) __syncthreads();
            if (live && wv == w) {
#pragma unroll
                for (int b = 0; b < 17; b++) {
                    if (b == 16 && !lane0) continue;
                    const int kk = pv2k_bin(b, ln);
                    sp[b] += sum[kk];
                    sum[kk] = (w == lastLive) ? sp[b] - rint(sp[b]) : sp[b];
                }
            }
        }
        if (live) {
            if (wv == lastLive) {
#pragma unroll
                for (int b = 0; b < 17; b++) {
                    if (b == 16 && !lane0) continue;
                    const int k = pv2k_bin(b, ln);
                    phPrev[k] = phPrev[(wv + 1) * nb + k];
                }
            }
#pragma unroll
            for (int b = 0; b < 17; b++) {
                if (b == 16 && !lane0) continue;
                double sn, cs;
                pv_sincos_turns(sp[b], sn, cs);
                const double re = mg[b] * cs, im = mg[b] * sn;
                if (b == 16) { X.hr = re; X.hi = im; }
                else if (b & 1) { X.mr[b >> 1] = re; X.mi[b >> 1] = im; }
                else { X.kr[b >> 1] = re; X.ki[b >> 1] = im; }
            }
            if (lane0) { X.ki[0] = 0.0; X.mi[0] = 0.0; }
            rfft_merge_conj_n<8>(e.re, e.im, hr, hi, xb, lane, ws, X, A.c);
            C8 o;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const d2 wt = wtop[q];
                const double dr = e.re[q] - hr[q], di = e.im[q] - hi[q];
                e.re[q] += hr[q]; e.im[q] += hi[q];
                o.re[q] = __builtin_fma(dr, wt.x, -(di * wt.y)); o.im[q] = __builtin_fma(dr, wt.y, di * wt.x);
            }
            fft512_rx(e, xb, L, tw1p, tw2p);
            fft512_rx(o, xb, L, tw1p, tw2p);
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int m = lane + 64 * r;
                const d2 w0 = ((const d2 *)A.win)[2 * m], w1 = ((const d2 *)A.win)[2 * m + 1];
                slot[m] = f4{(float)(e.re[r] * w0.x), (float)(-(e.im[r] * w0.y)), (float)(o.re[r] * w1.x), (float)(-(o.im[r] * w1.y))};
            }
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        stft_overlap_add(A, slots, carry, s, rd, rd >= R.rFirst, tid);
        __syncthreads();
    }
}

hipError_t vp_stft_stretch_prepare_device()
{
    hipError_t e = hipFuncSetAttribute((const void *)vp_k_stft_pv_stretch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)vp_k_stft_pv2k_stretch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_stft_launch_stretch(const VpStftArgs &a, const int *d_pos, int nIn, int nStreams, hipStream_t st)
{
    const size_t lds = vp_stft_lds_bytes(a.F, a.hop, 0);
    const dim3 grid(1, nStreams), block(64 * NWV);                             // (one run: the accumulator is a recurrence over the stream's frames)
    if (a.F == 2048) hipLaunchKernelGGL(vp_k_stft_pv2k_stretch, grid, block, lds + pv2k_lds_bytes(), st, a, d_pos, nIn);
    else hipLaunchKernelGGL(vp_k_stft_pv_stretch, grid, block, lds + pv_lds_bytes(), st, a, d_pos, nIn);
    return hipGetLastError();
}
