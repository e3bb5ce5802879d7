// vp_stft_curve.inc -- the phase-vocoder kernels along a RATIO CURVE (included at the end of vp_stft.hip: its helpers, tables and carves).
//
// vp_k_stft_fused<true, false>, vp_k_stft_pv2k and vp_k_pv_stream take one pitch ratio per launch (per stream in the streaming kernel).
// The builds below read it per frame: the one-shot ones from a table [S][nFrames], the streaming one from a table [nBlocks][S] (a frame
// takes the ratio of the block in which its last sample arrives).  The definition is tests/stft_reference.py's with `ratio` replaced by
// ratio[s][f] in frame f (tests/pv_stream_reference.py: "the ratio schedule is per frame"): the analysis, the previous-frame phases, the
// accumulator's rounds and the overlap-add do not depend on the ratio; what does -- 1 / ratio, the candidates' centre, their tests and
// the frequency scaling -- already sits inside the round loop.
//
// They are WRITTEN-OUT COPIES of the three kernels, statement for statement, and kernels of their own: tests/test_kernel_resources.py
// looks the parents up by name, and one stage shared as a function cost the one-shot 2 % (docs/HISTORY.md, "One phase-vocoder stage for
// both kernels").  What differs is marked "curve:".  The operations per bin and their order are the parents', so a curve that is constant
// per stream gives the parent's bits (tested).
//
// The ratio of a wavefront's frame is one uniform value: it is requested with the frame's samples (a round ahead where the parent requests
// those a round ahead) and used clamped to [0.5, 2] -- fmax first, so a NaN becomes 0.5; the gather clamps its indices anyway.  No LDS of
// its own.

// curve: the table's value as the stage uses it
__device__ __forceinline__ double pv_curve_clamp(double r) { return fmin(fmax(r, 0.5), 2.0); }

__global__ __launch_bounds__(64 * NWV) void vp_k_stft_pv_curve(VpStftArgs A, const double *ratioTab)
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
    const float *xs = A.in + (size_t)s * T;
    const double *rs = ratioTab + (size_t)s * A.nFrames;                       // curve: the stream's row
    // the frame's samples, and its ratio, are requested a round ahead
    f2 xv[8];
    double rq = 1.0;
    auto request = [&](int rd_) {
        const int f_ = rd_ * NWV + wv;
        if (rd_ < R.r1 && f_ < A.nFrames) { stft_load_frame(xv, xs + (size_t)f_ * hop, A.aligned, lane); rq = rs[f_]; }
    };
    request(R.r0);
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        C8 z;
        RPairs X;
        const double ratio = pv_curve_clamp(rq);                               // curve: this frame's (wavefront-uniform)
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
            // ---- phase-vocoder stage, phases in TURNS: vp_k_stft_fused<true, false>'s, with the frame's ratio
            const int nb = N + 1;
            const double invO = 1.0 / (double)O;
            const double invRatio = 1.0 / ratio;
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
                    double d = ph[e] - pv.phPrev[wv * nb + k] - (double)k * invO;
                    d -= rint(d);
                    pv.ana[k] = d2{mg[e], (double)k + d * (double)O};
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
                        if (k >= 0 && k <= N && (int)floor((double)k * ratio + 0.5) == kk) { sm += cand[c_].x; sf = cand[c_].y * ratio; }
                    }
                    mg[e] = sm;
                    pv.inc[wv * nb + kk] = sf * invO;
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

// ---- 2048-point frames: vp_k_stft_pv2k along a curve.  That kernel loads a frame's samples in the frame's own round (no registers to
// hold them a round ahead); the ratio is requested with them, two transforms in front of its first use.
__global__ __launch_bounds__(64 * NWV) void vp_k_stft_pv2k_curve(VpStftArgs A, const double *ratioTab)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 1024, nb = VP_PV2K_NB;
    const int F = A.F, hop = A.hop, O = A.O, T = A.T;
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
    const float *xs = A.in + (size_t)s * T;
    const double *rs = ratioTab + (size_t)s * A.nFrames;                       // curve: the stream's row
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) f4 lds_f4;
    const double invO = 1.0 / (double)O;
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        const int lastLive = min(NWV - 1, A.nFrames - 1 - rd * NWV);
        lds_f4 *slot = (lds_f4 *)(slots + wv * 2048);
        C8 e;
        double hr[8], hi[8];
        RPairsN<8> X;
        double rq = 1.0;                                                       // curve: this frame's ratio (wavefront-uniform)
        if (live) {
            const float *x = xs + (size_t)f * hop;
            rq = rs[f];
            C8 o;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int m = lane + 64 * r;
                f4 v;
                if (A.aligned) v = *(const f4 *)(x + 4 * m);
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
        const double ratio = pv_curve_clamp(rq);
        const double invRatio = 1.0 / ratio;
        // (the lane number through a register the compiler cannot see through: vp_k_stft_pv2k)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        double mg[17], sp[17];
        if (live) {
#pragma unroll
            for (int b = 0; b < 17; b++) {
                if (b == 16 && !lane0) continue;
                const int k = pv2k_bin(b, ln);
                double d = phPrev[(wv + 1) * nb + k] - phPrev[wv * nb + k] - (double)k * invO;
                d -= rint(d);
                an[2 * k + 1] = (double)k + d * (double)O;
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
                    if (k >= 0 && k <= N && (int)floor((double)k * ratio + 0.5) == kk) { sm += cand[c_].x; sf = cand[c_].y * ratio; }
                }
                mg[b] = sm;
                sp[b] = sf * invO;
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

// ---- streaming: vp_k_pv_stream with one ratio per block and stream, ratioTab [nBlocks][S].  Relative frame fr of the call ends at
// relative sample fr hop + F - 1 >= H (it was not complete before the call), that is in block (fr hop + F - 1 - H) / N < nBlocks.  The
// record's ratio -- the interval of the plain calls -- is carried through with the call's pending changes applied, as the plain kernel
// does, but no frame of this call uses it.  The call's bookkeeping is WRITTEN OUT here (and in the lock and formant builds), statement for
// statement what the pv_call_* helpers of vp_stft.hip hold for the other four streaming kernels: through the helpers this kernel ran 1.2 %
// slower at unchanged registers (docs/HISTORY.md, "One copy of the streaming call's bookkeeping").
__global__ __launch_bounds__(64 * NWV) void vp_k_pv_stream_curve(VpPvArgs A, const double *ratioTab)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x;
    constexpr int N = 512, F = 1024, nb = N + 1, RM = VP_PV_RING - 1;
    const int hop = A.hop, O = A.O, L = A.L, NB = A.N, S = A.S;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;
    lds_f32 *ring = (lds_f32 *)smem + NWV * 2048;                              // [VP_PV_RING]
    lds_f32 *hist = ring + VP_PV_RING;                                         // [F]
    const PvLds pv = pv_lds_carve((lds_f64 *)(hist + F), wv);
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)(pv_stream_lds_bytes() / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
    __syncthreads();
#endif
    unsigned char *rec = A.state + (size_t)s * VP_PV_REC_BYTES;
    double *recD = (double *)rec;
    float *recHist = (float *)(rec + VP_PV_HIST_BYTES), *recCarry = (float *)(rec + VP_PV_CARRY_BYTES);

    double recRatio = recD[VP_PV_RATIO];                                       // curve: written back, not used
    long long n = ((const long long *)recD)[VP_PV_COUNT];
    const bool rst = pv_scan_updates(A, s, recRatio);
    if (rst) n = 0;

    const int M = A.nBlocks * NB;
    const long long R = n + M;
    const long long fa = n >= F ? (n - F) / hop + 1 : 0;
    const long long fb = R >= F ? (R - F) / hop + 1 : 0;
    const int nf = (int)(fb - fa);
    const int H = (int)(n - fa * hop);
    const int er = H - L;
    const int fr0 = -(int)(fa & 3);

    for (int i = tid; i < H; i += 64 * NWV) hist[i] = recHist[i];
    for (int i = tid; i < nb; i += 64 * NWV) { pv.phPrev[i] = rst ? 0.0 : recD[i]; pv.sum[i] = rst ? 0.0 : recD[nb + i]; }
    for (int q = tid; q < VP_PV_RING; q += 64 * NWV) {
        const int i = (q - er) & RM;
        ring[q] = (i < F && !rst) ? recCarry[i] : 0.f;
    }

    FftLane Lf;
    fft_lane_init(Lf, lane, A.tw1, A.tw2);
    d2 wa[8];
    d2 ws[4];
#pragma unroll
    for (int r = 0; r < 8; r++) wa[r] = ((const d2 *)A.win)[lane + 64 * r];
#pragma unroll
    for (int q = 0; q < 4; q++) ws[q] = ((const d2 *)A.tws)[lane * 4 + q];
    const bool lane0 = lane == 0;
    __syncthreads();

    const float *xs = A.in + (size_t)s * NB;
    float *ys = A.out + (size_t)s * NB;
    auto sample = [&](int rel) -> float {
        if (rel < H) return hist[rel];
        const unsigned c = (unsigned)(rel - H), b = c / (unsigned)NB;
        return xs[(size_t)b * S * NB + (c - b * NB)];
    };
    auto emit = [&](int c, float v) {
        const unsigned b = (unsigned)c / (unsigned)NB;
        ys[(size_t)b * S * NB + ((unsigned)c - b * NB)] = v;
    };
    const int nRounds = nf > 0 ? (nf - fr0 + NWV - 1) / NWV : 0;
    int cb = er;
    f2 xv[8];
    double rq = 1.0;
    auto request = [&](int k_) {
        const int fr_ = fr0 + NWV * k_ + wv;
        if (k_ < nRounds && fr_ >= 0 && fr_ < nf) {
#pragma unroll
            for (int r = 0; r < 8; r++) { const int rel = fr_ * hop + 2 * (lane + 64 * r); xv[r] = f2{sample(rel), sample(rel + 1)}; }
            const unsigned blk = (unsigned)(fr_ * hop + F - 1 - H) / (unsigned)NB;   // curve: the block in which the frame's last sample arrives
            rq = ratioTab[(size_t)blk * S + s];
        }
    };
    request(0);
    for (int k = 0; k < nRounds; k++) {
        const int frW0 = fr0 + NWV * k;
        const int fr = frW0 + wv;
        const bool live = fr >= 0 && fr < nf;                                  // (wavefront-uniform)
        const int wFirst = max(0, -frW0), wLast = min(NWV - 1, nf - 1 - frW0);
        C8 z;
        RPairs X;
        const double ratio = pv_curve_clamp(rq);                               // curve: this frame's (wavefront-uniform)
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
            const double invO = 1.0 / (double)O;
            const double invRatio = 1.0 / ratio;
            const int prevSlot = wv == wFirst ? 0 : wv;
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
                kb[8] = N / 2; mg[8] = sqrt(X.hr * X.hr + X.hi * X.hi); ph[8] = pv_phase_turns(X.hi, X.hr);
#pragma unroll
                for (int e = 0; e < 9; e++) if (e < 8 || lane0) pv.phPrev[(wv + 1) * nb + kb[e]] = ph[e];
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int k_ = kb[e];
                    double d = ph[e] - pv.phPrev[prevSlot * nb + k_] - (double)k_ * invO;
                    d -= rint(d);
                    pv.ana[k_] = d2{mg[e], (double)k_ + d * (double)O};
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
                        const int k_ = kc - 2 + c_;
                        if (k_ >= 0 && k_ <= N && (int)floor((double)k_ * ratio + 0.5) == kk) { sm += cand[c_].x; sf = cand[c_].y * ratio; }
                    }
                    mg[e] = sm;
                    pv.inc[wv * nb + kk] = sf * invO;
                }
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int kk = kb[e];
                    double sp = pv.sum[kk];
                    for (int w = wFirst; w <= wv; w++) sp += pv.inc[w * nb + kk];
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
            if (live && wv == wLast) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    pv.phPrev[kb[e]] = pv.phPrev[(wv + 1) * nb + kb[e]];
                    pv.sum[kb[e]] = wv == NWV - 1 ? ph[e] - rint(ph[e]) : ph[e];
                }
            }
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
        const int frA = frW0 + wFirst, frB = frW0 + wLast;
        const int lo = frA * hop, hi = frB * hop + F;
        for (int j = lo + ((tid - lo) & (64 * NWV - 1)); j < hi; j += 64 * NWV) {
            float v = ring[j & RM];
            for (int w = wFirst; w <= wLast; w++) {
                const int o = j - (frW0 + w) * hop;
                if (o >= 0 && o < F) v += slots[w * 2048 + o];
            }
            ring[j & RM] = v;
        }
        const int emitEnd = min((frB + 1) * hop, er + M);
        for (int j = cb + ((tid - cb) & (64 * NWV - 1)); j < emitEnd; j += 64 * NWV) { emit(j - er, ring[j & RM]); ring[j & RM] = 0.f; }
        cb = max(cb, emitEnd);
        __syncthreads();
    }
    for (int j = cb + ((tid - cb) & (64 * NWV - 1)); j < er + M; j += 64 * NWV) { emit(j - er, ring[j & RM]); ring[j & RM] = 0.f; }

    const int Hn = H + M - nf * hop;
    for (int i = tid; i < Hn; i += 64 * NWV) recHist[i] = sample(nf * hop + i);
    const int ern = er + M;
    for (int q = tid; q < VP_PV_RING; q += 64 * NWV) {
        const int i = (q - ern) & RM;
        if (i < F) recCarry[i] = ring[q];
    }
    __syncthreads();
    for (int i = tid; i < nb; i += 64 * NWV) { recD[i] = pv.phPrev[i]; recD[nb + i] = pv.sum[i]; }
    if (tid == 0) { recD[VP_PV_RATIO] = recRatio; ((long long *)recD)[VP_PV_COUNT] = R; }
}

hipError_t vp_stft_curve_prepare_device()
{
    hipError_t e = hipFuncSetAttribute((const void *)vp_k_stft_pv_curve, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)vp_k_stft_pv2k_curve, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_stft_launch_curve(const VpStftArgs &a, const double *d_ratio, int nStreams, hipStream_t st)
{
    const size_t lds = vp_stft_lds_bytes(a.F, a.hop, 0);
    const dim3 grid(1, nStreams), block(64 * NWV);                             // (one run: the accumulator is a recurrence over the stream's frames)
    if (a.F == 2048) hipLaunchKernelGGL(vp_k_stft_pv2k_curve, grid, block, lds + pv2k_lds_bytes(), st, a, d_ratio);
    else hipLaunchKernelGGL(vp_k_stft_pv_curve, grid, block, lds + pv_lds_bytes(), st, a, d_ratio);
    return hipGetLastError();
}

hipError_t vp_pv_curve_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_pv_stream_curve, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_pv_launch_curve(const VpPvArgs &a, const double *d_ratio, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_pv_stream_curve, dim3(a.S), dim3(64 * NWV), vp_pv_lds_bytes(), st, a, d_ratio);
    return hipGetLastError();
}
