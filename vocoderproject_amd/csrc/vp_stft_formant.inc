// vp_stft_formant.inc -- the ratio-curve phase-vocoder kernels with a FORMANT correction (included at the end of vp_stft.hip: its helpers,
// tables and carves, and vp_stft_curve.inc's pv_curve_clamp).
//
// vp_k_stft_pv_curve and vp_k_pv_stream_curve move every bin to round(k ratio) with its magnitude: the spectral envelope -- the vocal
// tract's formants -- is transposed with the pitch.  The builds below estimate the frame's envelope from the magnitudes the stage already
// holds and scale each synthesis bin by the envelope at the bin's own position (divided by the stream's formant ratio phi) over the
// envelope at the position its content came from (divided by the frame's pitch ratio r).  The definition is tests/pv_formant_reference.py:
//     L[k]  = 0.5 log(m[k]^2 + 1e-12)                                     k = 0 .. 512
//     c     = irfft(L, 1024), liftered: c[n] kept for n < nc, halved at n = nc, dropped beyond (symmetric)
//     le    = rfft(c).real                                                the smoothed log envelope
//     at(rho)[kk] = le interpolated linearly at clip(kk / rho, 0, 512)
//     sm[kk] *= exp(clip(at(phi)[kk] - at(r)[kk], -ln 16, ln 16))
// phi = 1 (a null table) keeps the formants where they were; phi = r gives the curve kernel's bits (the exponent is exactly 0).  The
// correction has no state across frames: the streaming record, the latency and the call bookkeeping are vp_k_pv_stream_curve's.
//
// They are WRITTEN-OUT COPIES of the two curve kernels, statement for statement, and kernels of their own (tests/test_kernel_resources.py
// and tests/test_stft_parts_cpu.py look the parents up by name).  What differs is marked "formant:" -- the envelope, the gain, and
// where the twiddles live: the envelope's two transforms and the gain's reads are live on top of everything the parents keep, and with
// the transform's and the split's twiddles resident (80 registers) the builds need 256 + 171 registers; read from the global tables where
// they are used, as vp_k_stft_pv2k reads them, they need 256 + 111 and 256 + 104.  The values are the same, so are the bits.
//
// The envelope is work of one wavefront on its own frame, between the write of pv.ana[k] and the gather, with wave_sync() only.  L and
// the liftered cepstrum are real EVEN sequences of 1024 samples: laid out mirrored in the wavefront's exchange buffer (exactly 1024
// doubles, free between rfft_split and rfft_merge_conj) and read back as z[n] = (v[2n], v[2n + 1]), n = lane + 64 r, they go through the
// kernel's own forward transform and split; the result is real, and for an even sequence the inverse transform is the forward one over
// 1024.  The 513 values of le are then parked in the same buffer for the gather's interpolated reads: a wavefront's LDS operations
// execute in order, and the merge writes the buffer only after the gather.  No LDS of its own: the launchers pass the parents' sizes.
// Every index into the buffer is a bin in [0, 512] or its mirror (1024 - k) & 1023.

#define VP_PV_LN16 2.772588722239781          // the gain's clamp: +-24 dB

// formant: v[e], the lanes' nine bins kb[e] of a real even sequence's samples 0 .. 512 -> the real parts of its forward transform, same layout
__device__ __forceinline__ void pv_even_rfft(double (&v)[9], const int (&kb)[9], bool lane0, int lane, lds_d2 *xb, const FftAddr &L, const d2 *tw1p, const d2 *tw2p, const d2 *ws)
{
    lds_f64 *xl = (lds_f64 *)xb;
    wave_sync();
#pragma unroll
    for (int e = 0; e < 9; e++) {
        if (e == 8 && !lane0) continue;
        xl[kb[e]] = v[e];
        xl[(1024 - kb[e]) & 1023] = v[e];                                       // the mirror (bins 0 and 512 are their own)
    }
    wave_sync();
    C8 z;
    RPairs X;
#pragma unroll
    for (int r = 0; r < 8; r++) { const d2 t = xb[lane + 64 * r]; z.re[r] = t.x; z.im[r] = t.y; }
    fft512_rx(z, xb, L, tw1p, tw2p);
    rfft_split(z, xb, lane, ws, X);
#pragma unroll
    for (int q = 0; q < 4; q++) { v[2 * q] = X.kr[q]; v[2 * q + 1] = X.mr[q]; }
    v[8] = X.hr;
}

// formant: the smoothed log envelope of the frame whose magnitudes are mg[e], left as xl[0 .. 512] in the wavefront's exchange buffer
__device__ __forceinline__ void pv_formant_envelope(const double (&mg)[9], const int (&kb)[9], bool lane0, int lane, int nc, lds_d2 *xb, const FftAddr &L,
                                                    const d2 *tw1p, const d2 *tw2p, const d2 *ws)
{
    lds_f64 *xl = (lds_f64 *)xb;
    double v[9];
#pragma unroll
    for (int e = 0; e < 9; e++) v[e] = 0.5 * log(mg[e] * mg[e] + 1e-12);
    pv_even_rfft(v, kb, lane0, lane, xb, L, tw1p, tw2p, ws);                                // 1024 c[n], n = kb[e]
#pragma unroll
    for (int e = 0; e < 9; e++) v[e] *= (kb[e] < nc ? 1.0 : kb[e] == nc ? 0.5 : 0.0) * (1.0 / 1024.0);
    pv_even_rfft(v, kb, lane0, lane, xb, L, tw1p, tw2p, ws);                                // le[k], k = kb[e]
    wave_sync();
#pragma unroll
    for (int e = 0; e < 9; e++) if (e < 8 || lane0) xl[kb[e]] = v[e];
    wave_sync();
}

// formant: exp(clip(at(phi)[kk] - at(r)[kk])) from the envelope in xl; the four interpolation points are requested together
__device__ __forceinline__ double pv_formant_gain(const lds_f64 *xl, int kk, double invPhi, double invRatio)
{
    constexpr int N = 512;
    const double sa = fmin(fmax((double)kk * invPhi, 0.0), (double)N), sb = fmin(fmax((double)kk * invRatio, 0.0), (double)N);
    const int ia = min((int)sa, N - 1), ib = min((int)sb, N - 1);
    const double a0 = xl[ia], a1 = xl[ia + 1], b0 = xl[ib], b1 = xl[ib + 1];
    const double ea = __builtin_fma(sa - (double)ia, a1 - a0, a0), eb = __builtin_fma(sb - (double)ib, b1 - b0, b0);
    return exp(fmin(fmax(ea - eb, -VP_PV_LN16), VP_PV_LN16));
}

__global__ __launch_bounds__(64 * NWV) void vp_k_stft_pv_formant(VpStftArgs A, const double *ratioTab, const double *formantTab, int nc)
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

    // formant: the transform's and the split's twiddles come from the global tables where they are used, as in vp_k_stft_pv2k (L1 / L2-resident;
    // resident in registers they are 80 more of them, and the envelope's two transforms need the room)
    FftAddr L;
    fft_addr_init(L, lane);
    const d2 *tw1p = (const d2 *)A.tw1 + lane * 8, *tw2p = (const d2 *)A.tw2 + lane * 8;
    d2 wa[8];                                                                  // (w[2n], w[2n + 1]), n = lane + 64 r
#pragma unroll
    for (int r = 0; r < 8; r++) wa[r] = ((const d2 *)A.win)[lane + 64 * r];
    const d2 *ws = (const d2 *)A.tws + lane * 4;                               // formant: W_1024^(64 q + lane), from the global table
    const bool lane0 = lane == 0;
    // formant: the stream's formant ratio (a null table: 1) as the stage uses it, and the wavefront's exchange buffer as 1024 doubles
    const double invPhi = 1.0 / (formantTab ? pv_curve_clamp(formantTab[s]) : 1.0);
    lds_f64 *xl = (lds_f64 *)xb;

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
            fft512_rx(z, xb, L, tw1p, tw2p);
            rfft_split(z, xb, lane, ws, X);
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
                pv_formant_envelope(mg, kb, lane0, lane, nc, xb, L, tw1p, tw2p, ws);       // formant: le[0 .. 512] in xl
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
                // formant: the envelope at the bin over the envelope where its content came from, in a loop of its own (its LDS requests
                // in flight together with the gather's forty-five cost 90 registers)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    mg[e] *= pv_formant_gain(xl, kb[e], invPhi, invRatio);
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
            rfft_merge_conj(z, xb, lane, ws, X, A.c);
            fft512_rx(z, xb, L, tw1p, tw2p);
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

// ---- streaming: vp_k_pv_stream_curve with the formant correction; ratioTab [nBlocks][S] as there, formantTab [S].  The call's bookkeeping
// is written out, as there (the comment there says why).
__global__ __launch_bounds__(64 * NWV) void vp_k_pv_stream_formant(VpPvArgs A, const double *ratioTab, const double *formantTab, int nc)
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

    // formant: the transform's and the split's twiddles come from the global tables where they are used, as in vp_k_stft_pv2k (L1 / L2-resident;
    // resident in registers they are 80 more of them, and the envelope's two transforms need the room)
    FftAddr Lf;
    fft_addr_init(Lf, lane);
    const d2 *tw1p = (const d2 *)A.tw1 + lane * 8, *tw2p = (const d2 *)A.tw2 + lane * 8;
    d2 wa[8];
#pragma unroll
    for (int r = 0; r < 8; r++) wa[r] = ((const d2 *)A.win)[lane + 64 * r];
    const d2 *ws = (const d2 *)A.tws + lane * 4;                               // formant: W_1024^(64 q + lane), from the global table
    const bool lane0 = lane == 0;
    // formant: the stream's formant ratio (a null table: 1) as the stage uses it, and the wavefront's exchange buffer as 1024 doubles
    const double invPhi = 1.0 / (formantTab ? pv_curve_clamp(formantTab[s]) : 1.0);
    lds_f64 *xl = (lds_f64 *)xb;
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
            fft512_rx(z, xb, Lf, tw1p, tw2p);
            rfft_split(z, xb, lane, ws, X);
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
                pv_formant_envelope(mg, kb, lane0, lane, nc, xb, Lf, tw1p, tw2p, ws);       // formant: le[0 .. 512] in xl
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
                // formant: the envelope at the bin over the envelope where its content came from, in a loop of its own (its LDS requests
                // in flight together with the gather's forty-five cost 90 registers)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    mg[e] *= pv_formant_gain(xl, kb[e], invPhi, invRatio);
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
            rfft_merge_conj(z, xb, lane, ws, X, A.c);
            fft512_rx(z, xb, Lf, tw1p, tw2p);
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

hipError_t vp_stft_formant_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_stft_pv_formant, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

// (1024-point frames only: the caller's test)
hipError_t vp_stft_launch_formant(const VpStftArgs &a, const double *d_ratio, const double *d_formant, int nc, int nStreams, hipStream_t st)
{
    const size_t lds = vp_stft_lds_bytes(a.F, a.hop, 0);
    const dim3 grid(1, nStreams), block(64 * NWV);
    hipLaunchKernelGGL(vp_k_stft_pv_formant, grid, block, lds + pv_lds_bytes(), st, a, d_ratio, d_formant, nc);
    return hipGetLastError();
}

hipError_t vp_pv_formant_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_pv_stream_formant, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_pv_launch_formant(const VpPvArgs &a, const double *d_ratio, const double *d_formant, int nc, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_pv_stream_formant, dim3(a.S), dim3(64 * NWV), vp_pv_lds_bytes(), st, a, d_ratio, d_formant, nc);
    return hipGetLastError();
}
