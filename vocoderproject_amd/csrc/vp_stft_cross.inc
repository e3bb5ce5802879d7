// vp_stft_cross.inc -- STFT CROSS-SYNTHESIS: the spectral envelope of one signal (the voice) imposed on another (the carrier).  Included
// by vp_stft.hip in front of vp_stft_formant.inc: its helpers, tables and run arithmetic.  No reference counterpart (the reference's vocoder
// is the LPC cross-synthesis behind vp_process_block*; SURVEY.md section 0) -- the definition is tests/pv_cross_reference.py:
//     V = rfft(w v_frame),  C = rfft(w c_frame)                            frames, window, scale and overlap-add of the plain round trip
//     env(m) = rfft(lifter(irfft(0.5 log(m^2 + 1e-12)))).real             tests/pv_formant_reference.py::envelope; lifter 1 .. 1, 1/2 at nc, 0
//     d      = fmin(fmax(depth, 0), 1)                                     per stream; a NaN is 0, a null table is 1
//     delta  = min(d (env|V| - env|C|), ln 256)                            upper clamp only (+48 dB): a silent voice silences the carrier
//     Y      = C exp(delta)                                                a real gain per bin: bins 0 and 512 stay real by themselves
// The stage has no state across frames, no phase accumulator and no discontinuous decision, so the one-shot kernel splits a stream into
// runs like the plain round trip (vp_k_stft_fused<false, false>, whose skeleton it is: same rounds, same barriers, stft_overlap_add
// unchanged).  depth 0 and voice == carrier give delta = +-0, exp = 1 exactly: the carrier's frame goes through the operations of the
// plain round trip on the same operands and the output has vp_stft_roundtrip's bits (tested).
//
// Seven transforms per frame where the round trip runs two: voice forward, two for its envelope, carrier forward, two for its envelope,
// one back.  The envelopes are work of one wavefront on its own exchange buffer (wave_sync() only); the voice's stays in registers
// (18 of them) while the carrier's frame is transformed.  The transform's and the split's twiddles come from the global tables where they
// are used, as in vp_k_stft_pv_formant (the values are the resident ones, so are the bits).  No LDS beyond stft_lds_base(F, hop).

#define VP_XS_LN256 5.545177444479562         // the gain's upper clamp: +48 dB

// v[e], the lanes' nine bins kb[e] of a real even sequence's samples 0 .. 512 -> the real parts of its forward transform, same layout
// (a written-out copy of vp_stft_formant.inc's pv_even_rfft, which is included behind this file)
__device__ __forceinline__ void xs_even_rfft(double (&v)[9], const int (&kb)[9], bool lane0, int lane, lds_d2 *xb, const FftAddr &L, const d2 *tw1p, const d2 *tw2p, const d2 *ws)
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

// the smoothed log envelope of the frame whose bins are X, at the lane's nine bins, in registers
__device__ __forceinline__ void xs_envelope(double (&v)[9], const RPairs &X, const int (&kb)[9], bool lane0, int lane, int nc, lds_d2 *xb, const FftAddr &L,
                                            const d2 *tw1p, const d2 *tw2p, const d2 *ws)
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        v[2 * q] = 0.5 * log(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q] + 1e-12);
        v[2 * q + 1] = 0.5 * log(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q] + 1e-12);
    }
    v[8] = 0.5 * log(X.hr * X.hr + X.hi * X.hi + 1e-12);                       // lane 0 only
    xs_even_rfft(v, kb, lane0, lane, xb, L, tw1p, tw2p, ws);                    // 1024 c[n], n = kb[e]
#pragma unroll
    for (int e = 0; e < 9; e++) v[e] *= (kb[e] < nc ? 1.0 : kb[e] == nc ? 0.5 : 0.0) * (1.0 / 1024.0);
    xs_even_rfft(v, kb, lane0, lane, xb, L, tw1p, tw2p, ws);                    // env[k], k = kb[e]
}

// Y = C exp(min(d (ev - ec), ln 256)) on the lane's pairs: ev in registers, ec computed here from the carrier's bins
__device__ __forceinline__ void xs_stage(RPairs &X, const double (&ev)[9], double d, const int (&kb)[9], bool lane0, int lane, int nc, lds_d2 *xb, const FftAddr &L,
                                         const d2 *tw1p, const d2 *tw2p, const d2 *ws)
{
    double g[9];
    xs_envelope(g, X, kb, lane0, lane, nc, xb, L, tw1p, tw2p, ws);
#pragma unroll
    for (int e = 0; e < 9; e++) g[e] = exp(fmin(d * (ev[e] - g[e]), VP_XS_LN256));
#pragma unroll
    for (int q = 0; q < 4; q++) {
        X.kr[q] *= g[2 * q]; X.ki[q] *= g[2 * q];
        X.mr[q] *= g[2 * q + 1]; X.mi[q] *= g[2 * q + 1];
    }
    X.hr *= g[8]; X.hi *= g[8];
}

// the stream's depth as the stage uses it
__device__ __forceinline__ double xs_depth(const double *depthTab, int s) { return depthTab ? fmin(fmax(depthTab[s], 0.0), 1.0) : 1.0; }

// ---- one-shot: A.in is the carrier [S][T], voice [S][T] beside it (A.aligned holds for both), depthTab [S] or null, nc the lifter length
__global__ __launch_bounds__(64 * NWV) void vp_k_stft_cross(VpStftArgs A, const float *voice, const double *depthTab, int nc)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    const int F = A.F, hop = A.hop, T = A.T;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;                                    // this wavefront's exchange buffer ...
    lds_f32 *slots = (lds_f32 *)smem;                                          // ... whose first F floats double as its output slot (slot w at w * 2048)
    lds_f32 *carry = (lds_f32 *)smem + NWV * 2048;                             // [(O - 1) hop]
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)(stft_lds_base(F, hop) / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
    __syncthreads();
#endif

    FftAddr L;
    fft_addr_init(L, lane);
    const d2 *tw1p = (const d2 *)A.tw1 + lane * 8, *tw2p = (const d2 *)A.tw2 + lane * 8;
    d2 wa[8];                                                                  // (w[2n], w[2n + 1]), n = lane + 64 r
#pragma unroll
    for (int r = 0; r < 8; r++) wa[r] = ((const d2 *)A.win)[lane + 64 * r];
    const d2 *ws = (const d2 *)A.tws + lane * 4;                               // W_1024^(64 q + lane), from the global table
    const bool lane0 = lane == 0;
    const double depth = xs_depth(depthTab, s);
    int kb[9];                                                                 // the lane's bins: k = 64 q + lane and 512 - k; lane 0 also 256
#pragma unroll
    for (int q = 0; q < 4; q++) { kb[2 * q] = 64 * q + lane; kb[2 * q + 1] = 512 - kb[2 * q]; }
    kb[8] = 256;

    for (int i = tid; i < F - hop; i += 64 * NWV) carry[i] = 0.f;
    __syncthreads();

    const StftRun R = stft_run(A, run);
    const float *cs = A.in + (size_t)s * T, *vs = voice + (size_t)s * T;
    // both frames' samples are requested a round ahead
    f2 xv[8], xc[8];
    auto request = [&](int rd_) {
        const int f_ = rd_ * NWV + wv;
        if (rd_ < R.r1 && f_ < A.nFrames) {
            stft_load_frame(xv, vs + (size_t)f_ * hop, A.aligned, lane);
            stft_load_frame(xc, cs + (size_t)f_ * hop, A.aligned, lane);
        }
    };
    request(R.r0);
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        C8 z, zc;
        RPairs X;
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; r++) {
                z.re[r] = (double)xv[r].x * wa[r].x; z.im[r] = (double)xv[r].y * wa[r].y;
                zc.re[r] = (double)xc[r].x * wa[r].x; zc.im[r] = (double)xc[r].y * wa[r].y;
            }
        }
        request(rd + 1);
        lds_f2 *slot = (lds_f2 *)(slots + wv * 2048);
        if (live) {
            double ev[9];
            fft512_rx(z, xb, L, tw1p, tw2p);                                   // the voice: its envelope is all that is kept of it
            rfft_split(z, xb, lane, ws, X);
            xs_envelope(ev, X, kb, lane0, lane, nc, xb, L, tw1p, tw2p, ws);
            fft512_rx(zc, xb, L, tw1p, tw2p);                                  // the carrier
            rfft_split(zc, xb, lane, ws, X);
            xs_stage(X, ev, depth, kb, lane0, lane, nc, xb, L, tw1p, tw2p, ws);
            // ---- merge, inverse transform, window: the plain round trip's
            rfft_merge_conj(zc, xb, lane, ws, X, A.c);
            fft512_rx(zc, xb, L, tw1p, tw2p);
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f2{(float)(zc.re[r] * wa[r].x), (float)(-(zc.im[r] * wa[r].y))};
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f2{0.f, 0.f};
        }
        __syncthreads();
        stft_overlap_add(A, slots, carry, s, rd, rd >= R.rFirst, tid);
        __syncthreads();
    }
}

// ---- streaming: one workgroup per stream and call.  The call's bookkeeping (frames by their global index, ring, emit, history
// write-back) is the pv_call_* helpers of vp_stft.hip, with two input histories and no phase arrays; the stage is the one-shot's, so the
// outputs agree bit for bit.
// LDS: four exchange buffers / output slots, ring, voice history, carrier history = 56 KB
__host__ __device__ constexpr size_t xs_stream_lds_bytes() { return (size_t)NWV * 8192 + (VP_PV_RING + 2 * 1024) * sizeof(float); }

// whether one of the call's pending resets concerns stream s
__device__ __forceinline__ bool xs_scan_updates(const VpXsArgs &A, int s)
{
    bool rst = false;
    for (int i = 0; i < A.nUpd; i++)
        if ((A.upd[i].stream == s || A.upd[i].stream == -1) && A.upd[i].reset) rst = true;
    return rst;
}

__global__ __launch_bounds__(64 * NWV) void vp_k_xs_stream(VpXsArgs A)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x;
    constexpr int F = 1024;
    const int hop = A.hop, NB = A.N, S = A.S;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;                                          // wavefront w's output frame at w * 2048
    lds_f32 *ring = (lds_f32 *)smem + NWV * 2048;                              // [VP_PV_RING]
    lds_f32 *histV = ring + VP_PV_RING, *histC = histV + F;                    // [F] each
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)(xs_stream_lds_bytes() / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
    __syncthreads();
#endif
    unsigned char *rec = A.state + (size_t)s * VP_XS_REC_BYTES;
    float *recV = (float *)(rec + VP_XS_VOICE_BYTES), *recC = (float *)(rec + VP_XS_CARRIER_BYTES), *recCarry = (float *)(rec + VP_XS_CARRY_BYTES);

    long long n = *(const long long *)rec;                                     // samples received before this call
    const bool rst = xs_scan_updates(A, s);
    if (rst) n = 0;
    const PvCall C = pv_call_geometry(n, A.nBlocks * NB, hop, A.L);
    const int nf = C.nf;

    // state -> LDS (a reset stream starts from zeros)
    pv_call_load_hist(C, histV, recV, tid);
    pv_call_load_hist(C, histC, recC, tid);
    pv_call_load_ring(C, ring, recCarry, rst, tid);

    FftAddr Lf;
    fft_addr_init(Lf, lane);
    const d2 *tw1p = (const d2 *)A.tw1 + lane * 8, *tw2p = (const d2 *)A.tw2 + lane * 8;
    d2 wa[8];
#pragma unroll
    for (int r = 0; r < 8; r++) wa[r] = ((const d2 *)A.win)[lane + 64 * r];
    const d2 *ws = (const d2 *)A.tws + lane * 4;
    const bool lane0 = lane == 0;
    const double depth = xs_depth(A.depth, s);
    const int nc = A.nc;
    int kb[9];
#pragma unroll
    for (int q = 0; q < 4; q++) { kb[2 * q] = 64 * q + lane; kb[2 * q + 1] = 512 - kb[2 * q]; }
    kb[8] = 256;
    __syncthreads();

    const float *vs = A.voice + (size_t)s * NB, *cs = A.carrier + (size_t)s * NB;
    float *ys = A.out + (size_t)s * NB;
    const int nRounds = pv_call_rounds(C);
    int cb = C.er;                                                             // next relative index to emit (uniform)
    f2 xv[8], xc[8];
    auto request = [&](int k_) {
        const int fr_ = C.fr0 + NWV * k_ + wv;
        if (k_ < nRounds && fr_ >= 0 && fr_ < nf) {
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int rel = fr_ * hop + 2 * (lane + 64 * r);
                xv[r] = f2{pv_call_sample(C, histV, vs, NB, S, rel), pv_call_sample(C, histV, vs, NB, S, rel + 1)};
                xc[r] = f2{pv_call_sample(C, histC, cs, NB, S, rel), pv_call_sample(C, histC, cs, NB, S, rel + 1)};
            }
        }
    };
    request(0);
    for (int k = 0; k < nRounds; k++) {
        const int frW0 = C.fr0 + NWV * k;                                      // relative frame of wavefront 0 in this round
        const int fr = frW0 + wv;
        const bool live = fr >= 0 && fr < nf;                                  // (wavefront-uniform)
        const int wFirst = max(0, -frW0), wLast = min(NWV - 1, nf - 1 - frW0);
        C8 z, zc;
        RPairs X;
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; r++) {
                z.re[r] = (double)xv[r].x * wa[r].x; z.im[r] = (double)xv[r].y * wa[r].y;
                zc.re[r] = (double)xc[r].x * wa[r].x; zc.im[r] = (double)xc[r].y * wa[r].y;
            }
        }
        request(k + 1);
        lds_f2 *slot = (lds_f2 *)(slots + wv * 2048);
        if (live) {
            double ev[9];
            fft512_rx(z, xb, Lf, tw1p, tw2p);
            rfft_split(z, xb, lane, ws, X);
            xs_envelope(ev, X, kb, lane0, lane, nc, xb, Lf, tw1p, tw2p, ws);
            fft512_rx(zc, xb, Lf, tw1p, tw2p);
            rfft_split(zc, xb, lane, ws, X);
            xs_stage(X, ev, depth, kb, lane0, lane, nc, xb, Lf, tw1p, tw2p, ws);
            rfft_merge_conj(zc, xb, lane, ws, X, A.c);
            fft512_rx(zc, xb, Lf, tw1p, tw2p);
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f2{(float)(zc.re[r] * wa[r].x), (float)(-(zc.im[r] * wa[r].y))};
        }
        __syncthreads();
        cb = pv_call_round_tail(C, ring, slots, ys, NB, S, hop, frW0, wFirst, wLast, cb, tid);
        __syncthreads();
    }
    pv_call_emit(C, ring, ys, NB, S, cb, C.er + C.M, tid);                     // the flush

    // LDS -> state
    pv_call_store_hist(C, recV, histV, vs, NB, S, hop, tid);
    pv_call_store_hist(C, recC, histC, cs, NB, S, hop, tid);
    pv_call_store_carry(C, recCarry, ring, tid);
    if (tid == 0) *(long long *)rec = C.R;
}

// the pending resets alone (a call with more than VP_PV_MAX_UPDATES of them enqueues this first, on the same stream)
__global__ __launch_bounds__(256) void vp_k_xs_update(VpXsArgs A)
{
    const int s = blockIdx.x;
    unsigned char *rec = A.state + (size_t)s * VP_XS_REC_BYTES;
    if (!xs_scan_updates(A, s)) return;
    float *recCarry = (float *)(rec + VP_XS_CARRY_BYTES);
    for (int i = threadIdx.x; i < 1024; i += 256) recCarry[i] = 0.f;
    if (threadIdx.x == 0) *(long long *)rec = 0;
}

size_t vp_xs_lds_bytes() { return xs_stream_lds_bytes(); }

// (1024-point frames only: the caller's test; a.in is the carrier)
hipError_t vp_stft_launch_cross(const VpStftArgs &a, const float *d_voice, const double *d_depth, int nc, int nStreams, int nRuns, hipStream_t st)
{
    const dim3 grid(nRuns, nStreams), block(64 * NWV);
    hipLaunchKernelGGL(vp_k_stft_cross, grid, block, vp_stft_lds_bytes(a.F, a.hop, 0), st, a, d_voice, d_depth, nc);
    return hipGetLastError();
}

hipError_t vp_xs_launch(const VpXsArgs &a, hipStream_t st)
{
    if (a.nBlocks == 0) hipLaunchKernelGGL(vp_k_xs_update, dim3(a.S), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(vp_k_xs_stream, dim3(a.S), dim3(64 * NWV), vp_xs_lds_bytes(), st, a);
    return hipGetLastError();
}
